"""Cost of the sampled fields on one GPU: the per-sample kernel time (kernel class "fields": k_moments_accum<1> +
k_slab_reduce<unsigned long long, sample_sink>, timed on the dispatch like every other class) and the overhead of run(100) with a sample every 10 steps
against run(100) without sampling.  Prints one JSON line per workload.

    python tools/fields_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim

from argon_monte_carlo_amd import fields as FL


def measure(kind, n, reps, steps=100, every=10, samples=50):
    sim = make_sim(kind, n)
    g = FL.default_grid(sim.params)
    # 1. one sample, kernel time on the dispatch
    sim.enable_fields(g)
    for _ in range(5):
        sim.fields_sample()
    sim.engine.synchronize()
    sim.engine.profile(True)
    for _ in range(samples):
        sim.fields_sample()
    sim.engine.synchronize()
    ms, launches = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    per_sample_us = 1e3 * ms / (launches / 2)
    # 2. run(steps) with and without a sample every `every` steps, alternating
    sim.run(10)
    t_off, t_on = [], []
    for _ in range(reps):
        for on in (False, True):
            if on:
                sim.enable_fields(g, every=every)
            else:
                sim.disable_fields()
            t0 = time.perf_counter()
            sim.run(steps)
            (t_on if on else t_off).append(time.perf_counter() - t0)
    off, on = statistics.median(t_off), statistics.median(t_on)
    sim.close()
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "grid": [g.n1, g.n2, g.n3], "bins": FL.grid_bins(g),
            "sample_us": round(per_sample_us, 2), "run_ms_off": round(1e3 * off, 3), "run_ms_on": round(1e3 * on, 3),
            "every": every, "steps": steps, "overhead_pct": round(100.0 * (on - off) / off, 2), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
