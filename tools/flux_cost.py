"""Cost of the sampled fluxes on one GPU: the per-sample kernel time (kernel class "fields": k_moments_accum<2> +
k_slab_reduce<unsigned long long, sample_sink>, timed on the dispatch like every other class) beside a sample of the fields on the same grid in the same
process, and the overhead of run(100) with a flux sample every 10 steps against run(100) without sampling.  Prints one JSON
line per workload.

    python tools/flux_cost.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from argon_monte_carlo_amd import fields as FL  # noqa: E402
from argon_monte_carlo_amd import fluxes as FX  # noqa: E402
from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.sim import Simulation  # noqa: E402

WORKLOADS = [("pore", 1_000_000), ("cube", 100_000)]


def sample_us(sim, sample, samples):
    """kernel time of one sample (two launches), microseconds"""
    for _ in range(5):
        sample()
    sim.engine.synchronize()
    sim.engine.profile(True)
    ms0, launches0 = sim.engine.kernel_times()["fields"]       # (the class's times accumulate over the context's life)
    for _ in range(samples):
        sample()
    sim.engine.synchronize()
    ms, launches = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    return 1e3 * (ms - ms0) / ((launches - launches0) / 2)


def measure(kind, n, reps, steps=100, every=10, samples=50):
    # the benchmark's set-up (bench.py make_workload): count-and-continue on a degenerate solve, histograms only
    if kind == "cube":
        p, c = PR.cube_params_for_n(n)
        init = IC.cube_ic(p, c, seed=127)
    else:
        p, c = PR.pore_params(n=n)
        init = IC.pore_ic(p, c, seed=17)
    p.reserved1 = 1
    p.max_paths = -1
    sim = Simulation(kind, params=p, consts=c)
    sim.set_state(*init)
    g = FX.default_grid(sim.params)
    axes = 3 if g.kind == FL.AMC_FIELDS_CARTESIAN else 2
    # 1. one sample of the fluxes and one of the fields on the same grid, kernel time on the dispatch, alternated
    flux_us, fields_us = [], []
    for _ in range(3):
        sim.enable_fluxes(g)
        flux_us.append(sample_us(sim, sim.fluxes_sample, samples))
        sim.disable_fluxes()
        sim.enable_fields(FL.make_grid(g.kind, (g.n1, g.n2, g.n3)[:axes], list(g.lo), list(g.hi)))
        fields_us.append(sample_us(sim, sim.fields_sample, samples))
        sim.disable_fields()
    # 2. run(steps) with and without a flux sample every `every` steps, alternating
    sim.run(10)
    t_off, t_on = [], []
    for _ in range(reps):
        for on in (False, True):
            if on:
                sim.enable_fluxes(g, every=every)
            else:
                sim.disable_fluxes()
            t0 = time.perf_counter()
            sim.run(steps)
            (t_on if on else t_off).append(time.perf_counter() - t0)
    off, on = statistics.median(t_off), statistics.median(t_on)
    sim.close()
    fx, fl = statistics.median(flux_us), statistics.median(fields_us)
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "grid": [g.n1, g.n2, g.n3], "bins": FX.grid_bins(g),
            "flux_sample_us": round(fx, 2), "fields_sample_us_same_grid": round(fl, 2), "ratio": round(fx / fl, 3),
            "flux_sample_us_takes": [round(v, 2) for v in flux_us], "fields_sample_us_takes": [round(v, 2) for v in fields_us],
            "run_ms_off": round(1e3 * off, 3), "run_ms_on": round(1e3 * on, 3), "every": every, "steps": steps,
            "overhead_pct": round(100.0 * (on - off) / off, 2), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
