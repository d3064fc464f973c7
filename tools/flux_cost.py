"""Cost of the sampled fluxes on one GPU: the per-sample kernel time (kernel class "fields": k_moments_accum<2> +
k_slab_reduce<unsigned long long, sample_sink>, timed on the dispatch like every other class) beside a sample of the fields on the same grid in the same
process, and the overhead of run(100) with a flux sample every 10 steps against run(100) without sampling.  Prints one JSON
line per workload.

    python tools/flux_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim, sample_us

from argon_monte_carlo_amd import fields as FL
from argon_monte_carlo_amd import fluxes as FX


def measure(kind, n, reps, steps=100, every=10, samples=50):
    sim = make_sim(kind, n)
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
