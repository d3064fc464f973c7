"""Cost of the sampled velocity distributions on one GPU: the per-sample kernel time (kernel class "fields":
k_vdf_accum + k_slab_reduce<unsigned int, vdf_sink>, timed on the dispatch like every other class) on the default grid beside a sample of the fields and
one of the fluxes on THEIR default grids, on the same state in the same process, and the overhead of run(100) with a sample of
the distributions every 10 steps against run(100) without sampling.  Prints one JSON line per workload.

    python tools/vdf_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim, sample_us

from argon_monte_carlo_amd import distributions as VD


def measure(kind, n, reps, steps=100, every=10, samples=50):
    sim = make_sim(kind, n)
    g = VD.default_grid(sim.params)
    # 1. one sample of the distributions, of the fields and of the fluxes, each on its default grid, kernel time on the dispatch,
    #    alternated
    vdf_us, fields_us, flux_us = [], [], []
    for _ in range(3):
        sim.enable_distributions(g)
        vdf_us.append(sample_us(sim, sim.distributions_sample, samples))
        sim.disable_distributions()
        sim.enable_fields()
        fields_us.append(sample_us(sim, sim.fields_sample, samples))
        sim.disable_fields()
        sim.enable_fluxes()
        flux_us.append(sample_us(sim, sim.fluxes_sample, samples))
        sim.disable_fluxes()
    # 2. run(steps) with and without a sample of the distributions every `every` steps, alternating
    sim.run(10)
    t_off, t_on = [], []
    for _ in range(reps):
        for on in (False, True):
            if on:
                sim.enable_distributions(g, every=every)
            else:
                sim.disable_distributions()
            t0 = time.perf_counter()
            sim.run(steps)
            (t_on if on else t_off).append(time.perf_counter() - t0)
    off, on = statistics.median(t_off), statistics.median(t_on)
    sim.close()
    vd, fl, fx = statistics.median(vdf_us), statistics.median(fields_us), statistics.median(flux_us)
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "grid": [g.n1, g.n2, g.n3], "regions": VD.grid_bins(g), "hist_bins": int(g.hist_bins),
            "columns": VD.grid_bins(g) * VD.columns(g.hist_bins),
            "vdf_sample_us": round(vd, 2), "fields_sample_us_default_grid": round(fl, 2), "flux_sample_us_default_grid": round(fx, 2),
            "ratio_to_fields": round(vd / fl, 3), "ratio_to_flux": round(vd / fx, 3),
            "vdf_sample_us_takes": [round(v, 2) for v in vdf_us], "fields_sample_us_takes": [round(v, 2) for v in fields_us],
            "flux_sample_us_takes": [round(v, 2) for v in flux_us],
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
