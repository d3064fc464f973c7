"""Cost of the sampled pair distribution on one GPU: the kernel time of one sample (kernel class "fields": the six
kernels k_pair_file, k_pair_scan_sums, k_pair_scan, k_pair_scatter, k_pair_count, k_slab_reduce<unsigned long long, pair_sink>, timed on the dispatch like every other class) on
the default grid, on a standing state, beside the time of a step at the same size (run(200) without a sampler) and the pair tests
a sample makes (from its totals); and the time of a sample on a grid at the cap of 128 cells per axis that holds few particles
(what the cells cost, not the pairs).  Prints one JSON line per workload.

    python tools/pair_cost.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import pairs as PA  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.sim import Simulation  # noqa: E402

WORKLOADS = [("cube", 100_000), ("pore", 1_000_000)]
LAUNCHES = 6


def sample_us(sim, samples):
    """kernel time of one sample (six launches), microseconds"""
    for _ in range(3):
        sim.pairs_sample()
    sim.engine.synchronize()
    sim.engine.profile(True)
    ms0, launches0 = sim.engine.kernel_times()["fields"]       # (the class's times accumulate over the context's life)
    for _ in range(samples):
        sim.pairs_sample()
    sim.engine.synchronize()
    ms, launches = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    return 1e3 * (ms - ms0) / ((launches - launches0) / LAUNCHES)


def measure(kind, n, reps, steps=200, samples=20):
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
    g = PA.default_grid(sim.params)
    sim.run(10)
    sim.enable_pairs(g)
    us = [sample_us(sim, samples) for _ in range(reps)]
    sim.pairs_reset()
    sim.pairs_sample()
    d = sim.pairs()
    sim.disable_pairs()
    step = []
    for _ in range(reps):
        t0 = time.perf_counter()
        sim.run(steps)
        step.append(1e6 * (time.perf_counter() - t0) / steps)
    sim.close()
    lo, hi, cells, edge = PA.search_box(g)
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "grid": [g.n1, g.n2, g.n3], "hist_bins": int(g.hist_bins), "r_max": g.r_max,
            "cells": cells, "cell_edge_over_r_max": [round(e / g.r_max, 4) for e in edge],
            "pair_sample_us": round(statistics.median(us), 1), "pair_sample_us_takes": [round(v, 1) for v in us],
            "step_us": round(statistics.median(step), 2), "step_us_takes": [round(v, 2) for v in step],
            "sample_over_step": round(statistics.median(us) / statistics.median(step), 2),
            "centres": int(d["centres"].sum()), "ordered_pairs_within_r_max": int(d["pairs"].sum()), "n_outside": d["n_outside"],
            "n_unfiled": d["n_unfiled"], "overlap_per_centre": [float(v) for v in d["overlap_per_centre"]],
            "approach_fraction_below_d": float(d["approaching"][:, :2].sum() / max(1, d["pairs"][:, :2].sum())), "reps": reps}


def measure_cap(reps, n=2400, samples=10):
    """a cube context with n particles uniform in the cube and r_max = edge / 200: 128 x 128 x 128 cells, nearly all empty"""
    import numpy as np
    p, c = PR.cube_params(n=n)
    sim = Simulation("cube", params=p, consts=c)
    rng = np.random.RandomState(8)
    pos = rng.uniform(0.0, p.cube_x, size=(3, n))
    v = rng.normal(size=(3, n)) * 300.0
    sim.set_state(pos[0].copy(), pos[1].copy(), pos[2].copy(), v[0].copy(), v[1].copy(), v[2].copy())
    g = PA.make_grid("cartesian", (1, 1, 1), (0, 0, 0), (p.cube_x, p.cube_y, p.cube_z), p.cube_x / 200.0, hist_bins=32)
    sim.enable_pairs(g)
    us = [sample_us(sim, samples) for _ in range(reps)]
    sim.close()
    return {"workload": f"cube_{n}_at_the_cell_cap", "cells": PA.search_box(g)[2], "pair_sample_us": round(statistics.median(us), 1),
            "pair_sample_us_takes": [round(v, 1) for v in us], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps)), flush=True)
    print(json.dumps(measure_cap(args.reps)), flush=True)


if __name__ == "__main__":
    main()
