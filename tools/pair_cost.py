"""Cost of the sampled pair distribution on one GPU: the kernel time of one sample (kernel class "fields": the six
kernels k_pair_file, k_pair_scan_sums, k_pair_scan, k_pair_scatter, k_pair_count, k_slab_reduce<unsigned long long, pair_sink>, timed on the dispatch like every other class) on
the default grid, on a standing state, beside the time of a step at the same size (run(200) without a sampler) and the pair tests
a sample makes (from its totals); and the time of a sample on a grid at the cap of 128 cells per axis that holds few particles
(what the cells cost, not the pairs).  Prints one JSON line per workload.

    python tools/pair_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

import cost_common
from cost_common import make_sim

from argon_monte_carlo_amd import pairs as PA
from argon_monte_carlo_amd import params as PR
from argon_monte_carlo_amd.sim import Simulation

WORKLOADS = cost_common.WORKLOADS[::-1]         # the cube first


def sample_us(sim, samples):
    """kernel time of one sample (six launches, three samples of warm-up), microseconds"""
    return cost_common.sample_us(sim, sim.pairs_sample, samples, launches=6, warmup=3)


def measure(kind, n, reps, steps=200, samples=20):
    sim = make_sim(kind, n)
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
