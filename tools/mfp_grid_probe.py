"""What k_mfp_accum pays for: its time per launch on the pore at N = 1e6 for grids that differ in the number of
atomics per record and in how many records share a cell — one bin to 384 bins, with and without the histogram, and a grid
that lies outside the gas, so that nothing is quantised or added.  Kernel class "fields", timed on the dispatch.  Prints one
JSON line per grid; the records per step grow as the run goes on, so the grids are not at equal load.

    python tools/mfp_grid_probe.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from argon_monte_carlo_amd import free_paths as FP  # noqa: E402
from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.sim import Simulation  # noqa: E402


def main():
    p, c = PR.pore_params(n=1_000_000)
    p.reserved1 = 1
    sim = Simulation("pore", params=p, consts=c)
    sim.set_state(*IC.pore_ic(p, c, seed=17))
    sim.run(200)
    axes = ((0, 0), (p.R_oa, p.H))
    grids = {"default_4x16_h32": FP.default_grid(p),
             "one_bin_h0": FP.make_grid("axisymmetric", (1, 1), *axes, hist_bins=0),
             "one_bin_h32": FP.make_grid("axisymmetric", (1, 1), *axes, hist_bins=32),
             "4x16_h0": FP.make_grid("axisymmetric", (4, 16), *axes, hist_bins=0),
             "8x48_h0": FP.make_grid("axisymmetric", (8, 48), *axes, hist_bins=0),
             "outside_all": FP.make_grid("axisymmetric", (4, 16), (0, p.H * 2), (p.R_oa, p.H * 3), hist_bins=32)}
    for name, g in grids.items():
        sim.enable_free_paths(g)
        sim.run(20)
        sim.engine.synchronize()
        sim.engine.profile(True)
        ms0, l0 = sim.engine.kernel_times()["fields"]
        sim.run(100)
        ms, l1 = sim.engine.kernel_times()["fields"]
        sim.engine.profile(False)
        f = sim.free_paths()
        cnt = f["count"][:, :2].ravel()
        print(json.dumps({"grid": name, "k_mfp_accum_us": round(1e3 * (ms - ms0) / (l1 - l0), 2),
                          "records_per_step": round(f["n_records"] / f["n_steps"], 1), "outside_per_step": round(f["n_outside"] / f["n_steps"], 1),
                          "largest_cell_share": round(float(cnt.max()) / max(1, int(cnt.sum())), 3), "cells_used": int((cnt > 0).sum())}), flush=True)
    sim.close()


if __name__ == "__main__":
    main()
