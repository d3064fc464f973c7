"""Cost of a many-step run of the energised pore in device-RNG mode on one GPU: microseconds per step of
``TemperatureSimulation(device_rng_seed=...).run(200)`` at N = 1e6 (median of the repeats, after a warm-up run), and the
kernel-class times of a separate, profiled run.  It calls nothing but ``sim.run``, so it measures whatever that is: the
host-free run (AMC_TEMP_RUN_UNFUSED=1: with the single step's three streaming passes), or a loop of steps.  One JSON line.

    python tools/temp_run_cost.py [--reps 5] [--steps 200] [--n 1000000] [--surface] [--wall-law maxwell]

--surface samples the surfaces on the default grid in every step of every run.
--wall-law sets the wall law of the run (default: none is set, the reference law).

AMC_COST_TREE=<directory> measures the package of another checkout (an earlier commit, built there) with this same script.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("AMC_COST_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd.sim import TemperatureSimulation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--label", default="")
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--wall-law", default=None)
    a = ap.parse_args()
    sim = TemperatureSimulation(n=a.n, device_rng_seed=17)
    sim.set_state(*IC.pore_ic(sim.params, sim.consts, seed=17))        # the benchmark's initial conditions
    if a.surface:
        sim.enable_surface()
    if a.wall_law:
        sim.set_wall_law(a.wall_law)
    sim.run(20)                                                         # warm-up (allocations, first launches)
    sim.engine.synchronize()
    times = []
    for _ in range(max(a.reps, 5)):
        t0 = time.perf_counter()
        sim.run(a.steps)
        sim.engine.synchronize()
        times.append(1e6 * (time.perf_counter() - t0) / a.steps)
    # kernel classes, timed on the dispatch, in a run of their own (the events cost time themselves)
    sim.engine.profile(True)
    sim.run(a.steps)
    kt = sim.engine.kernel_times()
    sim.engine.profile(False)
    classes = {k: round(1e3 * ms / a.steps, 2) for k, (ms, cnt) in kt.items() if cnt}
    form = "loop of timesteps"
    if hasattr(sim.engine, "temp_run_device"):
        form = "run, single step's passes" if os.environ.get("AMC_TEMP_RUN_UNFUSED", "0") not in ("", "0") else "run"
    print(json.dumps(dict(workload="temp_device_rng", label=a.label, form=form, n=a.n, steps=a.steps, reps=len(times),
                          us_per_step_median=round(statistics.median(times), 2), us_per_step_min=round(min(times), 2),
                          us_per_step_max=round(max(times), 2), kernel_us_per_step=classes,
                          steps_done=sim.steps_done, surface=bool(a.surface), wall_law=a.wall_law or "unset")))
    sim.close()


if __name__ == "__main__":
    main()
