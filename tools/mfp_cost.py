"""Cost of the sampled free paths on one GPU: the per-step time of run(200) without a sampler, with the
sampled fields at cadence 1 and with the sampled free paths — the last two force the same plain loop, every step ending with
its own bounds pass — and the sampler's own kernel time (kernel class "fields": k_mfp_accum, timed on the dispatch like every
other class).  Median of ``--reps`` runs per setting, the settings alternated.  Prints one JSON line per workload.

    python tools/mfp_cost.py [--reps 5] [--steps 200]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim

SETTINGS = ("none", "fields_every_1", "free_paths")


def configure(sim, setting):
    sim.disable_fields()
    sim.disable_free_paths()
    if setting == "fields_every_1":
        sim.enable_fields(every=1)
    elif setting == "free_paths":
        sim.enable_free_paths()


def measure(kind, n, reps, steps):
    sim = make_sim(kind, n, keep_paths=True)    # with the path records on: the sampler reads them
    sim.run(steps)                             # warm-up: every particle has a collision behind it, paths complete
    times = {s: [] for s in SETTINGS}
    for _ in range(reps):
        for s in SETTINGS:
            configure(sim, s)
            sim.engine.drain_paths(sort=False)  # (an empty record buffer for every take)
            sim.engine.synchronize()
            t0 = time.perf_counter()
            sim.run(steps)
            times[s].append(time.perf_counter() - t0)
    # the sampler's kernel alone, on the dispatch
    configure(sim, "free_paths")
    sim.engine.synchronize()
    sim.engine.profile(True)
    ms0, launches0 = sim.engine.kernel_times()["fields"]
    sim.run(steps)
    ms, launches = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    f = sim.free_paths()
    sim.close()
    us = {s: 1e6 * statistics.median(v) / steps for s, v in times.items()}
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "steps": steps, "reps": reps,
            "us_per_step": {s: round(v, 2) for s, v in us.items()},
            "us_per_step_takes": {s: [round(1e6 * t / steps, 2) for t in v] for s, v in times.items()},
            "free_paths_minus_fields_us": round(us["free_paths"] - us["fields_every_1"], 2),
            "k_mfp_accum_us": round(1e3 * (ms - ms0) / max(1, launches - launches0), 2), "k_mfp_accum_launches": launches - launches0,
            "paths_per_step": round(f["n_records"] / max(1, f["n_steps"]), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps, args.steps)), flush=True)


if __name__ == "__main__":
    main()
