"""Cost of the sampled transits on one GPU: the per-sample kernel time (kernel class "fields": k_transit_accum +
k_slab_reduce<unsigned long long, transit_sink>, timed on the dispatch like every other class) on the default zones beside a sample of the velocity
distributions and one of the fields on THEIR default grids, on the same state in the same process, alternated; and run(200)
with the transits at every = 1, with the fields at every = 1 (both force the same plain loop) and with no sampler, alternated.
Five takes of everything: median, minimum and maximum.  Prints one JSON line per workload.

    python tools/transit_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim, sample_us, spread

from argon_monte_carlo_amd import transits as TR


def measure(kind, n, reps, steps=200, samples=50):
    sim = make_sim(kind, n)
    g = TR.default_grid(sim.params)
    sim.run(10)
    # 1. one sample of the transits, of the distributions and of the fields, each on its default grid, kernel time on the
    #    dispatch, alternated.  (The transits' samples of one unchanged state: the first sees everybody for the first time, the
    #    warm-up takes it; the others are the common path, no events.  The run below has the events.)
    tr_us, vdf_us, fields_us = [], [], []
    for _ in range(reps):
        sim.enable_transits(g, every=0)
        tr_us.append(sample_us(sim, sim.transits_sample, samples))
        sim.disable_transits()
        sim.enable_distributions()
        vdf_us.append(sample_us(sim, sim.distributions_sample, samples))
        sim.disable_distributions()
        sim.enable_fields()
        fields_us.append(sample_us(sim, sim.fields_sample, samples))
        sim.disable_fields()
    # 2. run(steps) with the transits, with the fields (each after every step) and with no sampler, alternating
    t = {"off": [], "transits": [], "fields": []}
    events = 0
    for _ in range(reps):
        for which in ("off", "transits", "fields"):
            if which == "transits":
                sim.enable_transits(g, every=1)
            elif which == "fields":
                sim.enable_fields(every=1)
            t0 = time.perf_counter()
            sim.run(steps)
            sim.engine.synchronize()
            t[which].append(1e3 * (time.perf_counter() - t0))
            if which == "transits":
                d = sim.transits()
                events = int(d["entries"].sum() + d["count"].sum() + d["skipped"].sum())
                sim.disable_transits()
            elif which == "fields":
                sim.disable_fields()
    sim.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "zones": TR.zones(g), "reps": reps, "steps": steps,
            "transit_sample_us": spread(tr_us, 2), "vdf_sample_us_default_grid": spread(vdf_us, 2),
            "fields_sample_us_default_grid": spread(fields_us, 2),
            "ratio_to_vdf": round(statistics.median(tr_us) / statistics.median(vdf_us), 3),
            "ratio_to_fields": round(statistics.median(tr_us) / statistics.median(fields_us), 3),
            "run_ms_off": spread(t["off"], 3), "run_ms_transits_every_1": spread(t["transits"], 3),
            "run_ms_fields_every_1": spread(t["fields"], 3),
            "us_per_step_off": round(1e3 * med["off"] / steps, 2), "us_per_step_transits": round(1e3 * med["transits"] / steps, 2),
            "us_per_step_fields": round(1e3 * med["fields"] / steps, 2),
            "events_in_last_transit_run": events}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
