"""Cost of the sampled correlations on one GPU: the per-sample kernel time of a lag sample and of an origin
sample (kernel class "fields": k_corr_accum<MODE> + k_slab_reduce<unsigned long long, sample_sink>, timed on the dispatch like every other class), the traffic
floor beside them, and the overhead of run(100) with a sample every 10 steps and 8 lags against run(100) without sampling.
Prints one JSON line per workload.

    python tools/corr_cost.py [--reps 5]
"""
import argparse
import json
import statistics
import time

from cost_common import WORKLOADS, make_sim

from argon_monte_carlo_amd import correlations as CO

HBM_BYTES_PER_US = 6.29e6               # measured float4-copy bandwidth of the MI355X (6.29 TB/s)


def _sample_us(sim, g, n_lags, samples):
    """Kernel time per sample of a window of ``n_lags`` lags: with n_lags = 2^16 - 1 every timed sample is a plain lag
    sample, with n_lags = 1 every one is the lag-and-origin pass."""
    sim.enable_correlations(g, n_lags=n_lags)
    for _ in range(5):
        sim.correlations_sample()
    sim.engine.synchronize()
    sim.engine.profile(True)
    for _ in range(samples):
        sim.correlations_sample()
    sim.engine.synchronize()
    ms, launches = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    sim.engine.corr_read()              # (no particle may have left the quantisers' range: the kernels did the whole work)
    return 1e3 * ms / (launches / 2)


def measure(kind, n, reps, steps=100, every=10, n_lags=8, samples=50):
    sim = make_sim(kind, n)
    g = CO.default_grid(sim.params)
    groups = CO.grid_groups(g)
    # 1. one sample, kernel time on the dispatch (the state stands still: every displacement is zero)
    lag_us = _sample_us(sim, g, (65536 // groups) - 1, samples)
    origin_us = _sample_us(sim, g, 1, samples)
    # 2. run(steps) with and without a sample every `every` steps, alternating
    sim.disable_correlations()
    sim.run(10)
    t_off, t_on = [], []
    for _ in range(reps):
        for on in (False, True):
            if on:
                sim.enable_correlations(g, every=every, n_lags=n_lags)
            else:
                sim.disable_correlations()
            t0 = time.perf_counter()
            sim.run(steps)
            (t_on if on else t_off).append(time.perf_counter() - t0)
    off, on = statistics.median(t_off), statistics.median(t_on)
    sim.close()
    return {"workload": f"{kind}_{n:.0e}".replace("+0", ""), "grid": [g.n1, g.n2, g.n3], "groups": groups,
            "lag_sample_us": round(lag_us, 2), "lag_and_origin_sample_us": round(origin_us, 2),
            "floor_lag_us": round(96.0 * n / HBM_BYTES_PER_US, 2), "floor_lag_and_origin_us": round(144.0 * n / HBM_BYTES_PER_US, 2),
            "run_ms_off": round(1e3 * off, 3), "run_ms_on": round(1e3 * on, 3), "run_ms_off_spread": [round(1e3 * min(t_off), 3), round(1e3 * max(t_off), 3)],
            "every": every, "n_lags": n_lags, "steps": steps, "overhead_pct": round(100.0 * (on - off) / off, 2), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    for kind, n in WORKLOADS:
        print(json.dumps(measure(kind, n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
