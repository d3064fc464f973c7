"""What the samplers' cost scripts (tools/*_cost.py) share: the benchmark's workloads and set-up, the kernel time of one sample,
and a summary of several takes.  Importing it puts the repository on the path."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from argon_monte_carlo_amd import ic as IC  # noqa: E402
from argon_monte_carlo_amd import params as PR  # noqa: E402
from argon_monte_carlo_amd.sim import Simulation  # noqa: E402

WORKLOADS = [("pore", 1_000_000), ("cube", 100_000)]


def make_sim(kind, n, keep_paths=False):
    """The benchmark's set-up (bench.py make_workload): count-and-continue on a degenerate solve, histograms only
    (``keep_paths``: with the path records on)."""
    if kind == "cube":
        p, c = PR.cube_params_for_n(n)
        init = IC.cube_ic(p, c, seed=127)
    else:
        p, c = PR.pore_params(n=n)
        init = IC.pore_ic(p, c, seed=17)
    p.reserved1 = 1
    if not keep_paths:
        p.max_paths = -1
    sim = Simulation(kind, params=p, consts=c)
    sim.set_state(*init)
    return sim


def sample_us(sim, sample, samples, launches=2, warmup=5):
    """kernel time of one sample (``launches`` launches of the kernel class "fields"), microseconds"""
    for _ in range(warmup):
        sample()
    sim.engine.synchronize()
    sim.engine.profile(True)
    ms0, launches0 = sim.engine.kernel_times()["fields"]       # (the class's times accumulate over the context's life)
    for _ in range(samples):
        sample()
    sim.engine.synchronize()
    ms, launches1 = sim.engine.kernel_times()["fields"]
    sim.engine.profile(False)
    return 1e3 * (ms - ms0) / ((launches1 - launches0) / launches)


def spread(v, digits):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
