"""The cadence mix of the tests that run every sampler together (tests/test_gpu_samplers_together.py), and the rule of a cadence
in plain Python.  Steps count from 1: step s is the one that leaves the context's step counter at s, and a sample of a sampler
with (every, step_offset) is due after it when (s + step_offset) % every == 0 — amc_cadence_due of the library's host code."""

STEPS = 24
N_LAGS = 2                  # the correlations' window: an origin, then two lags
# sampler -> (every, step_offset), the six samplers that run on a cadence (the free paths and the surfaces sample every step)
MIX = {
    "fields": (4, 0),
    "correlations": (6, 0),
    "fluxes": (5, 2),
    "distributions": (7, 1),
    "transits": (3, 1),
    "pairs": (9, 0),
}
# D: some sampler is due after the step (it ends with its own bounds pass in the pore), N: nobody is (inside a run the pass is
# left to the next step's).  All four transitions D->D, D->N, N->D and N->N occur; three samplers are due together after the
# steps 8, 18 and 20.
PATTERN = "NDDDDDNDDNDDDDNDDDNDNNDD"


def due(every, step_offset, step, on=True):
    """a sample is due after step ``step`` (1, 2, ...)"""
    return bool(on) and every > 0 and (step + step_offset) % every == 0


def due_steps(name, first=1, last=STEPS, mix=None):
    """the steps first .. last after which ``name`` samples"""
    every, offset = (MIX if mix is None else mix)[name]
    return [s for s in range(first, last + 1) if due(every, offset, s)]


def due_names(step, mix=None):
    """the samplers due after ``step``, in the mix's order"""
    m = MIX if mix is None else mix
    return [name for name, (every, offset) in m.items() if due(every, offset, step)]


def pattern(steps=STEPS, mix=None):
    return "".join("D" if due_names(s, mix) else "N" for s in range(1, steps + 1))
