"""Host-only: the cadence mix of tests/together_states.py keeps the properties the GPU tests of all samplers together rely on —
whatever mix is committed there, so that an edit of it cannot silently empty those tests."""
import os
import re

from tests import together_states as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_due_is_the_library_rule():
    src = open(os.path.join(ROOT, "argon_monte_carlo_amd", "csrc", "amc_host.h")).read()
    m = re.search(r"amc_cadence_due\(bool on, int64_t every, int64_t step_offset, int64_t step\) \{ return (.*?); \}", src)
    assert m and m.group(1) == "on && every > 0 && (step + step_offset) % every == 0", m
    assert TS.due(3, 1, 2) and TS.due(3, 1, 5) and not TS.due(3, 1, 3) and TS.due(1, 0, 7) and TS.due(5, 13, 2)
    assert not TS.due(0, 0, 4) and not TS.due(4, 0, 4, on=False) and not TS.due(4, 0, 0 + 1)


def test_the_mix_has_every_transition_enough_samples_and_a_crowded_step():
    pat = TS.pattern()
    assert len(pat) == TS.STEPS and pat == TS.PATTERN, pat
    pairs = {pat[k:k + 2] for k in range(len(pat) - 1)}
    assert pairs == {"DD", "DN", "ND", "NN"}, pairs                 # all four transitions inside one run
    assert pat[-1] == "D" and pat[0] == "N"                          # the last step is due, the first is not
    assert len(TS.MIX) == 6 and all(every > 0 and offset >= 0 for every, offset in TS.MIX.values())
    for name in TS.MIX:
        assert len(TS.due_steps(name)) >= 2, name                   # nothing compares a single sample
    crowded = [s for s in range(1, TS.STEPS + 1) if len(TS.due_names(s)) >= 3]
    assert crowded, "no step with three samplers due"
    # the split runs and the checkpoint of the GPU tests cut the run where both sides keep due and idle steps
    for cut in (7, 11, 15):
        assert {"D", "N"} <= set(pat[:cut]) and {"D", "N"} <= set(pat[cut:]), cut
    # an offset that matters: at least one cadence whose samples a resumed run without its offset would misplace
    assert any(offset % every for every, offset in TS.MIX.values())
    assert TS.N_LAGS >= 2 and len(TS.due_steps("correlations")) > TS.N_LAGS       # the window wraps: a second origin


def test_the_mix_of_the_record():
    """the figures written down with the mix"""
    assert {k: len(TS.due_steps(k)) for k in TS.MIX} == dict(fields=6, correlations=4, fluxes=5, distributions=3, transits=8, pairs=2)
    assert [s for s in range(1, 25) if len(TS.due_names(s)) >= 3] == [8, 18, 20]
