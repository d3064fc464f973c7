"""GPU (-m gpu): the sampled free paths' entry points behind every state a step can leave pending — the rows of
tests/test_gpu_pending.py that test_gpu_mfp.py's own cells (amc_timestep, a plain amc_run, one rank that owns everything) do
not drive: the stage calls, two ranks in one process with the sweep replicated and with detection sharded by index
(amc_mg_detect / amc_mg_resolve), on the cube and the pore, the energised pore's host-handshake step and amc_temp_run_device
with a device seed.  The on-demand and overlapped rows of that matrix do not exist here: with a grid configured amc_run takes
its plain loop.

The rig, its systems and its oracle trajectories are that module's (``Rig``: mid-flight states with a raised cross-section,
every collision of every sweep completes two paths).  A cell: the producer's three steps with the sampler on (keep_records,
every rank its own context), one of the six entry points on every rank, one more step.  The totals summed over the ranks must
equal tests/mfp_ref.py fed the ORACLE's records and states — what the undisturbed run bins — over the steps the entry point
leaves standing, and the state must be the oracle's: bit for bit.

The stage calls are no steps: they complete paths but run no hook, so their records wait behind the cursor and the next real
step (here: amc_timestep) bins them all, at that step's positions — unless a drain, amc_reset_outputs or a new grid has
dropped them."""
import numpy as np
import pytest
import torch                # noqa: F401  (first: the library then shares torch's HIP runtime — the two-rank rows exchange through torch)

from argon_monte_carlo_amd import free_paths as FP
from tests import mfp_ref as REF
from tests import test_gpu_pending as PD

pytestmark = pytest.mark.gpu

ROWS = [c for c in PD.CASES if c[0] in ("stages", "shard2_rep", "shard2_idx", "temp_host", "temp_run")]
CONSUMERS = ["config", "read", "load", "reset", "drain", "reset_outputs"]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def check_sum(rig, ref):
    """the ranks' totals, histograms and record counters summed equal the reference's; every rank has counted its steps"""
    reads = [e.mfp_read() for e in rig.engs]
    tot = sum(FP.words_to_ints(r[0]) for r in reads)
    assert (tot == ref.tot).all()
    assert np.array_equal(sum(r[1] for r in reads), ref.hist)
    assert (sum(r[2][0] for r in reads), sum(r[2][1] for r in reads)) == (ref.n_records, ref.n_outside)
    assert all(r[2][2] == ref.n_steps for r in reads)


@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("case", ROWS, ids=PD.case_id)
def test_entry_point_behind_a_pending_step(case, consumer, O, monkeypatch):
    rig = PD.Rig(O, case, monkeypatch)
    T = rig.T
    g = FP.default_grid(rig.p, keep_records=True)
    for e in rig.engs:
        e.mfp_config(g)
    hooked = rig.prod != "stages"
    ref, unseen = REF.Totals(g), []         # unseen: records behind the cursor that no hook has binned yet
    rig.produce()                           # (asserts that the oracle's last sweep has collisions and paths, on every rank)
    k = rig.k
    for s in range(k):
        rec = T.paths(s + 1, since=s)
        if hooked:
            ref.add_step(rec, T.state(s + 1))
        else:
            unseen.append(rec)
    if consumer == "config":
        for e in rig.engs:
            e.mfp_config(g)
        ref, unseen = REF.Totals(g), []
    elif consumer == "read":
        check_sum(rig, ref)
    elif consumer == "load":
        for e in rig.engs:
            tot, hist, counters = e.mfp_read()
            e.mfp_reset()
            e.mfp_load(tot, hist, counters)
    elif consumer == "reset":
        for e in rig.engs:
            e.mfp_reset()
        ref.reset()
    elif consumer == "drain":
        assert len(rig.drain()) == len(T.paths(k))
        unseen = []
    else:
        for e in rig.engs:
            e.reset_outputs()
        unseen = []
    # one more step, and the oracle from the state after k steps beside it (amc_reset_outputs restarts the step index the device
    # draws are keyed by)
    fork = T.fork(k, step=0 if consumer == "reset_outputs" else None)
    if hooked:
        rig.one_more()
    else:
        rig.engs[0].timestep(rig.dt)
    rc, _ = fork.timestep(rig.dt)
    assert rc == 0
    last = fork.paths()
    assert len(last) > 0
    ref.add_step(np.concatenate(unseen + [last]), fork.state())
    ref.check()
    check_sum(rig, ref)
    assert ref.n_records > 0 and ref.n_steps == (1 if consumer in ("config", "reset") or not hooked else k + 1)
    rig.assert_state(fork.state(), (case, consumer))
    kept = k + 1 if consumer in ("config", "read", "load", "reset") else 1      # steps whose records are still in the buffers
    assert rig.paths_pending() == len(last) + (len(T.paths(k)) if kept > 1 else 0)
    rig.close()
