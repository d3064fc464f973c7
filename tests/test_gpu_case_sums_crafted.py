"""GPU (-m gpu): the sums kernel of a device-RNG step (k_case_sums, csrc/amc_case_sums_dev.h) at its edges, on crafted
records.  A natural state reaches few of them: a tile filled to the record, a thread's second register slot, segment
lengths around the batches of 8 and 16, empty segments and cases, a case of failed solves only, 64 ranks.

One small energised pore (300 particles, so a hits block holds 512 records per case) in one `ShardEnergisedEngine` that owns
every particle; the hits exchange is given a world of its own (3 or 64 blocks).  Per crafted set the ordinary calls of a
sharded device-RNG step run up to `mg_hits_pack`; then the receive buffer is overwritten with the set's blocks
(tests/test_case_sums_host.py: the sets, their layout and the expected rows), `mg_hits_sums` forms row k, and the step is
finished.  One run per engine — per (world, AMC_MG_HITS_TILE) — holds all its sets; its series rows must equal the expected
rows in every bit of the three float64 sums and in the three flags."""
import numpy as np
import pytest
import torch                # (first: the library then shares torch's HIP runtime — the blocks are copied by torch)

from tests.test_case_sums_host import SETS, assert_tells_orders_apart, bits, block_words, expected_row

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def rows(request):
    """name of a crafted set -> the row the device wrote for it"""
    from argon_monte_carlo_amd.engine import ShardEnergisedEngine
    from tests.test_gpu_dist_device_rng import _case
    for cs in SETS:
        if cs["order_sensitive"]:
            assert_tells_orders_apart(cs)           # (on the CPU, before the device is asked)
    p, c, init, cfg = _case(N)
    mp = pytest.MonkeyPatch()
    request.addfinalizer(mp.undo)
    out = {}
    for world, tile in sorted({(cs["world"], cs["tile"]) for cs in SETS}, key=str):
        sets = [cs for cs in SETS if (cs["world"], cs["tile"]) == (world, tile)]
        if tile is None:
            mp.delenv("AMC_MG_HITS_TILE", raising=False)
        else:
            mp.setenv("AMC_MG_HITS_TILE", str(tile))        # (read when the engine creates its hits buffers)
        eng = ShardEnergisedEngine(p, 0, N)
        try:
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            eng.upload(*init)
            _, recv = eng.hits_buffers(world)
            eng.shard_run_begin(len(sets))
            for k, cs in enumerate(sets):
                words = block_words(cs)
                assert recv.numel() == len(words), (recv.numel(), len(words))
                eng.temp_begin(c["dt"])
                eng.temp_cases_device(cfg)
                eng.mg_hits_pack(world)
                recv.copy_(torch.from_numpy(words))
                eng.mg_hits_sums(world, k)
                eng.mg_bounds()
                eng.mg_sweep(1, 0)
                eng.mg_finish(False)
            _, sums, had = eng.shard_run_end(len(sets))
            for k, cs in enumerate(sets):
                out[cs["name"]] = tuple(float(v) for v in sums[k]) + tuple(bool(v) for v in had[k])
        finally:
            eng.close()
    return out


@pytest.mark.parametrize("cs", SETS, ids=lambda cs: cs["name"])
def test_crafted_blocks_give_the_expected_row(rows, cs):
    """The row of the series equals `energised.sum_device_cases` on the set's records merged per case: every bit of the sums,
    and the flags."""
    want, got = expected_row(cs), rows[cs["name"]]
    print(cs["name"], "want", want, "got", got)
    assert bits(got) == bits(want), (cs["name"], got, want)
