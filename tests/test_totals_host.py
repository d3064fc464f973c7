"""totals.sum_over_ranks — the one collective behind ShardedSimulation.fields(), .correlations() and
ShardedTemperatureSimulation.surface() — driven with a fake communicator: the 128-bit sums across every limb boundary against
Python ints, the status every rank reads out of the same all-reduce, and the shortcut of a single rank.  CPU only."""
import numpy as np
import pytest

from argon_monte_carlo_amd import _lib
from argon_monte_carlo_amd import totals as TT
from argon_monte_carlo_amd._abi import AMC_ERR_CAPACITY

# pairs whose sum crosses a limb boundary: bit 32, bit 64 (the word boundary), zero from below, and the two ends of the range
PAIRS = [(2 ** 32 - 1, 1), (2 ** 64 - 1, 1), (-1, 1), (-(2 ** 127), 2 ** 127 - 1)]


class FakeComm:
    """One rank's view of an all-reduce over ``world`` ranks: the sum of what this rank sends and what ``others`` (the other
    ranks' vectors, or a function of this rank's vector that returns them) send."""

    def __init__(self, others=(), shortcut=True):
        self.others, self.shortcut, self.calls = others, shortcut, 0

    def allreduce_sum_ints(self, values):
        self.calls += 1
        values = [int(v) for v in values]
        others = self.others(values) if callable(self.others) else self.others
        assert all(len(o) == len(values) for o in others)
        return [sum(col) for col in zip(values, *others)]


def _never(r, s):
    raise AssertionError(f"describe({r}, {s}) without a failing rank")


def _describe(r, s):
    if s > 0:
        return _lib.ArgonMCError(AMC_ERR_CAPACITY, f"particle {s - 1} (rank {r}) is out of range")
    return _lib.ArgonMCError(s, f"the read failed on rank {r}")


def _flat(world, rank, status, arrays, counters):
    """what a rank sends: every rank's status first, then the limbs, then the counters"""
    st = [0] * world
    st[rank] = status
    return st + [int(v) for a in arrays for v in TT.words_to_limbs(a).ravel()] + list(counters)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sums_cross_every_limb_boundary_exactly(world):
    """Each pair is split over the first two ranks (a third one adds a value of its own); one rank holds the whole pair's sum
    only when it is alone, where the all-reduce is skipped."""
    ints = np.zeros((world, len(PAIRS), 2), dtype=object)
    ints[...] = 0
    for k, (u, v) in enumerate(PAIRS):
        if world == 1:
            ints[0, k, 0], ints[0, k, 1] = u + v, v + u
        else:
            ints[0, k, 0], ints[1, k, 0] = u, v
            ints[0, k, 1], ints[1, k, 1] = v, u
            if world == 3:
                ints[2, k, 0], ints[2, k, 1] = -(2 ** 31), 2 ** 33 + 5
    second = np.array([[3, -7], [2 ** 64 - 2, 2], [-(2 ** 64), 2 ** 64 - 1]][:world], dtype=object)      # a second array, another shape
    counters = [[5, 2 ** 40], [7, 2 ** 40], [11, 1]][:world]
    words = [[TT.ints_to_words(ints[r]), TT.ints_to_words(second[r])] for r in range(world)]
    for rank in range(world):
        others = [_flat(world, r, 0, words[r], counters[r]) for r in range(world) if r != rank]
        comm = FakeComm(others)
        (a, b), c = TT.sum_over_ranks(comm, world, rank, None, words[rank], counters[rank], _never)
        assert comm.calls == (0 if world == 1 else 1)
        assert a.dtype == np.int64 and a.shape == (len(PAIRS), 2, 2) and b.shape == (2, 2)
        assert TT.words_to_ints(a).tolist() == ints.sum(axis=0).tolist()
        assert TT.words_to_ints(b).tolist() == second.sum(axis=0).tolist()
        assert c == [sum(col) for col in zip(*counters)]
    if world == 2:
        assert TT.words_to_ints(a)[:, 0].tolist() == [2 ** 32, 2 ** 64, 0, -1]


@pytest.mark.parametrize("world,bad_rank", [(2, 1), (3, 1), (3, 2)])
def test_a_particle_out_of_range_on_one_rank_raises_on_every_rank(world, bad_rank):
    p = 4098
    words, zeros = TT.ints_to_words(np.array([[1, 2]], dtype=object)), np.zeros((1, 2, 2), dtype=np.int64)
    own = _lib.ArgonMCError(AMC_ERR_CAPACITY, f"amc_fields: particle {p} has a velocity component outside the range")
    messages = []
    for rank in range(world):
        err = own if rank == bad_rank else None
        others = [_flat(world, r, p + 1 if r == bad_rank else 0, [zeros if r == bad_rank else words], [0]) for r in range(world) if r != rank]
        comm = FakeComm(others)
        with pytest.raises(_lib.ArgonMCError) as ei:
            TT.sum_over_ranks(comm, world, rank, err, [zeros if err else words], [0], _describe)
        assert comm.calls == 1 and ei.value.code == AMC_ERR_CAPACITY
        assert ei.value is not own and (ei.value.__cause__ is own) == (rank == bad_rank)
        messages.append(str(ei.value))
    assert len(set(messages)) == 1 and f"particle {p} " in messages[0] and f"rank {bad_rank}" in messages[0]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("own", [False, True])
def test_a_negative_code_on_one_rank_raises_that_code_on_every_rank(world, own):
    zeros = np.zeros((2, 2), dtype=np.int64)
    own = _lib.ArgonMCError(-6, "the read failed here")
    for rank in range(world):
        err = own if rank == 1 else None
        others = [_flat(world, r, -6 if r == 1 else 0, [zeros], [0, 0]) for r in range(world) if r != rank]
        with pytest.raises(_lib.ArgonMCError) as ei:
            TT.sum_over_ranks(FakeComm(others), world, rank, err, [zeros], [0, 0], _describe, own_if_all_failed=own)
        assert ei.value.code == -6 and "rank 1" in str(ei.value) and ei.value is not own


def test_a_capacity_error_of_one_rank_reaches_a_sampler_that_names_no_particle_with_its_code():
    """the surfaces' capacity message names a particle too; their ``describe`` turns the positive status back into the code"""
    zeros = np.zeros((2, 2), dtype=np.int64)
    own = _lib.ArgonMCError(AMC_ERR_CAPACITY, "amc_surface: the hit of particle 17 is outside the range")
    seen = []

    def describe(r, s):
        seen.append((r, s))
        return _lib.ArgonMCError(AMC_ERR_CAPACITY if s > 0 else s, f"surface_read failed on rank {r}")
    comm = FakeComm(lambda v: [[0, 0] + [0] * (len(v) - 2)])
    with pytest.raises(_lib.ArgonMCError) as ei:
        TT.sum_over_ranks(comm, 2, 0, own, [zeros], [0], describe, own_if_all_failed=True)
    assert seen == [(0, 18)] and ei.value.code == AMC_ERR_CAPACITY and "surface_read failed on rank 0" in str(ei.value)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_the_surfaces_ranks_that_all_failed_raise_their_own_error(world):
    zeros = np.zeros((1, 2), dtype=np.int64)
    for rank in range(world):
        own = _lib.ArgonMCError(-3, f"amc_surface_read: hits are missing (rank {rank}'s own text)")
        others = [_flat(world, r, -3, [zeros], [0]) for r in range(world) if r != rank]
        with pytest.raises(_lib.ArgonMCError) as ei:
            TT.sum_over_ranks(FakeComm(others), world, rank, own, [zeros], [0], _describe, own_if_all_failed=True)
        assert ei.value is own


def test_by_default_ranks_that_all_failed_name_the_first_of_them_but_a_single_rank_raises_its_own():
    zeros = np.zeros((1, 2), dtype=np.int64)
    own = _lib.ArgonMCError(AMC_ERR_CAPACITY, "amc_corr: particle 9 is outside the quantisers' range")
    with pytest.raises(_lib.ArgonMCError) as ei:
        TT.sum_over_ranks(FakeComm([_flat(2, 0, 4, [zeros], [0])]), 2, 1, own, [zeros], [0], _describe)
    assert ei.value is not own and "particle 3 (rank 0)" in str(ei.value)
    for shortcut in (True, False):
        with pytest.raises(_lib.ArgonMCError) as ei:
            TT.sum_over_ranks(FakeComm(shortcut=shortcut), 1, 0, own, [zeros], [0], _describe)
        assert ei.value is own


@pytest.mark.parametrize("shortcut,calls", [(True, 0), (False, 1)])
def test_a_single_rank_skips_the_all_reduce_only_with_the_shortcut(shortcut, calls):
    ints = np.array([[2 ** 64 - 1, -1], [-(2 ** 127), 2 ** 127 - 1]], dtype=object)
    comm = FakeComm(shortcut=shortcut)
    (a,), c = TT.sum_over_ranks(comm, 1, 0, None, [TT.ints_to_words(ints)], [3, 4], _never)
    assert comm.calls == calls
    assert TT.words_to_ints(a).tolist() == ints.tolist() and c == [3, 4]
