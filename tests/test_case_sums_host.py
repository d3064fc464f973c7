"""Host-only: crafted hit records for the sums of a device-RNG step (csrc/amc_case_sums_dev.h), and their expected rows.

A crafted set is what the blocks of `world` ranks hold in one step: per case 3..9 and rank, the records (particle index,
dp_z, dE, ok) in the order they stand in the block.  Particle indices ascend from rank to rank, as shards do, and are
shuffled inside each block.  Magnitudes mix +-1, 1e-17 and 1e+8 (each scaled by a factor in [1, 2)), so that a sum of more
than a few records depends on the order of its additions.  `expected_row` is the order the library defines: per case the
records of all ranks in ascending particle index, failed solves skipped, left to right from 0; the cases folded 3..9
(`energised.sum_device_cases`).  tests/test_gpu_case_sums_crafted.py writes the sets into the receive buffer of the hits
exchange and demands these rows bit for bit; here, without GPU or library, the expectation is checked against a literal
restatement of the fold and against three wrong orders that a crafted set must tell apart."""
import numpy as np
import pytest

from argon_monte_carlo_amd.energised import CASES, COLD_CASES, HOT_CASES, fold_case_parts, sequential_sum, sum_device_cases

HC = 512            # records per case and rank in a hits block of a system below 2,048 particles
HEADER = 8
MAGNITUDES = np.array([1.0, -1.0, 1e-17, -1e-17, 1e8, -1e8])


def craft(name, world, tile, lengths, seed, ok=None, scale=None, order_sensitive=True):
    """lengths[s][r] records of case 3 + s in the block of rank r; ok(s, r, n) -> bool[n] (default: all good);
    scale[s] multiplies the case's values.  `tile`: AMC_MG_HITS_TILE of the engine that sums the set (None: the default)."""
    rng = np.random.default_rng(seed)
    segs = []
    for s in range(7):
        row = []
        for r in range(world):
            n = int(lengths[s][r])
            assert 0 <= n <= HC
            idx = (r * 100_000 + rng.choice(100_000, size=n, replace=False)).astype(np.int64)       # ascending with r, shuffled inside
            val = [rng.choice(MAGNITUDES, size=n) * (1.0 + rng.random(n)) * (1.0 if scale is None else scale[s]) for _ in range(2)]
            good = np.ones(n, dtype=bool) if ok is None else np.asarray(ok(s, r, n), dtype=bool)
            row.append((idx, val[0], val[1], good))
        segs.append(row)
    return dict(name=name, world=world, tile=tile, segs=segs, order_sensitive=order_sensitive)


def spread(total, world, only=None):
    """`total` records over the 7 * world segments (or over those in `only`), unequal and none above HC"""
    free = only or [(s, r) for s in range(7) for r in range(world)]
    lengths = [[0] * world for _ in range(7)]
    left = total
    for k, (s, r) in enumerate(free):
        n = min(HC, left, max(1, (total * (1 + k % 3)) // (2 * len(free)) + 1)) if k + 1 < len(free) else left
        lengths[s][r] = n
        left -= n
    assert left == 0 and sum(map(sum, lengths)) == total and max(map(max, lengths)) <= HC, (total, lengths)
    return lengths


def crafted_sets():
    tails = [[0, 1, 7], [8, 9, 15], [16, 17, 31], [5, 0, 33], [64, 2, 0], [3, 40, 1], [24, 0, 0]]
    empties = [[0, 4, 9], [0, 0, 0], [6, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 11], [12, 3, 0]]      # case 4 wholly empty, cases 6-7 too
    mixed = [[20, 0, 5], [10, 10, 10], [4, 4, 4], [0, 0, 0], [0, 0, 0], [30, 1, 17], [0, 0, 0]]
    wide = [[0] * 64 for _ in range(7)]
    wide[0][0] = wide[6][63] = 1
    few = [(0, 0), (0, 1), (0, 2), (3, 1), (6, 0), (6, 2)]          # (so that a case has enough records for its order to matter)
    sets = [
        craft("tile64_at", 3, 64, spread(64, 3, few), 1),
        craft("tile64_over", 3, 64, spread(65, 3, few), 2),
        craft("tails_global", 3, 64, tails, 3),
        craft("tile6144_at", 3, None, spread(6144, 3), 4),
        craft("tile6144_over", 3, None, spread(6145, 3), 5),
        craft("second_slot", 3, None, spread(1025, 3), 6),
        craft("tails", 3, None, tails, 3),
        craft("empty_segments", 3, None, empties, 7),
        craft("no_records", 3, None, [[0] * 3 for _ in range(7)], 8, order_sensitive=False),
        # case 3 (the only cold case with records): every solve failed; case 4: good and failed records; case 8: good only
        craft("failed_solves", 3, None, mixed, 19, ok=lambda s, r, n: np.zeros(n, bool) if s == 0 else (np.arange(n) % 3 != 1 if s == 1 else np.ones(n, bool))),
        craft("index_order", 3, None, [[37, 41, 29]] * 7, 10),
        craft("case5_sentinel", 3, None, [[3, 2, 4]] * 7, 11, scale=[1, 1, 1e30, 1, 1, 1, 1]),
        craft("wide_world", 64, None, wide, 12, order_sensitive=False),
    ]
    assert len({cs["name"] for cs in sets}) == len(sets)
    return sets


def block_words(cs):
    """int64[world * (8 + 21 HC)]: the receive buffer of the hits exchange holding the set"""
    blk = HEADER + 21 * HC
    out = np.zeros(cs["world"] * blk, dtype=np.int64)
    for r in range(cs["world"]):
        b = out[r * blk:(r + 1) * blk]
        for s in range(7):
            idx, dpz, dE, ok = cs["segs"][s][r]
            n = len(idx)
            b[s] = n
            rec = b[HEADER + 3 * s * HC:HEADER + 3 * (s + 1) * HC]
            rec[:n] = idx | (ok.astype(np.int64) << 32)
            rec[HC:HC + n] = dpz.view(np.int64)
            rec[2 * HC:2 * HC + n] = dE.view(np.int64)
    return out


def _row(cs, order):
    """the row when each case's records are added in `order(segments of the case) -> (dpz, dE, ok)`"""
    results = {}
    for s, case in enumerate(CASES):
        results[case] = order(cs["segs"][s])
    return tuple(float(v) if k < 3 else bool(v) for k, v in enumerate(sum_device_cases(results)))


def _merged(segs, key):
    idx, dpz, dE, ok = (np.concatenate([g[k] for g in segs]) for k in range(4))
    o = key(idx)
    return dpz[o], dE[o], ok[o]


def expected_row(cs):
    return _row(cs, lambda segs: _merged(segs, lambda idx: np.argsort(idx, kind="stable")))


def arrival_row(cs):
    return _row(cs, lambda segs: _merged(segs, lambda idx: np.arange(len(idx))))


def descending_row(cs):
    return _row(cs, lambda segs: _merged(segs, lambda idx: np.argsort(-idx, kind="stable")))


def partial_sums_row(cs):
    """per rank a partial sum in ascending index, the partial sums combined afterwards"""
    part = {}
    for s, case in enumerate(CASES):
        segs = cs["segs"][s]
        if not sum(len(g[0]) for g in segs):
            continue
        m = e = 0
        for idx, dpz, dE, ok in segs:
            o = np.argsort(idx, kind="stable")
            m = m + sequential_sum(dpz[o][ok[o]])
            e = e + sequential_sum(dE[o][ok[o]])
        part[case] = (m, e, any(g[3].any() for g in segs))
    return tuple(float(v) if k < 3 else bool(v) for k, v in enumerate(fold_case_parts(part)))


def bits(row):
    return tuple(np.float64(v).view(np.uint64) if isinstance(v, float) else v for v in row)


def assert_tells_orders_apart(cs):
    want = bits(expected_row(cs))
    for other in (arrival_row, descending_row, partial_sums_row):
        assert bits(other(cs)) != want, (cs["name"], other.__name__)


SETS = crafted_sets()


@pytest.mark.parametrize("cs", SETS, ids=lambda cs: cs["name"])
def test_expected_row_is_the_literal_fold(cs):
    """The fold written out — momentum from every case with records, energies from the cold {3, 7, 9} and hot {4, 6, 8}
    cases, in the order 3..9, a flag only from a good record — on per-case sums formed here equals `fold_case_parts` and
    the expected row."""
    part, mom, cold, hot, had = {}, 0.0, 0.0, 0.0, [False, False, False]
    for s, case in enumerate((3, 4, 5, 6, 7, 8, 9)):
        dpz, dE, ok = _merged(cs["segs"][s], lambda idx: np.argsort(idx, kind="stable"))
        if not len(ok):
            continue
        m = e = 0.0
        for k in range(len(ok)):
            if ok[k]:
                m, e = m + float(dpz[k]), e + float(dE[k])
        part[case] = (m, e, bool(ok.any()))
        mom, had[0] = mom + m, had[0] or bool(ok.any())
        if case in (3, 7, 9):
            cold, had[1] = cold + e, had[1] or bool(ok.any())
        if case in (4, 6, 8):
            hot, had[2] = hot + e, had[2] or bool(ok.any())
    literal = (mom, cold, hot) + tuple(had)
    assert (COLD_CASES, HOT_CASES) == ((3, 7, 9), (4, 6, 8))
    assert bits(tuple(float(v) if k < 3 else bool(v) for k, v in enumerate(fold_case_parts(part)))) == bits(literal)
    assert bits(expected_row(cs)) == bits(literal)


@pytest.mark.parametrize("cs", [cs for cs in SETS if cs["order_sensitive"]], ids=lambda cs: cs["name"])
def test_wrong_orders_give_other_bits(cs):
    """Block-arrival order, descending index and per-rank partial sums each give a row with other bits."""
    assert_tells_orders_apart(cs)


def test_sets_reach_what_they_are_named_for():
    by = {cs["name"]: cs for cs in SETS}
    total = lambda cs: sum(len(g[0]) for row in cs["segs"] for g in row)
    assert [total(by[k]) for k in ("tile64_at", "tile64_over", "tile6144_at", "tile6144_over", "second_slot")] == [64, 65, 6144, 6145, 1025]
    assert total(by["tails_global"]) > 64 and total(by["tails"]) <= 6144
    assert {len(g[0]) for row in by["tails"]["segs"] for g in row} >= {0, 1, 7, 8, 9, 15, 16, 17, 31}
    assert total(by["no_records"]) == 0 and expected_row(by["no_records"]) == (0.0, 0.0, 0.0, False, False, False)
    e = by["empty_segments"]["segs"]
    assert len(e[0][0][0]) == 0 and len(e[6][2][0]) == 0 and all(len(g[0]) == 0 for s in (1, 3, 4) for g in e[s])
    f = expected_row(by["failed_solves"])
    assert f[3:] == (True, False, True) and f[1] == 0.0 and f[2] != 0.0
    ok4 = np.concatenate([g[3] for g in by["failed_solves"]["segs"][1]])
    assert ok4.any() and not ok4.all()
    s5 = expected_row(by["case5_sentinel"])
    assert abs(s5[0]) > 1e29 and abs(s5[1]) < 1e10 and abs(s5[2]) < 1e10
    w = by["wide_world"]
    assert w["world"] == 64 and total(w) == 2 and len(w["segs"][0][0][0]) == 1 and len(w["segs"][6][63][0]) == 1
    for cs in SETS:         # indices ascend from rank to rank and are not ascending inside a block of several records
        for row in cs["segs"]:
            tops = [(g[0].min(), g[0].max()) for g in row if len(g[0])]
            assert all(a[1] < b[0] for a, b in zip(tops, tops[1:])), cs["name"]
    assert any(len(g[0]) > 1 and (np.diff(g[0]) < 0).any() for row in by["index_order"]["segs"] for g in row)
