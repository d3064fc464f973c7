"""CPU: the crafted states of tests/allpairs_states.py through the oracle — every state hits the edges it is built for (each
tile pair, each in-tile offset class, the diagonal classes, margin < band at the far corner) with fillers silent — and the
mirrored constants equal the kernels' own, read from the text of amc_grid.hip."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import allpairs_states as A

SRC = Path(__file__).resolve().parents[1] / "argon_monte_carlo_amd" / "csrc" / "amc_grid.hip"
SF = ("x", "y", "z", "vx", "vy", "vz", "d", "dx", "dy", "dz")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_the_mirrored_constants_are_the_kernels():
    text = SRC.read_text()
    d = dict(re.findall(r"^#define[ \t]+(AP2?_\w+)[ \t]+(.+?)[ \t]*(?://.*)?$", text, flags=re.M))
    assert set(d) == {"AP_T", "AP2_T", "AP2_R", "AP2_THREADS", "AP2_CHUNK"}
    assert int(d["AP_T"]) == A.AP_T and int(d["AP2_T"]) == A.AP2_T and int(d["AP2_R"]) == A.AP2_R
    assert d["AP2_THREADS"] == "(AP2_T / AP2_R)" and A.AP2_THREADS == A.AP2_T // A.AP2_R == 256
    assert int(d["AP2_CHUNK"]) == A.AP2_CHUNK
    m = re.search(r"if \(n >= (\d+) \* AP2_T && c->G\.ncells > 0\)", text)
    assert m and int(m.group(1)) * A.AP2_T == A.SWITCH_N == 16384
    assert A.tile_of(A.SWITCH_N - 1) == A.AP_T and A.tile_of(A.SWITCH_N) == A.AP2_T
    # the thresholds: cr^2 inflated by 1e-9 for both kernels, raised by 64 u R^2 for the tiled one
    m = re.search(r"^#define AMC_CR2_INFLATE \((\S+) \+ (\S+)\)$", text, flags=re.M)
    assert m and float(m.group(1)) + float(m.group(2)) == A.CR2_INFLATE
    assert "thr = cr2i + 64.0 * 1.1102230246251565e-16 * (ex * ex + ey * ey + ez * ez)" in text
    assert 1.1102230246251565e-16 == 2.0 ** -53
    # the register rows and the diagonal rule the offsets are aimed at
    assert "ii[r] = bi * AP2_T + r * AP2_THREADS + (int)threadIdx.x" in text and "(diag ? j < ii[r] : true)" in text


def _through_the_oracle(O, s, steps, sweep_only=False):
    """the checks every state must pass on the CPU; returns the records of the first sweep"""
    orc = O.Oracle(s.p, mode="mul")
    a = s.arrays()
    orc.upload(*a[:10], flag=a[10])
    npp, first, recs = 0, None, []
    for q in range(steps):
        if sweep_only:
            rc, n1, _ = orc.sweep()
        else:
            rc, so = orc.timestep(s.dt)
            n1 = so["n_pp"]
        assert rc == 0
        st = orc.state()
        for k in SF:
            assert np.isfinite(st[k]).all(), (q, k)
        recs.append(orc.drain_paths())
        npp += n1
        if q == 0:
            first, npp0 = recs[0], n1
    assert npp0 > 0
    rec = np.concatenate(recs)
    for k in ("total", "px", "py", "pz"):
        assert np.isfinite(rec[k]).all(), k
    _, seen = A.pair_hits(rec, s.extra["pairs"])
    assert not s.extra["filler"][sorted(seen)].any()            # no filler in any completed-path record, wall or pair
    assert s.extra["filler"].sum() == s.n - len(np.unique(s.extra["pairs"]))
    hits, _ = A.pair_hits(first, s.extra["pairs"])
    return hits


@pytest.mark.parametrize("kind,T,ntiles,last", A.MATRIX)
def test_tile_matrix_hits_every_tile_pair_and_offset(O, kind, T, ntiles, last):
    s = A.tile_matrix(kind, T, ntiles, last)
    n = (ntiles - 1) * T + last
    assert s.n == n <= 17_000 and s.extra["T"] == T == A.tile_of(n)
    col, P, off, tiles = s.extra["collide"], s.extra["pairs"], s.extra["offsets"], s.extra["tiles"]
    hits = _through_the_oracle(O, s, 4)
    assert np.array_equal(hits > 0, col), np.flatnonzero((hits > 0) != col)[:8]
    want = {(bi, bj) for bi in range(ntiles) for bj in range(bi + 1)}
    assert A.tile_pairs_covered(s) == want and len(want) == {17: 153, 7: 28}[ntiles]
    assert (P[:, 0] > P[:, 1]).all() and (tiles[:, 0] >= tiles[:, 1]).all()
    # a pair that must not collide on one tile pair in four or more, all three kinds of it
    assert 4 * (~col).sum() >= len(want)
    assert {nm for nm, c in zip(s.extra["names"], col) if not c} == set(A.OUT)
    assert {nm for nm, c in zip(s.extra["names"], col) if c} == set(A.IN)
    # every boundary offset of a full tile and of the partial one carries a colliding pair; n - 1 does
    seen_full = {int(o) for t, o in zip(tiles[col].ravel(), off[col].ravel()) if t < ntiles - 1}
    seen_last = {int(o) for t, o in zip(tiles[col].ravel(), off[col].ravel()) if t == ntiles - 1}
    assert set(A.boundary_offsets(T, T)) <= seen_full, sorted(set(A.boundary_offsets(T, T)) - seen_full)
    assert set(A.boundary_offsets(T, last)) <= seen_last, sorted(set(A.boundary_offsets(T, last)) - seen_last)
    assert n - 1 in P[col]
    # in the role the boundary belongs to, OFF the diagonal: register rows for i, chunks for j
    offd = col & (tiles[:, 0] != tiles[:, 1])
    rows = {r * A.AP2_THREADS - e for r in range(1, A.AP2_R) for e in (0, 1)} if T == A.AP2_T else set()
    assert rows | {0, T - 1} <= {int(o) for o in off[offd, 0]}
    assert {0, A.AP2_CHUNK - 1, A.AP2_CHUNK, T - 1} <= {int(o) for o in off[offd, 1]}
    # the diagonal classes, each checked against what it claims
    cls = s.extra["diag"]
    for k, c in enumerate(cls):
        i, j = int(off[k, 0]), int(off[k, 1])
        if not c:
            continue
        assert tiles[k, 0] == tiles[k, 1] and col[k]
        if c == "adjacent":
            assert i == j + 1 and i % A.AP2_CHUNK == 0
        elif c == "same_thread":
            assert (i - j) % A.AP2_THREADS == 0 and i != j and i % A.AP2_THREADS == j % A.AP2_THREADS
        else:
            size = T if tiles[k, 0] < ntiles - 1 else last
            assert c == "ends" and j == 0 and i == size - 1
    assert set(cls) - {""} == ({"adjacent", "same_thread", "ends"} if T == A.AP2_T else {"adjacent", "ends"})
    if T == A.AP2_T:                    # register rows 0 and k of one thread, for every k
        assert {(int(off[k, 0]) - int(off[k, 1])) // A.AP2_THREADS for k, c in enumerate(cls) if c == "same_thread"} == {1, 2, 3}
    for t in range(ntiles):             # every diagonal tile has them, where its size allows
        mine = {c for k, c in enumerate(cls) if c and tiles[k, 0] == t}
        size = T if t < ntiles - 1 else last
        assert ("adjacent" in mine) == (size >= 2 * A.AP2_CHUNK + 2) and ("ends" in mine) == (t % 2 == 0)
        assert ("same_thread" in mine) == (T == A.AP2_T and size > 100 + t + A.AP2_THREADS)


def test_switch_sizes_stand_on_either_side_of_the_switch(O):
    states = A.switch_sizes()
    assert [s.n for s in states] == [A.SWITCH_N - 1, A.SWITCH_N, A.SWITCH_N + 1]
    assert [s.extra["T"] for s in states] == [A.AP_T, A.AP2_T, A.AP2_T]
    for s in states:
        n, T = s.n, s.extra["T"]
        col, P = s.extra["collide"], s.extra["pairs"]
        hits = _through_the_oracle(O, s, 3)
        assert np.array_equal(hits > 0, col)
        assert len(P) >= 12 and col.sum() == 16 and (~col).sum() == 4
        have = {(int(i), int(j)) for (i, j), c in zip(P, col) if c}
        assert {(n - 1, 0), (n - 1, n - 2)} <= have
        F = s.extra["last_full_tile"]
        assert (F + 1) * T <= n < (F + 2) * T + (T if n % T == 0 else 0)
        assert any(i // T == j // T == F for i, j in have)
        # the chunk re-walk: three partners j of one i in one chunk; the three upper register rows of one thread on one j
        i, js = s.extra["rewalk"]["same_chunk"]
        assert {(i, j) for j in js} <= have and len({j // A.AP2_CHUNK for j in js}) == 1 and len(js) == 3
        j, rows = s.extra["rewalk"]["same_thread"]
        assert {(i, j) for i in rows} <= have and len({i // A.AP2_T for i in rows}) == 1
        assert len({i % A.AP2_THREADS for i in rows}) == 1 and sorted(i % A.AP2_T // A.AP2_THREADS for i in rows) == [1, 2, 3]
    # 64 tiles, the last with 255 particles | sixteen full tiles | a 17th tile of one particle
    assert (states[0].n + A.AP_T - 1) // A.AP_T == 64 and states[0].n % A.AP_T == 255
    assert states[1].n == 16 * A.AP2_T and states[2].n == 16 * A.AP2_T + 1


def _at_the_sweep(s):
    return np.stack([s.x + s.dt * s.vx, s.y + s.dt * s.vy, s.z + s.dt * s.vz], axis=1)


@pytest.mark.parametrize("kind", ["cube", "pore"])
def test_far_corner_pairs_lie_where_the_raised_threshold_decides(O, kind):
    s = A.far_corner(kind)
    assert A.SWITCH_N <= s.n <= 17_000 and s.extra["T"] == A.AP2_T
    col, P, names = s.extra["collide"], s.extra["pairs"], s.extra["names"]
    anchor, margin, band = np.array(s.extra["anchor"]), s.extra["margin"], s.extra["band"]
    hits = _through_the_oracle(O, s, 4)
    assert np.array_equal(hits > 0, col)
    for a in ("far", "origin"):
        assert col[anchor == a].any() and (~col[anchor == a]).any()
    inm = np.array([nm in A.IN for nm in names])
    assert (inm & (anchor == "far")).sum() == 12 and col[inm].all()
    # the cancellation scale of the expanded form exceeds the pair's margin: the threshold's raise decides these pairs
    assert (margin[inm] > 0).all() and (margin[inm] < band).all(), (margin[inm].max(), band)
    assert len({int(t) for t in s.extra["tiles"].ravel()}) >= 12             # indices spread over the tiles
    # the kernel's own arithmetic, operation by operation: with the raised threshold no colliding pair is missed ...
    X, cr = _at_the_sweep(s), s.p.collision_range
    cr2i = cr * cr * A.CR2_INFLATE
    assert s.extra["thr"] == cr2i + 64.0 * band
    raised = np.array([A.tiled_test(X[i], X[j], s.extra["origin"], s.extra["thr"])[0] for i, j in P])
    assert raised[col].all()
    # ... and with thr = cr2i, the unraised one: in the pore half of the far corner's in_m pairs fall outside (the rounding
    # of |r|^2 ~ 1e-11 m^2 is 1.6e-27, the 1e-9 inflation of cr^2 1.1e-28); the cube's extent is too small to tell
    unraised = np.array([A.tiled_test(X[i], X[j], s.extra["origin"], cr2i)[0] for i, j in P])
    missed = int((col & ~unraised & (anchor == "far")).sum())
    print(f"far_corner {kind}: band {band:.3e}, inflation {cr2i - cr * cr:.3e}, largest in_m margin {margin[inm].max():.3e}, "
          f"colliding far pairs an unraised threshold misses: {missed} of {int((col & (anchor == 'far')).sum())}")
    if kind == "pore":
        assert cr2i - cr * cr < band and missed >= 1
    else:
        assert cr2i - cr * cr > band and missed == 0


@pytest.mark.parametrize("kind", ["cube", "pore"])
def test_the_raised_threshold_covers_every_colliding_pair_of_the_matrix(kind):
    """the tile matrix through the tiled kernel's arithmetic on the CPU: the detector is a superset on every tile pair"""
    s = A.tile_matrix(kind, A.AP2_T, 17, 544)
    G = A.grid_of(s.p, s.p.fine_cell)
    cr, X = s.p.collision_range, _at_the_sweep(s)
    R2 = (G.gx * G.h) ** 2 + (G.gy * G.h) ** 2 + (G.gz * G.h) ** 2
    thr = cr * cr * A.CR2_INFLATE + 64.0 * 2.0 ** -53 * R2
    ok = np.array([A.tiled_test(X[i], X[j], (G.x0, G.y0, G.z0), thr)[0] for i, j in s.extra["pairs"]])
    assert ok[s.extra["collide"]].all()


def test_outside_pairs_stand_outside_the_grid_extent(O):
    s = A.outside()
    assert A.SWITCH_N <= s.n <= 17_000
    P, col = s.extra["pairs"], s.extra["collide"]
    hits = _through_the_oracle(O, s, 1, sweep_only=True)
    assert (hits > 0).any() and (hits == 0).any()
    assert col[hits > 0].all()                                   # (the overlap is necessary; the reference cell decides)
    G = A.grid_of(s.p, s.p.fine_cell)
    lo = np.array([G.x0, G.y0, G.z0])
    hi = lo + np.array([G.gx, G.gy, G.gz]) * G.h
    pos = np.stack([s.x, s.y, s.z], axis=1)[P.ravel()]
    assert (pos < lo + G.h).any() and (pos > hi).any()           # in the guard cells below, beyond them above: past the extent the bound is computed from
    assert (pos[:, 2] < 0).any() and (pos[:, 2] > s.p.H).any() and (np.hypot(pos[:, 0], pos[:, 1]) > s.p.R_oa).any()
