"""CPU: the catalogue of tests/list_states.py through the oracle — every proof of every case, for both geometries, cell sizes,
index permutations and cycle lengths — and the host mirror of the kept lists' cell arithmetic on hand-computed cells."""
import struct

import numpy as np
import pytest

from tests import list_states as LS


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("K", LS.KS)
@pytest.mark.parametrize("cell", LS.CELLS)
@pytest.mark.parametrize("perm", LS.PERMS)
@pytest.mark.parametrize("kind", LS.KINDS + ("temp",))
def test_every_catalogue_proof_holds(O, kind, perm, cell, K):
    s = LS.catalogue(kind, perm, cell, K)
    assert s.n == LS.N_MAIN + LS.TAIL and s.n % 64 and s.n % 256 and s.n <= 1000
    run = LS.oracle_run(O, s, LS.steps(K))
    counts, ncand = LS.catalogue_proofs(s, run)
    wave_cap = 64 * (K - 1)
    # the fence: on the last step in between the three marching waves stand at wave_cap exactly, nobody beyond it
    for w in range(LS.FULL_WAVES):
        fw = s.extra["waves"][("march_full", w)][0]
        assert counts[K - 1, fw] == counts[2 * K - 1, fw] == wave_cap
    assert counts.max() == wave_cap
    # single lanes and the partial wave
    assert counts[1, s.extra["waves"][("march_lanes", (0,))][0]] == 1
    assert counts[1, s.extra["waves"][("march_lanes", (63,))][0]] == 1
    assert counts[1, s.extra["waves"][("march_lanes", (62, 63))][0]] == 2
    assert counts[1, LS.WAVES] == LS.TAIL_MARCHERS and counts.shape[1] == LS.WAVES + 1
    # lanes are where they are meant to be after the permutation
    lanes = sorted(i % 64 for i in s.cases["march_lanes"])
    assert lanes == [0, 62, 63, 63]
    assert sorted(s.cases["march_tail"]) == list(range(s.n - LS.TAIL_MARCHERS, s.n))
    # pool-pool pairs come from two waves; the pool-rest pairs have the marcher on either side of the rester
    for case, i, j, t in s.extra["meet"]:
        if case.startswith("pair_pool_pool"):
            assert i // 64 != j // 64 and t == K - 1
        if case.startswith("pair_pool_rest"):
            assert (i < j) == case.endswith("below")
    assert sum(ncand) >= len(s.extra["meet"]) - 1
    want = {"march_full", "march_lanes", "march_tail", "pair_pool_pool"}
    if kind != "temp":                  # (the energised pore: the groups that stay clear of every energised surface)
        want |= {"pair_pool_rest", "there_and_back", "rebound_mover"}
    if kind != "cube":
        want |= {"layer_window", "layer_window_back"}
    if kind == "pore":
        want |= {"bounds_jump"}
    assert want <= set(s.cases)


def test_both_index_orders_of_the_pool_pool_pairs_occur(O):
    order = set()
    for perm in LS.PERMS:
        s = LS.catalogue("cube", perm, "min", 4)
        order |= {(case, i < j) for case, i, j, t in s.extra["meet"] if case.startswith("pair_pool_pool")}
    assert len(order) == 6


@pytest.mark.parametrize("cell", LS.CELLS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_face_rounding_lands_on_the_rounded_face(O, kind, cell):
    s = LS.face_rounding(kind, cell)
    run = LS.oracle_run(O, s, LS.steps(4))
    LS.catalogue_proofs(s, run)
    i, below, k = s.extra["on_face"]
    G = LS.grid_of(s.p, s.extra["h_asked"])
    for t, want_double, want_filed in ((0, k - 1, k - 1), (1, k - 1, k)):      # (in step 1 it meets its partner)
        x = run[t]["pre"][0][i]
        assert np.floor((x - G.x0) * G.inv_h) == want_double, t
        assert LS.grid_coords(G, *[v[i:i + 1] for v in run[t]["pre"]])[0][0] == want_filed, t
    assert run[1]["pre"][0][i] == below


# ---------------------------------------------------------------------------------------------------------------- the mirror
def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_mirror_cells_of_the_cube_by_hand():
    s = LS.catalogue("cube", "identity", "wide", 2)
    p, h = s.p, s.extra["h_asked"]
    G = LS.grid_of(p, h)
    assert G.h == h and G.x0 == -h and G.z0 == -h           # no enlargement: 92^3 cells
    assert G.gx == G.gy == G.gz == int(np.ceil(p.cube_x / h)) + 2 == 92
    mid = lambda k: -h + (k + 0.5) * h
    # mid-cell, in the guard cells, clamped below and above
    xs = np.array([mid(1), mid(0), -7.0 * h, mid(91), p.cube_x + 9.0 * h, mid(40)])
    ys = np.array([mid(1), mid(5), mid(5), mid(91), mid(0), -3.0 * h])
    zs = np.array([mid(1), mid(9), mid(9), mid(91), p.cube_z + 2.0 * h, mid(17)])
    c, outside = LS.filed_cell(p, h, xs, ys, zs)
    want = [(1, 1, 1), (0, 5, 9), (0, 5, 9), (91, 91, 91), (91, 0, 91), (40, 0, 17)]
    assert c.tolist() == [(cz * 92 + cy) * 92 + cx for cx, cy, cz in want]
    assert not outside.any()                                 # (the cube's coordinates are clamped into the one window)
    # on a face and an ulp below: what decides is the single-precision record, read back as amc_rec_pos does
    for k in (2, 37, 90):
        for x in (-h + k * h, float(np.nextafter(-h + k * h, -np.inf))):
            rel = _f32(x - G.x0)
            cx = int(np.floor(((G.x0 + rel) - G.x0) * (1.0 / h)))
            got, _ = LS.filed_cell(p, h, np.array([x]), np.array([mid(3)]), np.array([mid(4)]))
            assert got[0] == (4 * 92 + 3) * 92 + cx and cx in (k - 1, k)


def test_mirror_cells_of_the_pore_by_hand():
    s = LS.catalogue("pore", "identity", "min", 2)
    p, asked = s.p, s.extra["h_asked"]
    G = LS.grid_of(p, asked)
    h = asked * 1.26 * 1.26 * 1.26
    assert G.h == h                                          # enlarged three times: 435^2 x 4613, 346^2 x 3661, 275^2 x 2906 cells
    for q in range(3):
        hq = asked * [1.0, 1.26, 1.26 * 1.26][q]
        assert (np.ceil(2 * p.R_oa / hq) + 2) ** 2 * (np.ceil(p.H / hq) + 2) >= 2.0e8
    gx, gz = int(np.ceil(2 * p.R_oa / h)) + 2, int(np.ceil(p.H / h)) + 2
    assert (G.gx, G.gz) == (gx, gz) and gx * gx * gz < 2.0e8
    # layers: the caps keep the full window, the body has the narrow one
    cr = p.collision_range
    kb = int(np.floor((p.h_oa + 2 * h + cr) / h)) + 1        # first k with -h + k h > h_oa + h + cr
    assert (G.lay_n[:kb] == gx).all() and G.lay_n[kb] < gx and G.lay_n[kb - 1] == gx
    w_lo = int(np.floor((-p.R_g - cr + p.R_oa + h) / h)) - 1
    w_n = int(np.floor((p.R_g + cr + p.R_oa + h) / h)) + 1 - w_lo + 1
    assert G.lay_lo[kb] == w_lo and G.lay_n[kb] == w_n
    assert G.lay_off[kb] == kb * gx * gx and G.lay_off[kb + 2] == kb * gx * gx + 2 * w_n * w_n
    top = int(np.flatnonzero(G.lay_n < gx)[-1])
    assert (G.lay_n[top + 1:] == gx).all() and G.ncells == (gz - (top - kb + 1)) * gx * gx + (top - kb + 1) * w_n * w_n
    x_of = lambda k: -p.R_oa - h + (k + 0.5) * h
    z_of = lambda k: -h + (k + 0.5) * h
    ca = gx // 2                                              # a cell on the axis
    # cap layer; body layer inside the window; body layer beyond the window on either side: clamped and flagged
    xs = np.array([x_of(ca), x_of(ca + 3), x_of(w_lo - 4), x_of(w_lo + w_n + 2), x_of(w_lo), x_of(w_lo + w_n - 1)])
    ys = np.array([x_of(ca + 1), x_of(ca - 2), x_of(ca), x_of(ca), x_of(w_lo), x_of(w_lo + w_n - 1)])
    zs = np.array([z_of(kb - 1), z_of(kb), z_of(kb + 1), z_of(kb + 1), z_of(kb + 5), z_of(kb + 5)])
    c, outside = LS.filed_cell(p, asked, xs, ys, zs)
    body = lambda k: kb * gx * gx + (k - kb) * w_n * w_n
    assert c.tolist() == [((kb - 1) * gx + ca + 1) * gx + ca,
                          body(kb) + (ca - 2 - w_lo) * w_n + (ca + 3 - w_lo),
                          body(kb + 1) + (ca - w_lo) * w_n + 0,
                          body(kb + 1) + (ca - w_lo) * w_n + (w_n - 1),
                          body(kb + 5), body(kb + 5) + w_n * w_n - 1]
    assert outside.tolist() == [False, False, True, True, False, False]


def test_movers_per_wave_counts_by_hand():
    """six particles in two 'waves' of three, K = 3: counters grow by the particles that change cell and fall to zero at the
    full build"""
    s = LS.catalogue("cube", "identity", "wide", 3)
    p, h = s.p, s.extra["h_asked"]
    at = lambda k: -h + (np.asarray(k) + 0.5) * h
    cells = [[5, 5, 5, 5, 5, 5], [6, 5, 5, 5, 5, 4], [7, 5, 6, 5, 5, 4], [8, 5, 6, 5, 5, 4], [8, 6, 6, 5, 5, 4], [8, 6, 6, 5, 5, 4]]
    pre = [(at(c), at([9] * 6), at([9] * 6)) for c in cells]
    counts, outside = LS.movers_per_wave(p, h, pre, 3, wave=np.arange(6) // 3, nwaves=2)
    assert counts.tolist() == [[0, 0], [1, 1], [3, 1], [0, 0], [1, 0], [1, 0]] and not outside.any()
    assert LS.expected_stats(counts, 3) == [(0, 0, 0, 1), (1, 2, 1, 1), (2, 4, 3, 1), (0, 0, 0, 2), (1, 1, 1, 2), (2, 1, 1, 2)]
