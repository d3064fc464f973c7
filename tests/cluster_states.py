"""Crafted clusters, each one side of a limit written into the wide cluster kernel (k_clusters_wide, amc_clusters.hip):
isolated pair, chain of two candidates, the one-lane 3-member path, the pair that pulls one particle in and continues from
its hit, RS_COOP_MAX = 11, CW_MAXM = 16 particles, CW_MAXC = 24 candidates, CW_PULLS = 4, CW_ITERS = 3, CW_ITEMS = 192, a
pulled particle that no longer fits, and the two halves of the validation.

Pure NumPy and deterministic (no random numbers).  Lengths below are in collision ranges (cr) and describe the state AFTER
the drift, which is what the detector sees; velocities are so small (0.05 cr per step) that a cluster stays at its site for
the few steps the tests run, and where a rebound lands depends on the geometry only: a head-on pair s apart ends 2 - s
apart, each particle 1 - s further out.

Sites: every cluster sits alone in the middle of one half of a reference cell, about 30 cr from the next site and clear of
the cell faces and their overlap strips, of walls and of the bounds thresholds.

Distance rule: after the drift no two particles are between 0.9 and 1.1 cr apart, so neither the single-precision list
records nor the widened probe radius (cr (1 + delta), amc_api.hip setup_grid) decides a candidate; ``distance_rule`` checks
it against the true band of the geometry.

Index permutations: ``identity``, ``reversed`` and ``interleaved`` (even rows first, then odd rows).  The in-place i > j
order of the reference (Pore:168-169) is by particle index, the kernel sorts members ascending and the detector numbers the
candidates, so the permutation decides the emulation order, the cluster's owner, via_x / via_y and where a pulled particle
is inserted.  Cases whose POINT is an index order (the bystander below / between / above the pair, the pulls that must
cascade, the conflicting pairs) pin the relative order of their own particles and keep it under every permutation; all
other clusters take whatever order the permutation gives them.  Where a pulled particle is inserted is covered by the
below / between / above variants of ``pair_pull1`` on the one-lane path and by ``pulls_low`` (in front of and between the
members) against ``pulls_4`` (behind them) on the cooperative path.

CW_ITERS fence (read off the kernel's loop): a cluster is emulated in the first trip of the loop, again with what it pulled
in in the second, and with what THAT pulled in in the third and last trip; a cluster that pulls again there is handed over
with a self edge.  So ``pull_depth_2`` is finished by the wide kernel and ``pull_depth_3`` is the first that is handed
over (``pull_depth_4`` as well): the fence is at depth 3.

Hits per candidate: a cluster can publish two hits per candidate (the history pairs its candidates brought along); one more
and it is flagged for the ordered workgroup.  A pair that pulls two particles in (``pair_pull2``: three hits, one
candidate) is therefore handed over, and the clusters that test CW_PULLS and CW_ITERS start from four candidates
(``_based``), so that the hit count is not what hands them over.
"""
from __future__ import annotations

import numpy as np

from argon_monte_carlo_amd import params as PR
from tests.edge_states import EdgeState

PERMS = ("identity", "reversed", "interleaved")
KINDS = ("cube", "pore")
# one state with everything the wide kernel must finish alone, one per reason to hand a cluster to the ordered workgroup
HANDOVER = ("chain_17", "cand_25", "clique_8", "full_pull", "pulls_5", "pull_depth_3", "pull_depth_4", "pair_pull2",
            "conflict_overlay", "conflict_grid")
WHICH = ("within",) + HANDOVER + ("items_over", "items_fit")
WITHIN_CASES = ("pair", "pair_pull1", "pulls_4", "pulls_low", "pull_depth_2", "chain2", "triangle", "chain_4", "chain_11",
                "chain_12", "chain_16", "cand_24")
# what structure() must find per case: (particles, candidates) of every component of the case
KNOWN = {"pair": (2, 1), "pair_pull1": (2, 1), "pair_pull2": (2, 1), "pulls_4": (4, 4), "pulls_5": (4, 4), "pulls_low": (4, 4),
         "pull_depth_2": (4, 4), "pull_depth_3": (4, 4), "pull_depth_4": (4, 4), "chain2": (3, 2), "triangle": (3, 3),
         "chain_4": (4, 3), "chain_11": (11, 10), "chain_12": (12, 11), "chain_16": (16, 15), "chain_17": (17, 16),
         "cand_24": (10, 24), "cand_25": (11, 25), "clique_8": (8, 28), "full_pull": (16, 15), "conflict_overlay": (2, 1),
         "conflict_grid": (2, 1), "items_over": (2, 1), "items_fit": (2, 1)}
CW_MAXM, CW_MAXC = 16, 24


def _params(kind):
    if kind == "cube":
        return PR.cube_params(n=0, cube_side=100.0e-9, n_sub=5)
    return PR.pore_params(n=0)


def probe_band(p):
    """delta of the widened probe radius crp = cr (1 + delta): setup_grid's arithmetic (amc_api.hip), per geometry"""
    cr = p.collision_range
    if p.geometry == 1:
        xlo, xhi, zlo, zhi = 0.0, max(p.cube_x, p.cube_y), 0.0, p.cube_z
    else:
        xlo, xhi, zlo, zhi = -p.R_oa, p.R_oa, 0.0, p.H
    extent = 1.05 * max(xhi - xlo, zhi - zlo) + 8 * cr
    return max(1.0e-6, 16.0 * extent * 5.9604644775390625e-08 / cr)


def _sites(kind, p):
    """site centres: the middle of each half of a reference cell along every axis (pitch d / 2, about 30 cr)"""
    if kind == "cube":
        ax = [(k + f) * p.dx for k in range(p.nx) for f in (0.25, 0.75)]
        return [(x, y, z) for z in ax for y in ax for x in ax]
    ax = [(k + f) * p.dx for k in range(-5, 5) for f in (0.25, 0.75)]
    zs = [(k + f) * p.dz for k in range(0, 4) for f in (0.25, 0.75)]        # the bottom open-air cap
    return [(x, y, z) for z in zs for y in ax for x in ax if np.hypot(x, y) < 110.0e-9]


def _rank(r0, m, perm):
    """the relative order rows r0 .. r0 + m - 1 have after the permutation: rank[k] of local row k"""
    rows = np.arange(r0, r0 + m)
    key = {"identity": rows, "reversed": -rows, "interleaved": (rows % 2) * (1 << 20) + rows}[perm]
    return np.argsort(np.argsort(key))


def _vel(k):
    """a distinct, small direction per k (components in -1 .. 1)"""
    return np.array([((k * 7) % 5 - 2) / 2.0, ((k * 3) % 7 - 3) / 3.0, ((k * 5) % 3 - 1) / 1.0])


class _Builder:
    def __init__(self, kind, perm):
        self.kind, self.perm = kind, perm
        self.p, c = _params(kind)
        self.dt = c["dt"]
        self.cr = self.p.collision_range
        self.v0 = 0.05 * self.cr / self.dt
        self.sites = iter(_sites(kind, self.p))
        self.rows = []          # (case, site, post-drift position, velocity)
        self.nsite = 0
        self.info = {}          # case -> list of {role: row}
        self.absent = []

    def put(self, case, pts, vels, pinned=None, roles=None, exact=()):
        """One cluster at the next site.  pts: offsets in cr after the drift; vels in units of v0; pinned: the final index
        order of the points (pinned[k] = rank of point k), kept under every permutation; exact: points whose velocity gets
        no per-row jitter.  Returns {role or k: row}."""
        try:
            ctr = np.array(next(self.sites))
        except StopIteration:
            self.absent.append(case)
            return None
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        vels = np.asarray(vels, dtype=np.float64).reshape(-1, 3)
        pts = pts - 0.5 * (pts.min(axis=0) + pts.max(axis=0))          # centred on the site
        m, r0 = len(pts), len(self.rows)
        order = np.arange(m)
        if pinned is not None:
            rank = _rank(r0, m, self.perm)
            order = np.array([int(np.flatnonzero(rank == pinned[k])[0]) for k in range(m)])       # point k -> local row
        slot = [None] * m
        for k in range(m):
            v = vels[k] * self.v0
            if k not in exact:
                v = v + self.v0 * 1.0e-3 * np.array([0.0, 1 + (r0 + k) % 11, 1 + (r0 + k) % 7])
            slot[order[k]] = (case, self.nsite, ctr + pts[k] * self.cr, v)
        self.rows += slot
        self.nsite += 1
        out = {(roles[k] if roles else k): r0 + int(order[k]) for k in range(m)}
        self.info.setdefault(case, []).append(out)
        return out

    def finish(self):
        n = len(self.rows)
        rows = np.arange(n)
        key = {"identity": rows, "reversed": -rows, "interleaved": (rows % 2) * (1 << 20) + rows}[self.perm]
        order = np.argsort(key, kind="stable")          # new index q holds row order[q]
        new_of = np.empty(n, dtype=np.int64)
        new_of[order] = np.arange(n)
        s = EdgeState(self.p, self.dt)
        for q in range(n):
            case, site, pos, v = self.rows[order[q]]
            start = pos - self.dt * v
            s.add(case, *start, *v, flag=1, landed=False, jitter=False)    # (flag set: every hit leaves a record)
        s.finish()
        s.p.reserved1 = 1               # (the equal-velocity pair's solve has a == 0: counted, not fatal)
        s.extra["site"] = np.array([self.rows[order[q]][1] for q in range(n)], dtype=np.int64)
        s.extra["roles"] = {case: [{r: int(new_of[row]) for r, row in d.items()} for d in lst]
                            for case, lst in self.info.items()}
        s.extra["absent"] = list(self.absent)
        s.extra["kind"], s.extra["perm"] = self.kind, self.perm
        return s


# ---------------------------------------------------------------------------------------------------------------- the cases
X = np.array([1.0, 0.0, 0.0])


def _line(xs):
    return [[x, 0.0, 0.0] for x in xs]


def _head_on(b, case, s, extra_pts=(), extra_roles=(), pinned=None, exact=()):
    """A at 0 moving +x, B at s moving -x (after their hit: A at -(1 - s), B at 1), plus particles at rest"""
    pts = _line([0.0, s]) + list(extra_pts)
    vels = [X, -X] + [[0.0, 0.0, 0.0]] * len(extra_pts)
    return b.put(case, pts, vels, pinned=pinned, roles=["A", "B"] + list(extra_roles), exact=exact)


def _pair(b):
    _head_on(b, "pair", 0.5)
    # obliquely: the line of centres and the relative velocity 40 degrees apart
    u = np.array([0.6, 0.64, 0.48])
    b.put("pair", [[0, 0, 0], 0.6 * u], [[0.9, 0.1, 0.3], [-0.7, -0.5, 0.2]], roles=["A", "B"])
    # equal velocities: a == 0 in the contact solve (counted with reserved1 bit0; the pair is left alone)
    b.put("pair", _line([0.0, 0.7]), [[0.5, 0.25, 0.0]] * 2, roles=["A", "B"], exact=(0, 1))


def _pair_pull1(b, case="pair_pull1", copies=1, only=None):
    # the bystander C rests 1.1 behind A: 0.6 from where A's rebound ends.  By C's index: below both, between, above both
    variants = {"below": (1, 2, 0), "between": (0, 2, 1), "above": (0, 1, 2)}
    for _ in range(copies):
        for name, pinned in variants.items():
            if only is None or name == only:
                _head_on(b, case, 0.5, _line([-1.1]), ["C"], pinned=pinned)


def _pair_pull2(b):
    # bystanders behind both ends: three hits on ONE candidate.  A cluster publishes at most two hits per candidate (the
    # history pairs 4c and 4c + 2 its candidates brought, rs_hit): the third takes counter-allocated entries and the
    # cluster is flagged for the ordered workgroup — pair_pull1 (two hits) is the other side of that fence
    _head_on(b, "pair_pull2", 0.5, _line([-1.1, 1.6]), ["C", "D"], pinned=(0, 1, 2, 3))


def _based(b, case, extra_pts, extra_roles, pinned=None):
    """The cluster the pulls start from: the head-on pair A (0) B (0.2) — A's rebound ends at -0.8, B's at 1 — and, to bring
    candidates (two publishable hits each), P2 within range of both and P3 beyond it: 4 particles, 4 candidates, room for
    8 hits.  P2 and P3 meet head-on across the line and stay 1.16 or more from every outsider.  Ascending indices, the
    outsiders last and in the order they are reached, so that every hit happens — unless `pinned` says otherwise."""
    u = np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
    p2 = np.array([0.2, 0.6, 0.6])
    pts = _line([0.0, 0.2]) + [p2, p2 + 0.8 * u] + list(extra_pts)
    vels = [X, -X, u, -u] + [[0.0, 0.0, 0.0]] * len(extra_pts)
    return b.put(case, pts, vels, pinned=pinned or tuple(range(len(pts))), roles=["A", "B", "P2", "P3"] + list(extra_roles))


def _pulls(b, n):
    # n outsiders 0.85 from where A's rebound ends, 1.17 or more from where A and B were and 1.2 from each other
    ring = [[-0.8, 0.85, 0.0], [-0.8, -0.85, 0.0], [-0.8, 0.0, 0.85], [-0.8, 0.0, -0.85], [-1.65, 0.0, 0.0]][:n]
    _based(b, f"pulls_{n}", ring, [f"O{k}" for k in range(n)])


def _pulls_low(b):
    # the cooperative path with the pulled particles at LOW indices: O0 below everybody, O1 between A and B.  Both are
    # tested against A before A's hit and never again (Pore:168-169), so the oracle hits neither; the kernel pulls both in
    # (its grid half sees A's rebound 0.85 from them), inserts them in front of and between its members and must find the
    # re-emulation without a hit on them.  Index order O0 A O1 B P2 P3.
    _based(b, "pulls_low", [[-0.8, 0.85, 0.0], [-0.8, -0.85, 0.0]], ["O0", "O1"], pinned=(1, 3, 4, 5, 0, 2))


def _pull_depth(b, depth):
    # a cradle: A's rebound (to -0.8) reaches C, C's reaches D, ...: each rests 1.1 or more from everybody before the sweep
    # and 0.4, 0.5, 0.6, 0.7 from where its neighbour's rebound ends
    xs = [-1.2, -2.3, -3.4, -4.5][:depth]
    _based(b, f"pull_depth_{depth}", _line(xs), ["C", "D", "E", "F"][:depth])


def _chain2(b):
    # P0 - S - P1 with the shared particle S at the lowest, middle and highest index
    for pinned in ((1, 0, 2), (0, 1, 2), (0, 2, 1)):
        b.put("chain2", _line([0.0, 0.8, 1.6]), [X, -X, X], pinned=pinned, roles=["P0", "S", "P1"])


def _triangle(b):
    h = 0.8 * np.sqrt(3.0) / 2.0
    b.put("triangle", [[0, 0, 0], [0.8, 0, 0], [0.4, h, 0]], [[0.5, 0.3, 0], [-0.5, 0.3, 0], [0, -0.6, 0.1]])


def _chain_pts(n):
    # 0.8 apart, velocities across the chain and alternating: every link hits, nobody is thrown far
    pts = _line([0.8 * m for m in range(n)])
    vels = [[0.1 * ((m % 3) - 1), 1.0 if m % 2 else -1.0, 0.0] for m in range(n)]
    return pts, vels


def _chain(b, n):
    b.put(f"chain_{n}", *_chain_pts(n))


OCTA = [[0, 0, 0], [0.4, 0, 0], [-0.4, 0, 0], [0, 0.4, 0], [0, -0.4, 0], [0, 0, 0.4], [0, 0, -0.4]]


def _cand(b, n):
    # a 7-clique (centre + octahedron of radius 0.4: 21 candidates) and pendants 0.85 beyond one vertex each
    pend = [[1.25, 0, 0], [-1.25, 0, 0], [0, 1.25, 0], [0, -1.25, 0]][:n - 21]
    pts = OCTA + pend
    b.put(f"cand_{n}", pts, [_vel(k) for k in range(len(pts))])


def _clique8(b):
    pts = [[0.5 * i, 0.5 * j, 0.5 * k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    b.put("clique_8", pts, [_vel(k + 3) for k in range(8)])


def _full_pull(b):
    # a 16-chain (CW_MAXM members already) whose end E0 meets E1 head-on, 0.6 apart: its rebound ends 0.4 further out,
    # 0.7 from an outsider that rested 1.1 away.  Ascending indices from the outsider's end: the hit E1-E0 comes first.
    pts, vels = _chain_pts(16)
    pts[1] = [0.6, 0.0, 0.0]
    pts[2] = [1.3, 0.35, 0.0]           # (0.78 from E1; the rest of the chain follows 0.8 apart)
    for m in range(3, 16):
        pts[m] = [1.3 + 0.8 * (m - 2), 0.35, 0.0]
    vels[0], vels[1] = [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]
    b.put("full_pull", pts + [[-1.1, 0.0, 0.0]], vels + [[0.0, 0.0, 0.0]], pinned=tuple(range(17)),
          roles=[f"P{m}" for m in range(16)] + ["C"])


def _conflict_overlay(b):
    # A B ... C D on a line, both pairs 0.5 apart, B and C 1.65 apart: B's rebound ends 1.15 from where C WAS (the grid
    # half sees nothing) and 0.65 from where C's rebound ends (the overlay half must).  Index order A D B C: both hits come
    # before the test of C against B, which then hits; A B D C: the oracle never tests them again.
    for pinned in ((0, 2, 3, 1), (0, 1, 3, 2)):
        b.put("conflict_overlay", _line([0.0, 0.5, 2.15, 2.65]), [X, -X, X, -X], pinned=pinned, roles=["A", "B", "C", "D"])


def _conflict_grid(b):
    # A B ... C D, both pairs 0.8 apart, B and C 1.1 apart: B's rebound ends 0.9 from where C is before the sweep —
    # the grid half's merge edge (C is in a candidate).  Ascending indices: the test of C against B follows the hit A-B.
    for pinned in ((0, 1, 2, 3), (0, 2, 3, 1)):
        b.put("conflict_grid", _line([0.0, 0.8, 1.9, 2.7]), [X, -X, X, -X], pinned=pinned, roles=["A", "B", "C", "D"])


def catalogue(kind, perm, which="within"):
    """The crafted state ``which`` (see WHICH) in geometry ``kind`` under index permutation ``perm``.

    extra["roles"][case]: per cluster of the case, {role: particle index}; extra["site"]: the site of every particle;
    extra["absent"]: cases that found no site (a test asserts there are none)."""
    b = _Builder(kind, perm)
    if which == "within":
        _pair(b); _pair_pull1(b); _pulls(b, 4); _pulls_low(b); _pull_depth(b, 2); _chain2(b); _triangle(b)
        for n in (4, 11, 12, 16):
            _chain(b, n)
        _cand(b, 24)
    elif which in ("items_over", "items_fit"):
        # copies of pair_pull1 whose bystander is hit: every copy is one candidate with two hits = four new positions, so
        # the 64 candidates of one wave and pass bring 256 > CW_ITEMS whichever way the detector numbers them; 40 copies fit
        _pair_pull1(b, which, copies=80 if which == "items_over" else 40, only="above")
    else:
        _head_on(b, "pair", 0.5)        # (company: an ordinary pair beside the cluster that is handed over)
        {"chain_17": lambda: _chain(b, 17), "cand_25": lambda: _cand(b, 25), "clique_8": lambda: _clique8(b),
         "full_pull": lambda: _full_pull(b), "pulls_5": lambda: _pulls(b, 5), "pull_depth_3": lambda: _pull_depth(b, 3),
         "pull_depth_4": lambda: _pull_depth(b, 4), "pair_pull2": lambda: _pair_pull2(b),
         "conflict_overlay": lambda: _conflict_overlay(b),
         "conflict_grid": lambda: _conflict_grid(b)}[which]()
    s = b.finish()
    s.extra["which"] = which
    return s


# ---------------------------------------------------------------------------------------------------------------- structure
def drifted(s):
    """the positions the detector sees: the drift's own arithmetic (no wall and no bound is near a site)"""
    return np.stack([s.x + s.dt * s.vx, s.y + s.dt * s.vy, s.z + s.dt * s.vz], axis=1)


def _distances(s):
    P = drifted(s)
    d = P[:, None, :] - P[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def structure(s):
    """The candidate graph the detector must find after drift and walls.

    Returns dict(pairs = (k, 2) array of i < j with distance < cr, comp = component label per particle (-1: in no
    candidate), components = list of dict(particles = sorted indices, candidates = count))."""
    D = _distances(s)
    cr = s.p.collision_range
    i, j = np.nonzero(np.triu(D < cr, k=1))
    pairs = np.stack([i, j], axis=1)
    parent = np.arange(s.n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, c in pairs:
        ra, rc = find(a), find(c)
        if ra != rc:
            parent[max(ra, rc)] = min(ra, rc)
    comp = np.full(s.n, -1, dtype=np.int64)
    comps = {}
    for a, c in pairs:
        r = find(a)
        e = comps.setdefault(r, dict(particles=set(), candidates=0))
        e["particles"] |= {int(a), int(c)}
        e["candidates"] += 1
    out = []
    for q, r in enumerate(sorted(comps)):
        e = comps[r]
        e["particles"] = sorted(e["particles"])
        comp[e["particles"]] = q
        out.append(e)
    return dict(pairs=pairs, comp=comp, components=out)


def distance_rule(s):
    """the distances (in cr) that fall inside [cr (1 - 2 delta), crp (1 + 2 delta)]: must be empty"""
    D = _distances(s)
    cr = s.p.collision_range
    delta = probe_band(s.p)
    lo, hi = cr * (1.0 - 2.0 * delta), cr * (1.0 + delta) * (1.0 + 2.0 * delta)
    bad = np.triu((D >= lo) & (D <= hi), k=1)
    return D[bad] / cr


def expected_waves(s):
    """What the wide kernel's per-kind wave counts must be when every candidate is lane 0 of its own wave: the owner of a
    component within CW_MAXM / CW_MAXC counts by its particles (pair, 3-cluster, 4+-cluster); every other candidate's
    lane — and every lane of a component beyond the limits — is "not owner"."""
    st = structure(s)
    out = {"pair": 0, "3-cluster": 0, "4+-cluster": 0, "not owner": 0}
    for c in st["components"]:
        m, nc = len(c["particles"]), c["candidates"]
        if m > CW_MAXM or nc > CW_MAXC:
            out["not owner"] += nc
            continue
        out["pair" if m == 2 else ("3-cluster" if m == 3 else "4+-cluster")] += 1
        out["not owner"] += nc - 1
    return out


# cases in which a pair pulls exactly one particle in at its first validation: the `cont` path (rs_first_hit)
CONT_CASES = ("pair_pull1", "items_over", "items_fit")
PULL_CASES = CONT_CASES + ("pair_pull2", "pulls_4", "pulls_5", "pulls_low", "pull_depth_2", "pull_depth_3", "pull_depth_4", "full_pull")


def expected_cont(s):
    """how many clusters take the `cont` path, and how often the one-lane 3-member path runs (3-particle components once
    each, plus every continuation)"""
    roles = s.extra["roles"]
    cont = sum(len(roles.get(c, [])) for c in CONT_CASES)
    three = sum(1 for c in structure(s)["components"] if len(c["particles"]) == 3)
    return cont, three + cont
