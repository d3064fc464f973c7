"""Crafted states, each one side of a size fence written into the ordered resolve workgroup (k_resolve, amc_resolve.hip;
helpers in amc_resolve_dev.h).  Pure NumPy and deterministic (no random numbers), in the style of tests/cluster_states.py,
whose point sets, site layout, ``structure()`` and distance rule are reused.

The fences (read off the kernel):

    wide_ns + 2 * nleft + 256 <= RS_NS (6144)   slot labels / sizes / dirty flags in LDS | in the global work space
    3 * gz <= RS_LAY (4096)                     grid layer tables in LDS | read from global memory
    nc <= 64                                    "split": wave 0 does the clusters beside the pair phase | bitonic sort, pairs first
    split, cluster heads <= 2                   clusters in turn on wave 0 | heads published, one cluster per wave
    members of one cluster <= RS_COOP_MAX (11)  rs_emulate_coop (a wave) | rs_emulate_generic (one lane)
    nc <= RS_POOL (256)                         working set in LDS | in W.cw_* (global)
    nc <= RS_SORT_LDS (2048)                    keys sorted in LDS | in W.sl_key (global)
    round 1 | later rounds                      label propagation | rs_union / rs_find over the new edges, touched clusters only
    rounds >= RS_MAX_ROUNDS (256)               clean in round 256 is good | still dirty: flag 4, AMC_ERR_CAPACITY
    slots <= W.max_slots                        validation claims a slot for every particle it pulls in | ovf, AMC_ERR_CAPACITY

nc = members of the dirty clusters with three or more particles in one round.

Family A (``cells()``): single cells for Engine.pairwise_cell / O.pair_cell — MODE 2, the ordered workgroup is the whole
sweep, the order of the reference is all i > j by index.  Lengths are in collision ranges.  A head-on pair s apart ends 2 - s
apart (tests/cluster_states.py); a particle at rest that a moving one meets g < 1 away takes its velocity and ends 1 - g
further on, while the moving one stops one range short of where the resting one was.  ``cascade_k`` is a row at rest with
spacing 1 + eps behind a head-on pair: the gap grows by eps per member, every round's last rebound pulls exactly the next
particle, and the sweep needs k + 1 rounds (read from the GPU's n_rounds on cascade_2, _3, _4 before it is relied on).

Family B (``grid_state()``): the same fences behind the wide cluster kernel in the cube and the pore, on cluster_states'
sites: chain_17 components, which the wide kernel can only hand over.

``mirror()`` is a host model of the rounds (clusters, literal emulation in index order, validation of every new position
against every particle and every other cluster's new positions, merge, re-emulation of what the edges touch): it gives the
number of rounds, the complex members and the emulated clusters of every round, and the slots claimed."""
from __future__ import annotations

import numpy as np

from argon_monte_carlo_amd import params as PR
from tests import cluster_states as CS

FIELDS = ("cont", "cx", "cy", "cz", "flag", "x", "y", "z", "vx", "vy", "vz")
RS_NS, RS_LAY, RS_SPLIT, RS_POOL, RS_SORT_LDS, RS_COOP_MAX, RS_MAX_ROUNDS = 6144, 4096, 64, 256, 2048, 11, 256
CR2_INFLATE = 1.0 + 1.0e-9
SPEED = 250.0                           # m / s
PITCH, PER_ROW = (16.0, 6.0, 6.0), 16   # site lattice of a cell: the longest part (a chain of 12) is 8.8 long
BASE = np.array([1.0e-8, -2.0e-8, 1.2e-6])
ROW_AT = np.array([0.0, -40.0, 0.0])    # where a cascade's row starts: beside the lattice, which has y >= 0
CASCADE_GAP0 = 0.55                     # first resting particle: 1.05 from where B was, 0.55 from where B's rebound ends
CASCADE_EPS = 0.0015                    # gap of depth k: 0.55 + 0.0015 k (0.934 at depth 256)
N_PAIRS = 100

# the cells small enough for the reference itself (tests/golden/func_resolve.npz) | compared with the oracle only
SMALL = ("nc_64", "nc_65", "nc_256", "nc_257", "heads_2", "heads_3", "merge", "cascade_2", "cascade_3", "cascade_4", "cascade_8")
LARGE = ("nc_2048", "nc_2049", "labels_2944", "labels_2945", "cascade_255", "pulls_2900")
FAILING = ("cascade_256", "slots_full")             # AMC_ERR_CAPACITY: round 257 / the slot table really full
CELLS = SMALL + LARGE + FAILING
MAX_CANDIDATES = {"slots_full": 1100}               # p.max_candidates (0: the default capacities)


def default_capacities(n, max_candidates=0):
    """alloc_resolve_ws (amc_api.hip): (max_cand, max_slots) of a context of n particles"""
    mc = max_candidates if max_candidates > 0 else max(4096, n // 8 + 1024)
    return mc, 2 * mc + max(1024, mc // 2)


class Cell:
    """one cell: the eleven arrays of pairwise_particles_in_cell, and which particles belong to which part"""

    def __init__(self, name, p, arrays, parts):
        self.name, self.p, self.arrays, self.parts = name, p, arrays, parts
        self.n = len(arrays["x"])

    def args(self):
        """fresh contiguous copies in the order of FIELDS (flag as uint8): Engine.pairwise_cell works in place"""
        return [np.ascontiguousarray(self.arrays[f], dtype=np.uint8 if f == "flag" else np.float64).copy() for f in FIELDS]

    def of(self, kind):
        return [idx for k, idx in self.parts if k == kind]


class _CellBuilder:
    def __init__(self, name):
        self.name = name
        self.p = PR.cell_params(n=0)[0]
        self.pos, self.vel, self.parts, self.nsite = [], [], [], 0

    def put(self, kind, pts, vels, exact=False, at=None):
        """one part at the next site of the lattice (or at `at`), its first point on the site, indices ascending"""
        if at is None:
            k = self.nsite
            self.nsite += 1
            at = np.array([(k % PER_ROW) * PITCH[0], (k // PER_ROW % PER_ROW) * PITCH[1], (k // PER_ROW ** 2) * PITCH[2]])
        pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
        vels = np.asarray(vels, dtype=np.float64).reshape(-1, 3)
        r0 = len(self.pos)
        for k in range(len(pts)):
            v = vels[k]
            if not exact:
                v = v + 1.0e-3 * np.array([0.0, 1 + (r0 + k) % 11, 1 + (r0 + k) % 7])
            self.pos.append(at + pts[k] - pts[0])
            self.vel.append(v)
        self.parts.append((kind, list(range(r0, r0 + len(pts)))))

    # ---- the parts
    def pairs(self, m):
        for _ in range(m):
            self.put("pair", CS._line([0.0, 0.5]), [CS.X, -CS.X])

    def triangles(self, m):
        h = 0.8 * np.sqrt(3.0) / 2.0
        for _ in range(m):
            self.put("triangle", [[0, 0, 0], [0.8, 0, 0], [0.4, h, 0]], [[0.5, 0.3, 0], [-0.5, 0.3, 0], [0, -0.6, 0.1]])

    def chain(self, k):
        self.put(f"chain_{k}", *CS._chain_pts(k))

    def complex_members(self, nc):
        """exactly nc members of clusters with three or more particles: triangles and one short chain"""
        k = next(k for k in (3, 4, 5) if (nc - k) % 3 == 0)
        self.triangles((nc - k) // 3)
        self.chain(k)

    def pulls(self, m):
        # cluster_states' pair_pull1 with the bystander above both: A's rebound ends 0.6 from C, and C is hit
        for _ in range(m):
            self.put("pull", CS._line([0.0, 0.5, -1.1]), [CS.X, -CS.X, [0.0, 0.0, 0.0]], exact=True)

    def cascade(self, depth):
        xs = [0.0, 0.5] + [1.0 + CASCADE_GAP0 + (1.0 + CASCADE_EPS) * k for k in range(depth)]
        self.put(f"cascade_{depth}", CS._line(xs), [CS.X, -CS.X] + [[0.0, 0.0, 0.0]] * depth, exact=True, at=ROW_AT)

    def finish(self):
        cr = self.p.collision_range
        n = len(self.pos)
        P = np.array(self.pos).reshape(n, 3) * cr + BASE
        V = np.array(self.vel).reshape(n, 3) * SPEED
        k = np.arange(n)
        a = dict(cont=(5.0 + 0.01 * (k % 17)) * cr, cx=(2.0 + 0.01 * (k % 13)) * cr, cy=(3.0 + 0.01 * (k % 11)) * cr,
                 cz=(2.5 + 0.01 * (k % 7)) * cr, flag=np.ones(n, dtype=np.uint8), x=P[:, 0], y=P[:, 1], z=P[:, 2], vx=V[:, 0],
                 vy=V[:, 1], vz=V[:, 2])            # (flag set: every hit leaves its two records)
        p = PR.cell_params(n=n)[0]
        p.max_candidates = MAX_CANDIDATES.get(self.name, 0)
        return Cell(self.name, p, a, self.parts)


def cell(name):
    b = _CellBuilder(name)
    kind, _, num = name.partition("_")
    if kind == "nc":
        # the split / pool / sort fences; the pair phase runs beside (split) or in front of (sorted) the cluster phase
        b.complex_members(int(num))
        b.pairs(N_PAIRS)
    elif kind == "heads":
        # split with 2 | 3 heads: a cluster of 11 (coop) and one of 12 (generic), on wave 0 | on the shared waves
        b.chain(11)
        b.chain(12)
        if num == "3":
            b.triangles(1)
        b.pairs(N_PAIRS)
    elif kind == "labels":
        # candidates on either side of 2 * nleft + 256 <= RS_NS, no pull: pairs, and one triangle for the cluster phase
        b.triangles(1)
        b.pairs(int(num) - 3)
    elif name == "merge":
        # (i) history against history: cluster_states' conflict_overlay, in the index order whose hit B-C the reference makes
        # (A D B C) and in the one where it never tests them again (A B D C)
        for order in ((0, 2, 3, 1), (0, 1, 3, 2)):
            xs = np.array([0.0, 0.5, 2.15, 2.65])[np.argsort(order)]
            vs = np.array([CS.X, -CS.X, CS.X, -CS.X])[np.argsort(order)]
            b.put("merge_two", CS._line(xs), vs, exact=True)
        # (ii) three pairs that merge as a chain through two edges of the same round
        b.put("merge_three", CS._line([0.0, 0.5, 2.15, 2.65, 4.3, 4.8]), [CS.X, -CS.X] * 3, exact=True)
        # (iii) what no edge touches keeps its round-1 results and records
        b.triangles(2)
        b.chain(5)
        b.pairs(20)
    elif kind == "cascade":
        b.cascade(int(num))
        b.triangles(1)
        b.pairs(10)
    elif name == "pulls_2900":
        # 5800 slots from candidates, 2900 claimed by the first validation: more than RS_NS, fewer than max_slots
        b.pulls(2900)
    elif name == "slots_full":
        # max_candidates = 1100: max_slots = 3224, the candidates bring 2200 slots and the pulls ask for 1100 more
        b.pulls(1100)
    else:
        raise KeyError(name)
    return b.finish()


# ---------------------------------------------------------------------------------------------------------------- structure
def _xyz(c):
    return np.stack([c.arrays["x"], c.arrays["y"], c.arrays["z"]], axis=1)


def close_pairs(P, r2, chunk=512, with_d2=False):
    """all i < j with squared distance < r2 (in chunks of rows: a cell holds up to 8,700 particles)"""
    out, dd = [], []
    for a in range(0, len(P), chunk):
        d2 = np.zeros((min(chunk, len(P) - a), len(P)))
        for k in range(3):
            d = P[a:a + chunk, None, k] - P[None, :, k]
            d2 += d * d
        i, j = np.nonzero(d2 < r2)
        keep = (i + a) < j
        out.append(np.stack([i[keep] + a, j[keep]], axis=1))
        dd.append(d2[i[keep], j[keep]])
    pairs = np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
    return (pairs, np.concatenate(dd) if dd else np.zeros(0)) if with_d2 else pairs


class _Sets:
    def __init__(self, n):
        self.parent = np.arange(n)

    def find(self, a):
        p = self.parent
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        return int(a)

    def union(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            self.parent[max(ra, rb)] = min(ra, rb)


def cell_structure(c):
    """the candidate graph of a cell: pairs (i < j within the detector's radius), the components as sorted particle lists
    with their candidate counts, nc of the first round"""
    cr = c.p.collision_range
    pairs = close_pairs(_xyz(c), cr * cr * CR2_INFLATE)
    S = _Sets(c.n)
    for a, b in pairs:
        S.union(a, b)
    comps = {}
    for a, b in pairs:
        e = comps.setdefault(S.find(a), dict(particles=set(), candidates=0))
        e["particles"] |= {int(a), int(b)}
        e["candidates"] += 1
    comps = [dict(particles=sorted(e["particles"]), candidates=e["candidates"]) for _, e in sorted(comps.items())]
    return dict(pairs=pairs, components=comps, nc=sum(len(e["particles"]) for e in comps if len(e["particles"]) >= 3),
                slots=sum(len(e["particles"]) for e in comps))


# ---------------------------------------------------------------------------------------------------------------- host mirror
def _collide(X, V, j, i, cr):
    """the contact solve and the elastic exchange of the reference's pair loop, exact squares; in place"""
    e = X[i] - X[j]
    u = V[j] - V[i]
    a, b, c = u @ u, 2.0 * (e @ u), e @ e - cr * cr
    if a == 0.0:
        return False
    root = np.sqrt(b * b - 4.0 * a * c)
    t = max((-b + root) / (2.0 * a), (-b - root) / (2.0 * a))
    r1, r2 = X[j] - V[j] * t, X[i] - V[i] * t
    nrm = (r2 - r1) / cr
    pm = V[j] @ nrm - V[i] @ nrm
    w1, w2 = V[j] - pm * nrm, V[i] + pm * nrm
    X[j], X[i], V[j], V[i] = r1 + w1 * t, r2 + w2 * t, w1, w2
    return True


def _emulate(P0, V0, members, cr):
    """the reference's loop over one cluster (members ascending, all a > c): [(particle, new position)] of every hit"""
    X, V = P0[members].copy(), V0[members].copy()
    out = []
    for a in range(1, len(members)):
        c0 = 0
        while c0 < a:
            d = X[c0:a] - X[a]
            near = np.flatnonzero((d * d).sum(axis=1) < cr * cr)
            if not len(near):
                break
            c = c0 + int(near[0])
            if _collide(X, V, c, a, cr):
                out += [(members[c], X[c].copy()), (members[a], X[a].copy())]
            c0 = c + 1
    return out


def _near(A, B, r2, chunk=256):
    """all (a, b) with |A[a] - B[b]|^2 < r2"""
    out = []
    for a0 in range(0, len(A), chunk):
        d2 = np.zeros((min(chunk, len(A) - a0), len(B)))
        for k in range(3):
            d = A[a0:a0 + chunk, None, k] - B[None, :, k]
            d2 += d * d
        a, b = np.nonzero(d2 < r2)
        out += zip((a + a0).tolist(), b.tolist())
    return out


def mirror(c, max_rounds=RS_MAX_ROUNDS):
    """The rounds of the ordered workgroup in MODE 2 on cell c.  Returns dict(rounds, clean, hits, claims, slots, per_round =
    [dict(nc, sizes = members of every emulated cluster, slots = slots at the round's start)])."""
    cr = c.p.collision_range
    cr2i = cr * cr * CR2_INFLATE
    P0 = _xyz(c)
    V0 = np.stack([c.arrays["vx"], c.arrays["vy"], c.arrays["vz"]], axis=1)
    st = cell_structure(c)
    S = _Sets(c.n)
    in_slot = np.zeros(c.n, dtype=bool)
    for a, b in st["pairs"]:
        S.union(a, b)
        in_slot[[a, b]] = True
    hist = {}                   # root -> [(particle, position)] of its latest emulation
    dirty, rounds, per_round, claims, edges = None, 0, [], 0, []
    while True:
        rounds += 1
        clusters = {}
        for q in np.flatnonzero(in_slot):
            clusters.setdefault(S.find(q), []).append(int(q))
        todo = sorted(clusters) if dirty is None else sorted(dirty)
        sizes, new = [], []
        for r in todo:
            sizes.append(len(clusters[r]))
            hist[r] = _emulate(P0, V0, clusters[r], cr)
            new += [(r, q, x) for q, x in hist[r]]
        per_round.append(dict(nc=sum(m for m in sizes if m >= 3), sizes=sizes, slots=int(in_slot.sum())))
        edges = []
        if new:
            others = [(r, q, x) for r, lst in hist.items() for q, x in lst]
            oroot = np.array([r for r, _, _ in others])
            opart = np.array([q for _, q, _ in others])
            opos = np.array([x for _, _, x in others])
            npos = np.array([x for _, _, x in new])
            for k, idx in _near(npos, P0, cr2i):            # every new position against every particle
                r, q, _ = new[k]
                if idx == q or (in_slot[idx] and S.find(idx) == r):
                    continue
                if not in_slot[idx]:
                    in_slot[idx] = True
                    claims += 1
                edges.append((q, int(idx)))
            for k, k2 in _near(npos, opos, cr2i):           # ... and against every other cluster's new positions
                if oroot[k2] != new[k][0]:
                    edges.append((new[k][1], int(opart[k2])))
        if not edges or rounds >= max_rounds:
            break
        for a, b in edges:
            S.union(a, b)
        dirty = {S.find(a) for a, _ in edges}
        hist = {r: lst for r, lst in hist.items() if S.find(r) == r and r not in dirty}
    return dict(rounds=rounds, clean=not edges, hits=sum(len(lst) for lst in hist.values()) // 2, claims=claims,
                slots=int(in_slot.sum()), per_round=per_round, candidates=len(st["pairs"]))


def rounds_of(c):
    """``mirror(c)``, or — for a cell made of pairs, triangles, chains and pulls only — the same record written down from the
    parts without emulating anything (the mirror takes seconds on thousands of pairs): round 1 emulates every component;
    where there are pulls, every pull pair claims its bystander and round 2 emulates the clusters of three."""
    if not all(k in ("pair", "triangle", "pull") or k.startswith("chain_") for k, _ in c.parts):
        return mirror(c)
    st = cell_structure(c)
    sizes = [len(e["particles"]) for e in st["components"]]
    per_round = [dict(nc=sum(m for m in sizes if m >= 3), sizes=sizes, slots=st["slots"])]
    pulls = len(c.of("pull"))
    if pulls:
        per_round.append(dict(nc=3 * pulls, sizes=[3] * pulls, slots=st["slots"] + pulls))
    return dict(rounds=len(per_round), clean=True, hits=len(st["pairs"]) + pulls, claims=pulls, slots=st["slots"] + pulls,
                per_round=per_round, candidates=len(st["pairs"]))


def figures(m, max_slots, wide_ns=0, nleft=None):
    """What the debug line of k_resolve must show for ONE launch whose rounds are m (a ``mirror()``), by the kernel's own
    inequalities: rounds, candidates, complex members of the last round, and per path how many rounds / clusters took it."""
    nleft = m["candidates"] if nleft is None else nleft
    f = dict(rounds=m["rounds"], cand=m["candidates"], complex_last=m["per_round"][-1]["nc"],
             labels_global=int(not (wide_ns + 2 * nleft + 256 <= RS_NS)), moved=0, split=0, shared=0, sorted=0, pool_global=0,
             sort_global=0, later=m["rounds"] - 1, by_wave=0, by_lane=0, most=max(r["nc"] for r in m["per_round"]))
    for r in m["per_round"]:
        nc, big = r["nc"], [s for s in r["sizes"] if s >= 3]
        if not f["labels_global"] and not f["moved"] and min(r["slots"], max_slots) > RS_NS:
            f["moved"] = 1
        if 0 < nc <= RS_SPLIT:
            f["split"] += 1
            f["shared"] += len(big) > 2
            f["by_wave"] += sum(s <= RS_COOP_MAX for s in big)
            f["by_lane"] += sum(s > RS_COOP_MAX for s in big)
        elif nc > 0:
            f["sorted"] += 1
            f["pool_global"] += nc > RS_POOL
            f["sort_global"] += nc > RS_SORT_LDS
            f["by_lane"] += len(big)
    return f


# ---------------------------------------------------------------------------------------------------------------- family B
GRID_STATES = ("chains_3", "chains_4", "chains_16", "chains_121", "pairs_under", "pairs_over", "pull_beside", "conflict_beside")
GRID_NC = {"chains_3": 51, "chains_4": 68, "chains_16": 272, "chains_121": 2057}
FENCE_CHAINS = {"cube": 1, "pore": 60}
SIDE = {"cube": dict(cube_side=160.0e-9, n_sub=8)}     # 16^3 sites where the 100 nm cube's 10^3 are too few


FINE = ("min", "coarse")


def fine_cell(p, fine):
    """the requested fine_cell: the smallest the library takes (a probe box then spans 8 cells) | 30 collision ranges"""
    crp = p.collision_range * (1.0 + CS.probe_band(p))
    return 2.01 * 1.02 * crp if fine == "min" else 30.0 * p.collision_range


def _grid_params(kind):
    if kind == "cube":
        return PR.cube_params(n=0, **SIDE["cube"])
    return PR.pore_params(n=0)


def label_fence_pairs(extra_candidates, extra_left):
    """the largest P for which P isolated pairs beside a component of `extra_candidates` candidates that the wide kernel
    leaves (`extra_left` of them) keep the labels in LDS: 2 * ncand + 2 * nleft + 256 <= RS_NS (every candidate owns two
    slots of the wide kernel's, and the left ones claim theirs again)"""
    return (RS_NS - 256 - 2 * extra_left) // 2 - extra_candidates


def grid_state(kind, perm, which):
    """Family B: state ``which`` in geometry ``kind`` under index permutation ``perm`` (cluster_states' builder and sites).
    extra["absent"] lists what found no site; a test asserts there is none."""
    params = CS._params
    CS._params = _grid_params               # (the builder asks the module for its geometry)
    try:
        b = CS._Builder(kind, perm)
    finally:
        CS._params = params
    name, _, num = which.partition("_")
    if name == "chains":
        for _ in range(int(num)):
            CS._chain(b, 17)
        CS._head_on(b, "pair", 0.5)
    elif name == "pairs":
        # one chain among pairs in the cube; FENCE_CHAINS["pore"] chains in the pore, whose bottom cap has fewer than the
        # 2,914 sites that takes: every further chain is worth 32 pairs at the fence
        chains = FENCE_CHAINS[kind]
        for _ in range(chains):
            CS._chain(b, 17)
        fence = label_fence_pairs(16 * chains, 16 * chains)
        for _ in range(fence if num == "under" else fence + 1):
            CS._head_on(b, "pair", 0.5)
    else:
        for _ in range(4):
            CS._chain(b, 17)
        if name == "pull":
            CS._pull_depth(b, 3)
        else:
            CS._conflict_overlay(b)
            CS._conflict_grid(b)
    s = b.finish()
    s.extra["which"] = which
    return s


def grid_structure(s):
    """cluster_states.structure() without its n x n x 3 array: the same pairs and components for states of thousands"""
    P = CS.drifted(s)
    cr = s.p.collision_range
    pairs = close_pairs(P, cr * cr)
    S = _Sets(s.n)
    for a, b in pairs:
        S.union(a, b)
    comps = {}
    for a, b in pairs:
        e = comps.setdefault(S.find(a), dict(particles=set(), candidates=0))
        e["particles"] |= {int(a), int(b)}
        e["candidates"] += 1
    return dict(pairs=pairs, components=[dict(particles=sorted(e["particles"]), candidates=e["candidates"])
                                         for _, e in sorted(comps.items())])
