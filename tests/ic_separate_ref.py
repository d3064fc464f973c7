"""Host mirror of the overlap removal of a synthetic start (include/argonmc-ic.h): the rule as the header states it — the loser
search as a NumPy cell hash with brute force over the 27 cells around each occupied cell, the redraw from the plain-Python
Philox4x32-10 of tests/philox_ref.py, and the loop.  Test infrastructure: nothing here knows the library's cell grid, launch
geometry or order of anything; the hash's own cells only need an edge of at least min_dist."""
import math

import numpy as np

from tests.philox_ref import MASK, philox4x32_10

IC_TAG = 0x414d4349          # "AMCI"
STATS = ("searches", "rounds", "redrawn", "pairs_first", "losers_first", "pairs_left", "losers_left", "next_round")
TWO_PI = 6.283185307179586


def uniforms(seed, particle, rnd):
    """u0, u1, u2 of particle `particle` in round `rnd`: Philox blocks 0 and 1 with counter (particle, block, rnd, "AMCI")"""
    out = []
    for blk in range(2):
        c = philox4x32_10([particle, blk, rnd, IC_TAG], [seed & MASK, (seed >> 32) & MASK])
        out.append((((c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0))
        out.append((((c[2] << 32) | c[3]) >> 11) * (1.0 / 9007199254740992.0))
    return out[:3]


def regions_of(cfg):
    """[(first, end, radius, z_lo, z_hi)] of an AmcIcConfig; empty: the cube"""
    return [(int(cfg.first[r]), int(cfg.first[r + 1]), float(cfg.radius[r]), float(cfg.z_lo[r]), float(cfg.z_hi[r]))
            for r in range(int(cfg.n_regions))]


def region_index(cfg, p):
    r = 0
    while r + 1 < int(cfg.n_regions) and p >= int(cfg.first[r + 1]):
        r += 1
    return r


def position(cfg, cube, p, rnd):
    """the position of particle p in round rnd (0: amc_init_synthetic's), in the device's order of operations; cube: (X, Y, Z).
    In the cube every operation is one IEEE product: bit for bit the device's.  In a cylinder cos, sin and sqrt come from libm."""
    u0, u1, u2 = uniforms(int(cfg.seed), p, rnd)
    if int(cfg.n_regions) == 0:
        return u0 * cube[0], u1 * cube[1], u2 * cube[2]
    r = region_index(cfg, p)
    th, rad = TWO_PI * u0, float(cfg.radius[r]) * math.sqrt(u1)
    zl, zh = float(cfg.z_lo[r]), float(cfg.z_hi[r])
    return rad * math.cos(th), rad * math.sin(th), zl + (zh - zl) * u2


def initial_positions(cfg, cube, n):
    """x, y, z of amc_init_synthetic (round 0)"""
    xyz = np.array([position(cfg, cube, p, 0) for p in range(n)], dtype=np.float64).reshape(n, 3)
    return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()


def search(x, y, z, min_dist, max_cells_axis=16):
    """(pairs, losers): the number of pairs (i, j), i < j, with dx*dx + dy*dy + dz*dz < min_dist*min_dist, and the sorted indices
    j that have such a partner.  Cell hash over the state's own bounding box; every unordered pair is met once, from the cell of
    its lower index."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    n = len(x)
    if n < 2:
        return 0, np.zeros(0, dtype=np.int64)
    md2 = np.float64(min_dist) * np.float64(min_dist)
    edge = float(min_dist) * (1.0 + 2.0 ** -20)
    cell = []
    for u in (x, y, z):
        lo, ext = float(u.min()), float(u.max() - u.min())
        m = int(min(max(math.floor(ext / edge), 1), max_cells_axis)) if ext > 0.0 else 1
        w = ext / m if ext > 0.0 else 1.0
        cell.append(np.clip(np.floor((u - lo) / w).astype(np.int64), 0, m - 1))
    # two atoms closer than min_dist on an axis are at most one cell apart: w >= edge > min_dist, and the clip is monotone
    key = (cell[0] * (max_cells_axis + 2) + cell[1]) * (max_cells_axis + 2) + cell[2]
    order = np.argsort(key, kind="stable")
    keys, start = np.unique(key[order], return_index=True)
    end = np.append(start[1:], n)
    members = {int(k): order[a:b] for k, a, b in zip(keys, start, end)}
    s = max_cells_axis + 2
    lose = np.zeros(n, dtype=bool)
    pairs = 0
    for k, home in members.items():
        cx, cy, cz = k // (s * s), (k // s) % s, k % s
        near = [members[(X * s + Y) * s + Z] for X in (cx - 1, cx, cx + 1) for Y in (cy - 1, cy, cy + 1) for Z in (cz - 1, cz, cz + 1)
                if X >= 0 and Y >= 0 and Z >= 0 and (X * s + Y) * s + Z in members]
        nb = np.concatenate(near)
        for a in range(0, len(home), 512):          # (bounded temporaries: the all-at-one-point state is 4,096 x 4,096)
            i = home[a:a + 512]
            dx = x[i][:, None] - x[nb][None, :]
            dy = y[i][:, None] - y[nb][None, :]
            dz = z[i][:, None] - z[nb][None, :]
            hit = ((dx * dx + dy * dy) + dz * dz < md2) & (i[:, None] < nb[None, :])
            pairs += int(hit.sum())
            lose[nb[hit.any(axis=0)]] = True
    return pairs, np.flatnonzero(lose)


def brute_search(x, y, z, min_dist):
    """the same by brute force over all pairs (small n): what pins `search`"""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    n = len(x)
    md2 = np.float64(min_dist) * np.float64(min_dist)
    dx, dy, dz = x[:, None] - x[None, :], y[:, None] - y[None, :], z[:, None] - z[None, :]
    hit = ((dx * dx + dy * dy) + dz * dz < md2) & (np.arange(n)[:, None] < np.arange(n)[None, :])
    return int(hit.sum()), np.flatnonzero(hit.any(axis=0))


def separate(x, y, z, cfg, cube, min_dist, first_round=1, max_rounds=64):
    """The loop of amc_init_separate on copies of x, y, z.  Returns (x, y, z, stats dict)."""
    x, y, z = (np.array(a, dtype=np.float64) for a in (x, y, z))
    t, rounds, redrawn, searches = int(first_round), 0, 0, 0
    first = None
    while True:
        pairs, losers = search(x, y, z, min_dist)
        searches += 1
        if first is None:
            first = (pairs, len(losers))
        if pairs == 0 or rounds == max_rounds:
            break
        for j in losers:
            x[j], y[j], z[j] = position(cfg, cube, int(j), t)
        redrawn += len(losers)
        t += 1
        rounds += 1
    st = dict(zip(STATS, (searches, rounds, redrawn, first[0], first[1], pairs, len(losers), t)))
    return x, y, z, st
