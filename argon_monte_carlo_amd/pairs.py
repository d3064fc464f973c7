"""Sampled pair distribution (include/argonmc_pair.h): the region grid, the default grid per geometry and the
derived quantities — g(r), the coordination number, the pairs left closer than the collision range and the share of pairs still
approaching — computed on the host from the exact integer counts the device accumulates.  Nothing here needs a GPU.

Totals come as int64[regions][C], C = 1 + 2 * H with H = hist_bins, plain counts in this order:
centres | pairs[0..H) | approaching[0..H).
A centre is a particle of the region; its neighbours are all other particles of the system, wherever they are; column k holds
the ordered pairs with floor(r / (r_max / H)) == k.  A pair whose ends both are centres is therefore counted twice, once from
either end (in the region of that end)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._abi import AMC_GEOM_CUBE, AMC_PAIR_MAX_CELLS_AXIS, AMC_PAIR_MAX_COLUMNS, AMC_PAIR_MAX_HIST_BINS, AmcPairGrid
from ._abi import AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN     # noqa: F401  (the grid kinds, for callers that build a grid)
from . import fields as FL
from .fields import bin_volumes, copy_grid, edges, grid_bins, widths  # noqa: F401  (shared helpers: the grids have the fields' axes)

# default grids: one region over the cube, 1 radial (r up to the open-air radius R_oa) x 16 axial (z over [0, H]) in the pore;
# 64 columns up to r_max = 32 collision ranges d: the column width d / 2 is a power-of-two scaling of r_max, so d is exactly the
# edge between columns 1 and 2
DEFAULT_CUBE_REGIONS = (1, 1, 1)
DEFAULT_PORE_REGIONS = (1, 16)
DEFAULT_HIST_BINS = 64
DEFAULT_R_MAX_RANGES = 32.0


def columns(hist_bins):
    """counters per region: centres, pairs per column, approaching pairs per column"""
    return 1 + 2 * int(hist_bins)


def make_grid(kind, n, lo, hi, r_max, hist_bins=DEFAULT_HIST_BINS, every=0, step_offset=0):
    """An ``AmcPairGrid``, validated like ``amc_pair_config`` (ValueError instead of AMC_ERR_INVALID): the axes and rules of
    ``fields.make_grid``, 1 .. 256 columns, r_max finite and > 0 and at most 6,144 columns in all."""
    f = FL.make_grid(kind, n, lo, hi, every, step_offset)
    hist_bins = int(hist_bins)
    if not 1 <= hist_bins <= AMC_PAIR_MAX_HIST_BINS:
        raise ValueError(f"{hist_bins} histogram bins: 1 .. {AMC_PAIR_MAX_HIST_BINS}")
    r_max = float(r_max)
    if not (math.isfinite(r_max) and r_max > 0.0):
        raise ValueError("r_max must be finite and > 0")
    if grid_bins(f) * columns(hist_bins) > AMC_PAIR_MAX_COLUMNS:
        raise ValueError(f"{grid_bins(f)} regions x (1 + 2 x {hist_bins}) columns: at most {AMC_PAIR_MAX_COLUMNS} in all")
    g = AmcPairGrid()
    g.struct_size = C.sizeof(AmcPairGrid)
    g.kind, g.n1, g.n2, g.n3 = f.kind, f.n1, f.n2, f.n3
    g.hist_bins, g.r_max = hist_bins, r_max
    g.every, g.step_offset = f.every, f.step_offset
    for a in range(3):
        g.lo[a], g.hi[a] = f.lo[a], f.hi[a]
    return g


def default_grid(params, every=0):
    """The geometry's natural grid: one Cartesian region over the cube [0, cube_x] x [0, cube_y] x [0, cube_z]; axisymmetric
    1 (r over [0, R_oa]) x 16 (z over [0, H]) in the pore, specular or energised; 64 columns up to 32 collision ranges."""
    r_max = DEFAULT_R_MAX_RANGES * float(params.collision_range)
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", DEFAULT_CUBE_REGIONS, (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z), r_max, every=every)
    return make_grid("axisymmetric", DEFAULT_PORE_REGIONS, (0.0, 0.0), (params.R_oa, params.H), r_max, every=every)


def totals_shape(g):
    return (grid_bins(g), columns(g.hist_bins))


def grid_to_array(g):
    """float64[14] for a checkpoint: kind, n1, n2, n3, every, lo[3], hi[3], step_offset (the fields' layout), hist_bins, r_max."""
    return np.concatenate([FL.grid_to_array(g), [g.hist_bins, g.r_max]])


def grid_from_array(a):
    """the inverse of ``grid_to_array``"""
    a = np.asarray(a, dtype=np.float64)
    f = FL.grid_from_array(a[:12])
    axes = 3 if f.kind == AMC_FIELDS_CARTESIAN else 2
    return make_grid(f.kind, (f.n1, f.n2, f.n3)[:axes], list(f.lo)[:axes], list(f.hi)[:axes], float(a[13]), int(a[12]), f.every, f.step_offset)


def search_box(g):
    """The sampler's search cells: (lo[3], hi[3], cells[3], edge[3]) — the grid's bounding box ([-hi_r, hi_r]^2 x [lo_z, hi_z]
    on an axisymmetric grid) grown by r_max, min(floor(extent / (r_max * (1 + 2^-20))), 128) cells per axis, at least 1; fp64 as
    ``amc_pair_config`` forms them."""
    r_max = float(g.r_max)
    if g.kind == AMC_FIELDS_CARTESIAN:
        lo = [float(g.lo[k]) - r_max for k in range(3)]
        hi = [float(g.hi[k]) + r_max for k in range(3)]
    else:
        lo = [-float(g.hi[0]) - r_max, -float(g.hi[0]) - r_max, float(g.lo[1]) - r_max]
        hi = [float(g.hi[0]) + r_max, float(g.hi[0]) + r_max, float(g.hi[1]) + r_max]
    edge = r_max * (1.0 + 2.0 ** -20)
    cells = [int(max(1.0, min(math.floor((hi[k] - lo[k]) / edge), float(AMC_PAIR_MAX_CELLS_AXIS)))) for k in range(3)]
    return lo, hi, cells, [(hi[k] - lo[k]) / cells[k] for k in range(3)]


def r_edges(g):
    """the column edges k * (r_max / H), the last one r_max"""
    H = int(g.hist_bins)
    e = np.arange(H + 1, dtype=np.float64) * (float(g.r_max) / H)
    e[H] = float(g.r_max)
    return e


def split(g, totals):
    """the columns of int64[regions, C] totals by name: centres [regions], pairs, approaching [regions, H] (views)"""
    H = int(g.hist_bins)
    t = np.asarray(totals, dtype=np.int64).reshape(grid_bins(g), columns(H))
    return {"centres": t[:, 0], "pairs": t[:, 1:1 + H], "approaching": t[:, 1 + H:]}


def shell_volumes(g):
    """float64[H]: 4 pi / 3 (r_{k+1}^3 - r_k^3), the exact volume of column k's shell"""
    e = r_edges(g)
    return 4.0 * math.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)


def derive(g, totals, n_samples, n_outside, n_unfiled, collision_range):
    """Structure per region from the integer counts.  With c the region's centres over all samples, V its volume and
    rho = c / (n_samples * V) the mean number density of the region:
      g[r, k]                = pairs[r, k] / (c * rho * V_shell[k])       the pair distribution; 1 for an ideal gas far from walls
      g_err[r, k]            = sqrt(pairs[r, k]) / (c * rho * V_shell[k]) its Poisson error (a pair inside one region is counted
                                                                          from both ends: the error is that of the ordered count)
      coordination[r, k]     = sum_{k' <= k} pairs[r, k'] / c             neighbours within the column's upper edge per centre
      overlap_per_centre[r]  = pairs with r < d per centre, d the collision range: what the step leaves unresolved.  Exact
                               only when d is one of the column edges (the columns are not split); otherwise NaN.  The default
                               grid makes d the edge of column 2.
      approach_fraction[r,k] = approaching / pairs, NaN where pairs == 0
    NaN in a region without centres.  There is NO wall correction: the neighbours are the particles that exist, so a centre
    nearer than r to a wall (or to the end of the gas) sees a truncated shell and g dips there by construction; rho is the
    region's own mean density, so a region with a density gradient is normalised by its mean."""
    H = int(g.hist_bins)
    regions = grid_bins(g)
    t = np.asarray(totals, dtype=np.int64).reshape(regions, columns(H))
    s = split(g, t)
    c = s["centres"].astype(np.float64)
    pairs = s["pairs"].astype(np.float64)
    e = r_edges(g)
    vs = shell_volumes(g)
    vol = bin_volumes(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = (c * c / (float(n_samples) * vol))[:, None] * vs[None, :]         # c * rho * V_shell
        gr = np.where(c[:, None] > 0, pairs / norm, np.nan)
        g_err = np.where(c[:, None] > 0, np.sqrt(pairs) / norm, np.nan)
        coordination = np.where(c[:, None] > 0, np.cumsum(s["pairs"], axis=1) / c[:, None], np.nan)
        approach = np.where(s["pairs"] > 0, s["approaching"] / pairs, np.nan)
        at = np.flatnonzero(e == float(collision_range))
        if at.size:
            overlap = np.where(c > 0, s["pairs"][:, :int(at[0])].sum(axis=1) / c, np.nan)
        else:
            overlap = np.full(regions, np.nan)
    return {"r_edges": e, "r_mid": 0.5 * (e[:-1] + e[1:]), "centres": s["centres"].copy(), "pairs": s["pairs"].copy(),
            "approaching": s["approaching"].copy(), "g": gr, "g_err": g_err, "coordination": coordination, "overlap_per_centre": overlap,
            "approach_fraction": approach, "n_samples": int(n_samples), "n_outside": int(n_outside), "n_unfiled": int(n_unfiled), "totals": t,
            "edges": edges(g), "kind": int(g.kind), "shape": (int(g.n1), int(g.n2), int(g.n3))}
