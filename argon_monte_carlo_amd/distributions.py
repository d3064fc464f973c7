"""Sampled velocity distributions (include/argonmc_vdf.h): the region grid, the default grid per geometry, the
bin-integrated Maxwell distribution to compare with and the derived quantities — probability densities of the three velocity
components and of the speed per region — computed on the host from the exact integer counts the device accumulates.  Nothing
here needs a GPU.

Totals come as int64[regions][C], C = 4 * H + 8 with H = hist_bins, plain counts in this order:
count | c1: under, h[0..H), over | c2: under, h[0..H), over | c3: under, h[0..H), over | speed: h[0..H), over.
The components' histograms cover [-v_max, v_max], the speed's [0, v_max]; components x, y, z on a Cartesian grid, r, theta, z
on an axisymmetric one."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._abi import AMC_GEOM_CUBE, AMC_VDF_MAX_COLUMNS, AMC_VDF_MAX_HIST_BINS, AmcVdfGrid
from ._abi import AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN     # noqa: F401  (the grid kinds, for callers that build a grid)
from . import fields as FL
from .fields import boltzmann_constant, copy_grid, edges, grid_bins, widths  # noqa: F401  (shared helpers: the grids have the fields' axes)

V_RANGE = 16384.0           # the samplers' range: every component of a binned particle is below it in magnitude; v_max at most

# default grids: 2 x 2 x 2 regions over the cube, 1 radial (r up to the open-air radius R_oa) x 32 axial (z over [0, H]) in the
# pore; 64 bins over [-2048, 2048] m/s (64 m/s each) and over [0, 2048] m/s (32 m/s each): every edge is exact in fp64
DEFAULT_CUBE_REGIONS = (2, 2, 2)
DEFAULT_PORE_REGIONS = (1, 32)
DEFAULT_HIST_BINS = 64
DEFAULT_V_MAX = 2048.0


def columns(hist_bins):
    """counters per region: count, three times (under, hist_bins, over), the speed's (hist_bins, over)"""
    return 4 * int(hist_bins) + 8


def make_grid(kind, n, lo, hi, hist_bins=DEFAULT_HIST_BINS, v_max=DEFAULT_V_MAX, every=0, step_offset=0):
    """An ``AmcVdfGrid``, validated like ``amc_vdf_config`` (ValueError instead of AMC_ERR_INVALID): the axes and rules of
    ``fields.make_grid``, 1 .. 256 histogram bins, 0 < v_max <= 16384 m/s and at most 24,576 columns in all."""
    f = FL.make_grid(kind, n, lo, hi, every, step_offset)
    hist_bins = int(hist_bins)
    if not 1 <= hist_bins <= AMC_VDF_MAX_HIST_BINS:
        raise ValueError(f"{hist_bins} histogram bins: 1 .. {AMC_VDF_MAX_HIST_BINS}")
    v_max = float(v_max)
    if not (math.isfinite(v_max) and 0.0 < v_max <= V_RANGE):
        raise ValueError("v_max must be finite, > 0 and at most 16384 m/s")
    if grid_bins(f) * columns(hist_bins) > AMC_VDF_MAX_COLUMNS:
        raise ValueError(f"{grid_bins(f)} regions x (4 x {hist_bins} + 8) columns: at most {AMC_VDF_MAX_COLUMNS} in all")
    g = AmcVdfGrid()
    g.struct_size = C.sizeof(AmcVdfGrid)
    g.kind, g.n1, g.n2, g.n3 = f.kind, f.n1, f.n2, f.n3
    g.hist_bins, g.v_max = hist_bins, v_max
    g.every, g.step_offset = f.every, f.step_offset
    for a in range(3):
        g.lo[a], g.hi[a] = f.lo[a], f.hi[a]
    return g


def default_grid(params, every=0):
    """The geometry's natural grid: Cartesian 2 x 2 x 2 over the cube [0, cube_x] x [0, cube_y] x [0, cube_z]; axisymmetric
    1 (r over [0, R_oa]) x 32 (z over [0, H]) in the pore, specular or energised; 64 bins up to 2048 m/s."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", DEFAULT_CUBE_REGIONS, (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z), every=every)
    return make_grid("axisymmetric", DEFAULT_PORE_REGIONS, (0.0, 0.0), (params.R_oa, params.H), every=every)


def totals_shape(g):
    return (grid_bins(g), columns(g.hist_bins))


def grid_to_array(g):
    """float64[14] for a checkpoint: kind, n1, n2, n3, every, lo[3], hi[3], step_offset (the fields' layout), hist_bins, v_max."""
    return np.concatenate([FL.grid_to_array(g), [g.hist_bins, g.v_max]])


def grid_from_array(a):
    """the inverse of ``grid_to_array``"""
    a = np.asarray(a, dtype=np.float64)
    f = FL.grid_from_array(a[:12])
    axes = 3 if f.kind == AMC_FIELDS_CARTESIAN else 2
    return make_grid(f.kind, (f.n1, f.n2, f.n3)[:axes], list(f.lo)[:axes], list(f.hi)[:axes], int(a[12]), float(a[13]), f.every, f.step_offset)


def edges_v(g):
    """the components' bin edges, np.linspace(-v_max, v_max, hist_bins + 1)"""
    return np.linspace(-g.v_max, g.v_max, int(g.hist_bins) + 1)


def edges_speed(g):
    """the speed's bin edges, np.linspace(0, v_max, hist_bins + 1)"""
    return np.linspace(0.0, g.v_max, int(g.hist_bins) + 1)


def split(g, totals):
    """the columns of int64[regions, C] totals by name: count [regions], under, over [regions, 3], hist [regions, 3, H],
    hist_speed [regions, H], over_speed [regions] (views)"""
    H = int(g.hist_bins)
    t = np.asarray(totals, dtype=np.int64).reshape(grid_bins(g), columns(H))
    comp = t[:, 1:1 + 3 * (H + 2)].reshape(-1, 3, H + 2)
    sp = t[:, 1 + 3 * (H + 2):]
    return {"count": t[:, 0], "under": comp[:, :, 0], "hist": comp[:, :, 1:H + 1], "over": comp[:, :, H + 1],
            "hist_speed": sp[:, :H], "over_speed": sp[:, H]}


# ---- the Maxwell distribution, integrated over the bins ------------------------------------------------------------------------
def _speed_cdf(s, a):
    """P(speed <= s) of a Maxwell distribution with component deviation a"""
    if s <= 0.0:
        return 0.0
    t = s / a
    return math.erf(t / math.sqrt(2.0)) - math.sqrt(2.0 / math.pi) * t * math.exp(-0.5 * t * t)


def maxwell_expected(g, T, mass, k_b, u=(0.0, 0.0, 0.0)):
    """The probabilities a gas in equilibrium at temperature ``T`` (atoms of ``mass``, flow velocity ``u``) puts into the
    columns of one region, integrated over each bin through ``math.erf``, tails included: float64[4, H + 2], rows c1, c2, c3
    and the speed, columns (under, h[0..H), over).  Every row sums to 1; the speed's ``under`` is 0.  The speed's row is the
    Maxwell speed distribution of a gas at rest: with u != 0 it is NaN (the components' rows are shifted by u)."""
    H = int(g.hist_bins)
    a = math.sqrt(k_b * T / mass)
    out = np.zeros((4, H + 2))
    ev = [float(v) for v in edges_v(g)]
    for k in range(3):
        cdf = [0.5 * (1.0 + math.erf((e - u[k]) / (a * math.sqrt(2.0)))) for e in ev]
        out[k, 0] = cdf[0]
        # (the upper tail through erfc's symmetry: 1 - cdf loses it to rounding)
        out[k, H + 1] = 0.5 * (1.0 + math.erf((u[k] - ev[-1]) / (a * math.sqrt(2.0))))
        for j in range(H):
            out[k, 1 + j] = cdf[j + 1] - cdf[j]
    if any(float(v) != 0.0 for v in u):
        out[3, 1:] = np.nan
        return out
    es = [float(v) for v in edges_speed(g)]
    cdf = [_speed_cdf(e, a) for e in es]
    for j in range(H):
        out[3, 1 + j] = cdf[j + 1] - cdf[j]
    out[3, H + 1] = 1.0 - cdf[-1]
    return out


# ---- derived quantities -----------------------------------------------------------------------------------------------------------
def derive(g, totals, n_samples, n_outside, mass, k_b):
    """Densities per region from the integer counts.  With n the region's count:
      pdf[r, k, j]      = h_k[j] / (n * 2 v_max / H)    per m/s; integrates to 1 - (under + over) / n over [-v_max, v_max]
      pdf_speed[r, j]   = h_s[j] / (n * v_max / H)      per m/s; integrates to 1 - over_speed / n over [0, v_max]
    (NaN in an empty region) and, as HISTOGRAM ESTIMATES that put every count at its bin's midpoint m_j — NaN where the region
    is empty or the component's (the speed's) tail counts are not zero, and biased by the binning: the variance by about
    w^2 / 12 for bins of width w —
      mean[r, k]        = sum_j h_k[j] m_j / n
      variance[r, k]    = sum_j h_k[j] m_j^2 / n - mean^2
      T_est[r]          = mass / k_b * (variance[r, 0] + variance[r, 1] + variance[r, 2]) / 3
      mean_speed[r]     = sum_j h_s[j] m_j / n."""
    H = int(g.hist_bins)
    regions = grid_bins(g)
    t = np.asarray(totals, dtype=np.int64).reshape(regions, columns(H))
    s = split(g, t)
    count = s["count"].copy()
    ev, es = edges_v(g), edges_speed(g)
    wv, ws = 2.0 * g.v_max / H, g.v_max / H
    mv, ms = 0.5 * (ev[:-1] + ev[1:]), 0.5 * (es[:-1] + es[1:])
    pdf = np.full((regions, 3, H), np.nan)
    pdf_speed = np.full((regions, H), np.nan)
    mean = np.full((regions, 3), np.nan)
    var = np.full((regions, 3), np.nan)
    mean_speed = np.full(regions, np.nan)
    for r in range(regions):
        n = int(count[r])
        if n < 1:
            continue
        pdf[r] = s["hist"][r] / (n * wv)
        pdf_speed[r] = s["hist_speed"][r] / (n * ws)
        for k in range(3):
            if s["under"][r, k] == 0 and s["over"][r, k] == 0:
                h = s["hist"][r, k].astype(np.float64)
                mean[r, k] = float((h * mv).sum()) / n
                var[r, k] = float((h * mv * mv).sum()) / n - mean[r, k] * mean[r, k]
        if s["over_speed"][r] == 0:
            mean_speed[r] = float((s["hist_speed"][r] * ms).sum()) / n
    T_est = mass / k_b * (var[:, 0] + var[:, 1] + var[:, 2]) / 3
    return {"count": count, "pdf": pdf, "pdf_speed": pdf_speed, "under": s["under"].copy(), "over": s["over"].copy(),
            "over_speed": s["over_speed"].copy(), "edges_v": ev, "edges_speed": es, "mean": mean, "variance": var, "T_est": T_est,
            "mean_speed": mean_speed, "n_samples": int(n_samples), "n_outside": int(n_outside), "totals": t, "edges": edges(g),
            "kind": int(g.kind), "shape": (int(g.n1), int(g.n2), int(g.n3))}
