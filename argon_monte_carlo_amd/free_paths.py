"""Sampled free paths (include/argonmc_mfp.h): the bin grid, the default grid per geometry and the derived
quantities — local mean free path, the wall's share of path ends, the rate of path ends per volume and the local histogram —
computed on the host from the exact integer totals the device accumulates.  Nothing here needs a GPU.

Totals come as int64[bins][2][7][2]: per bin and ending kind (0: a wall, 1: another atom) seven quantities (count,
sum q(total), sum q(px), sum q(py), sum q(pz), sum q2(total), reserved) with q(v) = rint(ldexp(v, 56)) and
q2(v) = rint(ldexp(v * v, 72)), each a signed 128-bit number stored as (low 64 bits, high 64 bits signed); the histogram as
int64[bins][2][hist_bins + 1] plain counts of ``total`` over [0, hist_hi), the last column "beyond"."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from ._abi import AMC_GEOM_CUBE, AMC_MFP_MAX_COLUMNS, AMC_MFP_MAX_HIST_BINS, AmcMfpGrid
from ._abi import AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN     # noqa: F401  (the grid kinds, for callers that build a grid)
from . import fields as FL
from .fields import bin_volumes, edges, grid_bins, widths  # noqa: F401  (shared helpers: the grids have the fields' axes)
from .totals import ints_to_words, words_to_ints  # noqa: F401

Q_SCALE = 2 ** 56           # sum q / Q_SCALE:   sum of a length            (m)
Q2_SCALE = 2 ** 72          # sum q2 / Q2_SCALE: sum of total^2             (m^2)
RANGE = 2.0 ** -16          # every length of a binned record lies in [0, RANGE)
QUANTITIES = ("count", "q_total", "q_x", "q_y", "q_z", "q2_total", "reserved")
KINDS = ("wall", "pp", "all")

# default grids: 4 x 4 x 4 over the cube, 4 radial bins (r up to the open-air radius R_oa) x 16 axial bins (z over [0, H]) in
# the pore; 32 histogram columns over [0, 1e-6 m], the range of the reference's own histograms
DEFAULT_CUBE_BINS = (4, 4, 4)
DEFAULT_PORE_BINS = (4, 16)
DEFAULT_HIST_BINS = 32
DEFAULT_HIST_HI = 1e-6


def columns(n_bins, hist_bins):
    """64-bit words of one launch's table: n_bins * 2 * (7 + hist_bins + 1), at most AMC_MFP_MAX_COLUMNS"""
    return int(n_bins) * 2 * (7 + int(hist_bins) + 1)


def make_grid(kind, n, lo, hi, hist_bins=DEFAULT_HIST_BINS, hist_hi=DEFAULT_HIST_HI, keep_records=False):
    """An ``AmcMfpGrid``, validated like ``amc_mfp_config`` (ValueError instead of AMC_ERR_INVALID): the axes and rules of
    ``fields.make_grid``, 0 .. 64 histogram columns over [0, hist_hi) and at most 6,144 table columns in all."""
    f = FL.make_grid(kind, n, lo, hi)
    hist_bins = int(hist_bins)
    if not 0 <= hist_bins <= AMC_MFP_MAX_HIST_BINS:
        raise ValueError(f"{hist_bins} histogram bins: 0 .. {AMC_MFP_MAX_HIST_BINS}")
    hist_hi = float(hist_hi)
    if hist_bins > 0 and not (math.isfinite(hist_hi) and hist_hi > 0.0):
        raise ValueError("hist_hi must be finite and > 0")
    if columns(grid_bins(f), hist_bins) > AMC_MFP_MAX_COLUMNS:
        raise ValueError(f"{grid_bins(f)} bins x 2 x (7 + {hist_bins} + 1) columns: at most {AMC_MFP_MAX_COLUMNS} in all")
    g = AmcMfpGrid()
    g.struct_size = C.sizeof(AmcMfpGrid)
    g.kind, g.n1, g.n2, g.n3 = f.kind, f.n1, f.n2, f.n3
    g.hist_bins, g.keep_records, g.hist_hi = hist_bins, int(bool(keep_records)), hist_hi
    for a in range(3):
        g.lo[a], g.hi[a] = f.lo[a], f.hi[a]
    return g


def copy_grid(g, keep_records=None):
    out = AmcMfpGrid.from_buffer_copy(g)
    if keep_records is not None:
        out.keep_records = int(bool(keep_records))
    return out


def default_grid(params, keep_records=False):
    """The geometry's natural grid: Cartesian 4 x 4 x 4 over the cube [0, cube_x] x [0, cube_y] x [0, cube_z]; axisymmetric
    4 (r over [0, R_oa]) x 16 (z over [0, H]) in the pore, specular or energised; 32 histogram columns over [0, 1e-6 m]."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", DEFAULT_CUBE_BINS, (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z),
                         keep_records=keep_records)
    return make_grid("axisymmetric", DEFAULT_PORE_BINS, (0.0, 0.0), (params.R_oa, params.H), keep_records=keep_records)


def totals_shape(g):
    return (grid_bins(g), 2, 7, 2)


def hist_shape(g):
    return (grid_bins(g), 2, int(g.hist_bins) + 1)


def grid_to_array(g):
    """float64[13] for a checkpoint: kind, n1, n2, n3, hist_bins, keep_records, lo[3], hi[3], hist_hi."""
    return np.array([g.kind, g.n1, g.n2, g.n3, g.hist_bins, g.keep_records] + list(g.lo) + list(g.hi) + [g.hist_hi], dtype=np.float64)


def grid_from_array(a):
    a = np.asarray(a, dtype=np.float64)
    kind = int(a[0])
    n = [int(a[1]), int(a[2]), int(a[3])]
    lo, hi = list(a[6:9]), list(a[9:12])
    if kind == AMC_FIELDS_AXISYMMETRIC:
        n, lo, hi = n[:2], lo[:2], hi[:2]
    return make_grid(kind, n, lo, hi, int(a[4]), float(a[12]), bool(int(a[5])))


def hist_edges(g):
    """np.linspace(0, hist_hi, hist_bins + 1) (empty without a histogram)"""
    return np.linspace(0.0, g.hist_hi, int(g.hist_bins) + 1) if int(g.hist_bins) > 0 else np.zeros(0)


# ---- derived quantities -----------------------------------------------------------------------------------------------
def derive(g, words, hist, n_records, n_outside, n_steps, dt):
    """Per bin and ending kind — the last axis of every per-kind array is (wall, p-p, both together) — from the integer totals.
    With n the count, S1 = sum q(total) / 2^56, S2 = sum q2(total) / 2^72, V the bin's volume:
      count                 n
      mean_free_path        S1 / n                                                                       m
      mean_abs_x / _y / _z  sum q(p_k) / 2^56 / n                                                        m
      var_free_path         S2 / n - (S1 / n)^2                                                          m^2
      wall_fraction         n_wall / n_both                 (per bin)
      end_rate              n / (n_steps dt V)              paths ended per m^3 and s
      hist                  the counts, int64[bins, 3, hist_bins + 1] (the last column: beyond hist_hi)
      hist_density          counts / (in-range counts * column width): np.histogram(density=True) over the in-range columns
    The means, the variance and wall_fraction are formed exactly, as ``Fraction``s of Python ints, and rounded to a float
    once; end_rate and hist_density are float arithmetic in the order written (their inputs dt, V and the column width are
    floats).  A (bin, kind) without paths has NaN means, variance and density (a bin without any, a NaN wall_fraction) and
    end_rate 0; without steps end_rate is NaN."""
    bins, hb = grid_bins(g), int(g.hist_bins)
    w = np.asarray(words, dtype=np.int64).reshape(bins, 2, 7, 2)
    h = np.asarray(hist, dtype=np.int64).reshape(bins, 2, hb + 1)
    t2 = words_to_ints(w)
    tot = np.empty((bins, 3, 7), dtype=object)
    tot[:, :2] = t2
    tot[:, 2] = t2[:, 0] + t2[:, 1]
    h3 = np.concatenate([h, h.sum(axis=1, keepdims=True)], axis=1)
    vol = bin_volumes(g)
    count = np.array([[int(v) for v in row] for row in tot[:, :, 0]], dtype=np.int64).reshape(bins, 3)
    mean = np.full((bins, 3), np.nan)
    mabs = np.full((3, bins, 3), np.nan)
    var = np.full((bins, 3), np.nan)
    wall = np.full(bins, np.nan)
    rate = np.full((bins, 3), np.nan)
    dens = np.full((bins, 3, hb), np.nan)
    width = g.hist_hi / hb if hb > 0 else 0.0
    for b in range(bins):
        if count[b, 2] > 0:
            wall[b] = float(Fraction(int(count[b, 0]), int(count[b, 2])))
        for k in range(3):
            n = int(count[b, k])
            if n_steps > 0:
                rate[b, k] = n / (n_steps * dt * vol[b])
            if n < 1:
                continue
            m = Fraction(int(tot[b, k, 1]), Q_SCALE * n)
            mean[b, k] = float(m)
            for a in range(3):
                mabs[a, b, k] = float(Fraction(int(tot[b, k, 2 + a]), Q_SCALE * n))
            var[b, k] = float(Fraction(int(tot[b, k, 5]), Q2_SCALE * n) - m * m)
            inside = int(h3[b, k, :hb].sum())
            if hb > 0 and inside > 0:
                dens[b, k] = h3[b, k, :hb] / inside / width
    return {"count": count, "mean_free_path": mean, "mean_abs_x": mabs[0], "mean_abs_y": mabs[1], "mean_abs_z": mabs[2],
            "var_free_path": var, "wall_fraction": wall, "end_rate": rate, "hist": h3, "hist_density": dens,
            "hist_edges": hist_edges(g), "edges": edges(g), "bin_volume": vol, "n_records": int(n_records),
            "n_outside": int(n_outside), "n_steps": int(n_steps), "totals": w, "hist_totals": h, "kind": int(g.kind),
            "shape": (int(g.n1), int(g.n2), int(g.n3))}
