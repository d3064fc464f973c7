"""Sampled correlations (include/argonmc.h "sampled correlations"): the group grid, the default grid per
geometry and the derived quantities — mean-square displacement, velocity autocorrelation function and the two
self-diffusion estimates per group — computed on the host from the exact integer totals the device accumulates.  Nothing
here needs a GPU.

Totals come as int64[groups][n_lags + 1][7][2]: quantities (count, m_x m_y m_z, c_x c_y c_z) with
m_k = rint(ldexp(D_k * D_k, 74)) for the displacement D_k from the time origin and c_k = rint((v_k * v0_k) * 2^10), each a
signed 128-bit number stored as (low 64 bits, high 64 bits signed)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import AMC_CORR_MAX_CELLS, AMC_CORR_MAX_GROUPS, AMC_GEOM_CUBE, AmcCorrGrid
from ._abi import AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN     # the grid kinds, for callers that build an AmcCorrGrid
from . import fields as FL
from .fields import edges, widths  # noqa: F401  (shared helpers)
from .totals import ints_to_words, limbs_to_words, words_to_ints, words_to_limbs  # noqa: F401

M_SCALE = 2 ** 74
C_SCALE = 2 ** 10
QUANTITIES = ("count", "m_x", "m_y", "m_z", "c_x", "c_y", "c_z")
COUNTERS = ("n_origins", "n_samples", "n_outside", "window_pos")

# default grids: one group over the cube; 1 radial x 32 axial groups (r up to the open-air radius R_oa, z over [0, H]) in the pore
DEFAULT_PORE_GROUPS = (1, 32)
DEFAULT_N_LAGS = 16


def make_grid(kind, n, lo, hi, every=0, step_offset=0, n_lags=DEFAULT_N_LAGS):
    """An ``AmcCorrGrid``, validated like ``amc_corr_config`` (ValueError instead of AMC_ERR_INVALID).  The group grid
    follows ``fields.make_grid``; at most 256 groups and groups * (n_lags + 1) <= 65,536."""
    groups = 1
    for v in n:
        groups *= max(int(v), 1)
    if groups > AMC_CORR_MAX_GROUPS:        # (tighter than the fields' limit on bins)
        raise ValueError(f"{groups} groups: at most {AMC_CORR_MAX_GROUPS} in all")
    return _from_field_grid(FL.make_grid(kind, n, lo, hi, every, step_offset), n_lags)


def _from_field_grid(f, n_lags):
    """the ``AmcFieldGrid`` f as the group grid of an ``AmcCorrGrid`` with ``n_lags`` lags"""
    g = AmcCorrGrid()
    g.struct_size = C.sizeof(AmcCorrGrid)
    g.kind, g.n1, g.n2, g.n3 = f.kind, f.n1, f.n2, f.n3
    g.every, g.step_offset = f.every, f.step_offset
    for a in range(3):
        g.lo[a], g.hi[a] = f.lo[a], f.hi[a]
    return copy_grid(g, n_lags=n_lags)


def copy_grid(g, every=None, step_offset=None, n_lags=None):
    if every is not None and int(every) < 0:
        raise ValueError("every must be >= 0")
    out = FL.copy_grid(g, every, step_offset)
    if n_lags is not None:
        n_lags = int(n_lags)
        if n_lags < 1 or grid_groups(g) * (n_lags + 1) > AMC_CORR_MAX_CELLS:
            raise ValueError(f"n_lags {n_lags}: at least 1 and groups * (n_lags + 1) at most {AMC_CORR_MAX_CELLS}")
        out.n_lags = n_lags
    return out


def default_grid(params, every=0, n_lags=DEFAULT_N_LAGS):
    """The geometry's natural groups: one group over the cube [0, cube_x] x [0, cube_y] x [0, cube_z]; axisymmetric 1 (r over
    [0, R_oa]) x 32 (z over [0, H]) along the pore, specular or energised."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", (1, 1, 1), (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z), every, 0, n_lags)
    return make_grid("axisymmetric", DEFAULT_PORE_GROUPS, (0.0, 0.0), (params.R_oa, params.H), every, 0, n_lags)


def grid_groups(g):
    return int(g.n1) * int(g.n2) * int(g.n3)


def totals_shape(g):
    return (grid_groups(g), int(g.n_lags) + 1, 7, 2)


def grid_to_array(g):
    """float64[13] for a checkpoint: kind, n1, n2, n3, every, lo[3], hi[3], step_offset, n_lags."""
    return np.append(FL.grid_to_array(g), float(g.n_lags))


def grid_from_array(a):
    a = np.asarray(a, dtype=np.float64)
    f = FL.grid_from_array(a[:12])
    if FL.grid_bins(f) > AMC_CORR_MAX_GROUPS:
        raise ValueError(f"{FL.grid_bins(f)} groups: at most {AMC_CORR_MAX_GROUPS} in all")
    return _from_field_grid(f, int(a[12]))


# ---- derived quantities -----------------------------------------------------------------------------------------------
def derive(g, words, counters, dt, every):
    """MSD, VACF and the diffusion estimates per (group, lag, component) from the integer totals (exact integers until the one
    correctly rounded int / int division per value).  ``counters``: (n_origins, n_samples, n_outside[, window_pos]); ``dt`` the
    time step and ``every`` the steps between two samples.  Every (group, lag) is divided by its OWN count: the counts of the
    later lags are smaller while the last window is incomplete.
      msd[g, l, k]   = sum m_k / (2^74 count)      m^2          vacf[g, l, k] = sum c_k / (2^10 count)     m^2/s^2
      lag_time[l]    = l every dt
      D_msd[g, l, k] = msd / (2 lag_time), l >= 1 (NaN at lag 0)
      D_vacf[g, k]   = every dt * trapezoid sum of vacf over the lags that have a count (NaN without lag 0 and 1)"""
    groups, lags1 = grid_groups(g), int(g.n_lags) + 1
    w = np.asarray(words, dtype=np.int64).reshape(groups, lags1, 7, 2)
    tot = words_to_ints(w)
    step = float(every) * float(dt)
    lag_time = np.array([l * step for l in range(lags1)])
    count = np.array([[int(tot[b, l, 0]) for l in range(lags1)] for b in range(groups)], dtype=np.int64)
    msd = np.full((groups, lags1, 3), np.nan)
    vacf = np.full((groups, lags1, 3), np.nan)
    d_msd = np.full((groups, lags1, 3), np.nan)
    d_vacf = np.full((groups, 3), np.nan)
    for b in range(groups):
        for l in range(lags1):
            cnt = int(tot[b, l, 0])
            if cnt < 1:
                continue
            for k in range(3):
                msd[b, l, k] = int(tot[b, l, 1 + k]) / (M_SCALE * cnt)
                vacf[b, l, k] = int(tot[b, l, 4 + k]) / (C_SCALE * cnt)
                if l >= 1 and lag_time[l] > 0:
                    d_msd[b, l, k] = msd[b, l, k] / (2 * lag_time[l])
        have = 0
        while have < lags1 and count[b, have] > 0:
            have += 1
        if have >= 2:
            for k in range(3):
                s = 0.0
                for l in range(have - 1):
                    s += (vacf[b, l, k] + vacf[b, l + 1, k]) / 2
                d_vacf[b, k] = s * step
    counters = [int(v) for v in counters]
    return {"count": count, "msd": msd, "vacf": vacf, "lag_time": lag_time, "D_msd": d_msd, "D_vacf": d_vacf,
            "n_origins": counters[0], "n_samples": counters[1], "n_outside": counters[2],
            "window_pos": counters[3] if len(counters) > 3 else 0, "edges": edges(g), "totals": w, "kind": int(g.kind),
            "shape": (int(g.n1), int(g.n2), int(g.n3)), "n_lags": int(g.n_lags)}
