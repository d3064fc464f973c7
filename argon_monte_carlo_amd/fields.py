"""Sampled fields (include/argonmc.h "sampled fields"): the bin grid, the default grid per geometry and the
derived quantities — number density, flow velocity and temperature per bin — computed on the host from the exact integer
totals the device accumulates.  Nothing here needs a GPU.

Totals come as int64[bins][7][2]: quantities (count, sum q1(c1..c3), sum q2(c1..c3)) with q1(c) = rint(c * 2^24),
q2(c) = rint((c * c) * 2^10), each a signed 128-bit number stored as (low 64 bits, high 64 bits signed)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._abi import (AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN, AMC_FIELDS_MAX_BINS, AMC_GEOM_CUBE,
                   AMC_GEOM_PORE_ENERGISED, AmcFieldGrid)
from . import params as PR
from .totals import ints_to_words, limbs_to_words, words_to_ints, words_to_limbs  # noqa: F401  (the 128-bit totals: totals.py)

Q1_SCALE = 2 ** 24
Q2_SCALE = 2 ** 10
QUANTITIES = ("count", "q1_c1", "q1_c2", "q1_c3", "q2_c1", "q2_c2", "q2_c3")

# default grids: about 8 x 8 x 8 over the cube, 16 radial bins (r up to the open-air radius R_oa) x 128 axial bins
# (z over [0, H]) in the pore
DEFAULT_CUBE_BINS = (8, 8, 8)
DEFAULT_PORE_BINS = (16, 128)


def make_grid(kind, n, lo, hi, every=0, step_offset=0):
    """An ``AmcFieldGrid``, validated like ``amc_fields_config`` (ValueError instead of AMC_ERR_INVALID).
    kind "cartesian": n = (n1, n2, n3), lo / hi = the box corners.  kind "axisymmetric": n = (n_r, n_z),
    lo = (0, z_lo), hi = (r_max, z_hi) (a third entry, if given, must describe n3 = 1)."""
    n, lo, hi = [int(v) for v in n], [float(v) for v in lo], [float(v) for v in hi]
    if kind in ("cartesian", AMC_FIELDS_CARTESIAN):
        k = AMC_FIELDS_CARTESIAN
        if len(n) != 3 or len(lo) != 3 or len(hi) != 3:
            raise ValueError("a Cartesian grid has three axes")
        axes = 3
    elif kind in ("axisymmetric", AMC_FIELDS_AXISYMMETRIC):
        k = AMC_FIELDS_AXISYMMETRIC
        if len(n) == 3:
            if n[2] != 1:
                raise ValueError("an axisymmetric grid has n3 == 1")
            n = n[:2]
        if len(n) != 2 or len(lo) < 2 or len(hi) < 2:
            raise ValueError("an axisymmetric grid has a radial and an axial axis")
        if lo[0] != 0.0:
            raise ValueError("the radial axis of an axisymmetric grid starts at r = 0")
        n, lo, hi = n + [1], lo[:2] + [0.0], hi[:2] + [1.0]
        axes = 2
    else:
        raise ValueError(f"unknown grid kind {kind!r}")
    if min(n) < 1 or n[0] * n[1] * n[2] > AMC_FIELDS_MAX_BINS:
        raise ValueError(f"{n[0]} x {n[1]} x {n[2]} bins: each axis >= 1 and at most {AMC_FIELDS_MAX_BINS} bins in all")
    for a in range(axes):
        if not (math.isfinite(lo[a]) and math.isfinite(hi[a]) and lo[a] < hi[a]):
            raise ValueError(f"axis {a + 1} needs finite bounds lo < hi")
    if int(every) < 0 or int(step_offset) < 0:
        raise ValueError("every and step_offset must be >= 0")
    g = AmcFieldGrid()
    g.struct_size = C.sizeof(AmcFieldGrid)
    g.kind = k
    g.n1, g.n2, g.n3 = n
    g.every, g.step_offset = int(every), int(step_offset)
    for a in range(3):
        g.lo[a], g.hi[a] = lo[a], hi[a]
    return g


def copy_grid(g, every=None, step_offset=None):
    out = type(g).from_buffer_copy(g)         # (an AmcFieldGrid, or the AmcCorrGrid of correlations.py)
    if every is not None:
        out.every = int(every)
    if step_offset is not None:
        out.step_offset = int(step_offset)
    return out


def default_grid(params, every=0):
    """The geometry's natural grid: Cartesian 8 x 8 x 8 over the cube [0, cube_x] x [0, cube_y] x [0, cube_z];
    axisymmetric 16 (r over [0, R_oa]) x 128 (z over [0, H]) in the pore, specular or energised."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", DEFAULT_CUBE_BINS, (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z), every)
    return make_grid("axisymmetric", DEFAULT_PORE_BINS, (0.0, 0.0), (params.R_oa, params.H), every)


def boltzmann_constant(params):
    """The simulation's own k_B: BOLTZMAN_TEMP in the energised pore, BOLTZMAN otherwise (then an initial condition built
    with a_shape = sqrt(k_B T / m) reads back as T)."""
    return PR.BOLTZMAN_TEMP if int(params.geometry) == AMC_GEOM_PORE_ENERGISED else PR.BOLTZMAN


def grid_bins(g):
    return int(g.n1) * int(g.n2) * int(g.n3)


def grid_to_array(g):
    """float64[12] for a checkpoint: kind, n1, n2, n3, every, lo[3], hi[3], step_offset."""
    return np.array([g.kind, g.n1, g.n2, g.n3, g.every] + list(g.lo) + list(g.hi) + [g.step_offset], dtype=np.float64)


def grid_from_array(a):
    a = np.asarray(a, dtype=np.float64)
    kind = int(a[0])
    n = [int(a[1]), int(a[2]), int(a[3])]
    lo, hi = list(a[5:8]), list(a[8:11])
    if kind == AMC_FIELDS_AXISYMMETRIC:
        return make_grid(kind, n[:2], lo[:2], hi[:2], int(a[4]), int(a[11]))
    return make_grid(kind, n, lo, hi, int(a[4]), int(a[11]))


def widths(g):
    """Bin widths (hi - lo) / n per axis, in fp64 as NumPy forms them (radial, axial for an axisymmetric grid)."""
    n = (g.n1, g.n2, g.n3)
    axes = 3 if g.kind == AMC_FIELDS_CARTESIAN else 2
    return [(g.hi[a] - g.lo[a]) / n[a] for a in range(axes)]


def edges(g):
    """Bin edges per axis, np.linspace(lo, hi, n + 1) (r and z for an axisymmetric grid)."""
    n = (g.n1, g.n2, g.n3)
    axes = 3 if g.kind == AMC_FIELDS_CARTESIAN else 2
    return [np.linspace(g.lo[a], g.hi[a], n[a] + 1) for a in range(axes)]


def bin_volumes(g):
    """float64[bins]: w1 w2 w3 (Cartesian), pi (r_{i+1}^2 - r_i^2) w_z (axisymmetric), in linear bin order."""
    w = widths(g)
    if g.kind == AMC_FIELDS_CARTESIAN:
        return np.full(grid_bins(g), w[0] * w[1] * w[2])
    r = edges(g)[0]
    ring = np.array([math.pi * (r[i + 1] * r[i + 1] - r[i] * r[i]) * w[1] for i in range(g.n1)])
    return np.repeat(ring, g.n2)


# ---- derived fields --------------------------------------------------------------------------------------------------
def derive(g, words, n_samples, n_outside, mass, k_b):
    """Number density, mean velocity and temperature per bin from the integer totals (exact integers until the one
    correctly rounded int / int division per quantity)."""
    bins = grid_bins(g)
    tot = words_to_ints(np.asarray(words).reshape(bins, 7, 2))
    vol = bin_volumes(g)
    count = np.array([int(v) for v in tot[:, 0]], dtype=np.int64)
    dens = np.zeros(bins)
    vel = np.full((bins, 3), np.nan)
    temp = np.full((bins, 3), np.nan)
    for b in range(bins):
        cnt = int(tot[b, 0])
        if n_samples > 0:
            dens[b] = cnt / (n_samples * vol[b])
        if cnt < 1:
            continue
        for k in range(3):
            u = int(tot[b, 1 + k]) / (Q1_SCALE * cnt)
            vel[b, k] = u
            if cnt >= 2:
                msq = int(tot[b, 4 + k]) / (Q2_SCALE * cnt)
                temp[b, k] = mass / k_b * (msq - u * u)
    with np.errstate(invalid="ignore"):
        T = (temp[:, 0] + temp[:, 1] + temp[:, 2]) / 3
    return {"count": count, "number_density": dens, "velocity": vel, "temperature": temp, "T": T, "edges": edges(g),
            "bin_volume": vol, "n_samples": int(n_samples), "n_outside": int(n_outside),
            "totals": np.asarray(words, dtype=np.int64).reshape(bins, 7, 2), "kind": int(g.kind),
            "shape": (int(g.n1), int(g.n2), int(g.n3))}
