"""Sampled fluxes (include/argonmc_flux.h): the bin grid, the default grid per geometry and the derived
quantities — pressure tensor, energy flux and heat flux per bin — computed on the host from the exact integer totals the
device accumulates.  Nothing here needs a GPU.

Totals come as int64[bins][2][7][2]: per bin two rows of seven quantities, each a signed 128-bit number stored as (low 64 bits,
high 64 bits signed).  Row A is the sampled fields' (count, sum q1(c_k), sum q2(c_k c_k)); row B is (0, sum q2(c1 c2),
sum q2(c1 c3), sum q2(c2 c3), sum q3(c_k)) with q1(c) = rint(c * 2^24), q2(a b) = rint((a * b) * 2^10) and
q3(c_k) = rint(ldexp(e * c_k, -6)), e = (c1*c1 + c2*c2) + c3*c3."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

from ._abi import AMC_FLUX_MAX_BINS, AMC_GEOM_CUBE, AmcFluxGrid
from ._abi import AMC_FIELDS_AXISYMMETRIC, AMC_FIELDS_CARTESIAN     # noqa: F401  (the grid kinds, for callers that build a grid)
from . import fields as FL
from .fields import bin_volumes, boltzmann_constant, copy_grid, edges, grid_bins, grid_to_array, widths  # noqa: F401  (shared helpers)
from .totals import ints_to_words, limbs_to_words, words_to_ints, words_to_limbs  # noqa: F401

Q1_SCALE = 2 ** 24          # sum q1 / Q1_SCALE: sum of c_k            (m/s)
Q2_SCALE = 2 ** 10          # sum q2 / Q2_SCALE: sum of c_a c_b        (m^2/s^2)
Q3_UNIT = 2 ** 6            # sum q3 * Q3_UNIT:  sum of |c|^2 c_k      (m^3/s^3)
QUANTITIES = (("count", "q1_c1", "q1_c2", "q1_c3", "q2_c1c1", "q2_c2c2", "q2_c3c3"),
              ("reserved", "q2_c1c2", "q2_c1c3", "q2_c2c3", "q3_c1", "q3_c2", "q3_c3"))

# default grids: 8 x 8 x 8 over the cube, 8 radial bins (r up to the open-air radius R_oa) x 128 axial bins (z over [0, H])
# in the pore
DEFAULT_CUBE_BINS = (8, 8, 8)
DEFAULT_PORE_BINS = (8, 128)


def make_grid(kind, n, lo, hi, every=0, step_offset=0):
    """An ``AmcFluxGrid``, validated like ``amc_flux_config`` (ValueError instead of AMC_ERR_INVALID): the axes and rules of
    ``fields.make_grid``, at most 1024 bins."""
    bins = 1
    for v in n:
        bins *= max(int(v), 1)
    if bins > AMC_FLUX_MAX_BINS:                    # (tighter than the fields' limit: fourteen integers per bin, not seven)
        raise ValueError(f"{bins} bins: at most {AMC_FLUX_MAX_BINS} in all")
    g = AmcFluxGrid.from_buffer_copy(FL.make_grid(kind, n, lo, hi, every, step_offset))      # (the same fields)
    g.struct_size = C.sizeof(AmcFluxGrid)
    return g


def default_grid(params, every=0):
    """The geometry's natural grid: Cartesian 8 x 8 x 8 over the cube [0, cube_x] x [0, cube_y] x [0, cube_z]; axisymmetric
    8 (r over [0, R_oa]) x 128 (z over [0, H]) in the pore, specular or energised."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        return make_grid("cartesian", DEFAULT_CUBE_BINS, (0.0, 0.0, 0.0), (params.cube_x, params.cube_y, params.cube_z), every)
    return make_grid("axisymmetric", DEFAULT_PORE_BINS, (0.0, 0.0), (params.R_oa, params.H), every)


def totals_shape(g):
    return (grid_bins(g), 2, 7, 2)


def grid_from_array(a):
    """the inverse of ``grid_to_array`` (float64[12], the fields' layout)"""
    f = FL.grid_from_array(a)
    return make_grid(f.kind, (f.n1, f.n2, f.n3), list(f.lo), list(f.hi), f.every, f.step_offset)


# ---- derived quantities -----------------------------------------------------------------------------------------------
_OFF = {(0, 1): 1, (0, 2): 2, (1, 2): 3}        # row B's place of the cross product c_a c_b, a < b


def moments(row_a, row_b):
    """One bin's moments as exact ``Fraction``s from its fourteen integer totals (count >= 1): (n, u[3], M[3][3], F[3]) with
    u_a = sum q1_a / 2^24 / n, M_ab = sum q2_ab / 2^10 / n (symmetric) and F_a = sum q3_a * 2^6 / n."""
    n = int(row_a[0])
    u = [Fraction(int(row_a[1 + a]), Q1_SCALE * n) for a in range(3)]
    M = [[None] * 3 for _ in range(3)]
    for a in range(3):
        M[a][a] = Fraction(int(row_a[4 + a]), Q2_SCALE * n)
        for b in range(a + 1, 3):
            M[a][b] = M[b][a] = Fraction(int(row_b[_OFF[(a, b)]]), Q2_SCALE * n)
    F = [Fraction(int(row_b[4 + a]) * Q3_UNIT, n) for a in range(3)]
    return n, u, M, F


def derive(g, words, n_samples, n_outside, mass, k_b):
    """Pressure tensor, energy flux and heat flux per bin from the integer totals.  With n the bin's count, S the samples, V
    the bin's volume and u, M, F of ``moments``:
      number_density        = n / (S V)                                                                   m^-3
      velocity[a]           = u_a                                                                         m/s
      pressure_tensor[a][b] = number_density * mass * (M_ab - u_a u_b)                                    Pa
      pressure              = (P_11 + P_22 + P_33) / 3,   T = pressure / (number_density * k_b)
      energy_flux[a]        = number_density * mass / 2 * F_a                                             W/m^2
      heat_flux[a]          = number_density * mass / 2 * (F_a - u_a sum_b M_bb - 2 sum_b u_b M_ab + 2 u_a sum_b u_b^2)
    The heat flux is a small difference of large terms: every bracket (and u_a, F_a) is formed exactly, as a ``Fraction`` of
    Python ints, and rounded to a float once; the factors in front are then applied in the order written.  Velocity, pressure
    tensor, pressure, T and the fluxes are NaN in a bin with fewer than two particles; number_density is 0 without samples."""
    bins = grid_bins(g)
    w = np.asarray(words, dtype=np.int64).reshape(bins, 2, 7, 2)
    tot = words_to_ints(w)
    vol = bin_volumes(g)
    count = np.array([int(v) for v in tot[:, 0, 0]], dtype=np.int64)
    dens = np.zeros(bins)
    vel = np.full((bins, 3), np.nan)
    P = np.full((bins, 3, 3), np.nan)
    p = np.full(bins, np.nan)
    T = np.full(bins, np.nan)
    eflux = np.full((bins, 3), np.nan)
    q = np.full((bins, 3), np.nan)
    for b in range(bins):
        if n_samples > 0:
            dens[b] = int(count[b]) / (n_samples * vol[b])
        if count[b] < 2:
            continue
        _, u, M, F = moments(tot[b, 0], tot[b, 1])
        tr = M[0][0] + M[1][1] + M[2][2]
        uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
        for a in range(3):
            vel[b, a] = float(u[a])
            for c in range(3):
                P[b, a, c] = dens[b] * mass * float(M[a][c] - u[a] * u[c])
            eflux[b, a] = dens[b] * mass / 2 * float(F[a])
            uM = u[0] * M[a][0] + u[1] * M[a][1] + u[2] * M[a][2]
            q[b, a] = dens[b] * mass / 2 * float(F[a] - u[a] * tr - 2 * uM + 2 * u[a] * uu)
        p[b] = (P[b, 0, 0] + P[b, 1, 1] + P[b, 2, 2]) / 3
        if dens[b] > 0:
            T[b] = p[b] / (dens[b] * k_b)
    return {"count": count, "number_density": dens, "velocity": vel, "pressure_tensor": P, "pressure": p, "T": T,
            "energy_flux": eflux, "heat_flux": q, "edges": edges(g), "bin_volume": vol, "n_samples": int(n_samples),
            "n_outside": int(n_outside), "totals": w, "kind": int(g.kind), "shape": (int(g.n1), int(g.n2), int(g.n3))}
