"""Sampled surfaces (include/argonmc.h "sampled surfaces"): the wall bins of the energised pore's seven
surfaces, the default grid and the derived quantities — hit rate, gas-side z-momentum rate and gas-side energy rate per
area — computed on the host from the exact integer totals the device accumulates.  Nothing here needs a GPU.

Totals come as int64[7][nbins + 1][3][2]: per case (3..9, index case - 3) and bin (the last one: hits outside the case's
range) the quantities (count, sum rint(dpz * 2^110), sum rint(dE * 2^97)), each a signed 128-bit number stored as
(low 64 bits, high 64 bits signed).  dpz and dE are the changes of the PARTICLE's z-momentum and energy in the hit
(Temp:384-389): what the gas gains; the wall gains the opposite."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._abi import AMC_SURFACE_CASES, AMC_SURFACE_MAX_BINS, AmcSurfaceGrid
from .energised import CASES
from .fields import words_to_ints

DPZ_SCALE = 2 ** 110
DE_SCALE = 2 ** 97
DPZ_LIMIT = 2.0 ** -70          # kg m/s: |dpz| of a hit the quantiser takes
DE_LIMIT = 2.0 ** -57           # J
QUANTITIES = ("count", "q_dpz", "q_dE")
PLANE_CASES = (3, 4, 6, 7)      # binned by the contact point's r = sqrt(cx*cx + cy*cy)
CYLINDER_CASES = (5, 8, 9)      # binned by the contact point's z
SURFACE_NAMES = {3: "cold plate", 4: "hot plate", 5: "gap side wall", 6: "gap floor", 7: "gap ceiling",
                 8: "hot pore wall", 9: "cold pore wall"}


def make_grid(nbins, lo, hi):
    """An ``AmcSurfaceGrid``, validated like ``amc_surface_config`` (ValueError instead of AMC_ERR_INVALID);
    ``lo`` / ``hi``: seven values, [case - 3]."""
    nbins, lo, hi = int(nbins), [float(v) for v in lo], [float(v) for v in hi]
    if not 1 <= nbins <= AMC_SURFACE_MAX_BINS:
        raise ValueError(f"{nbins} bins: 1 .. {AMC_SURFACE_MAX_BINS}")
    if len(lo) != AMC_SURFACE_CASES or len(hi) != AMC_SURFACE_CASES:
        raise ValueError("a surface grid has one range per energised case (seven)")
    for s in range(AMC_SURFACE_CASES):
        if not (math.isfinite(lo[s]) and math.isfinite(hi[s]) and lo[s] < hi[s]):
            raise ValueError(f"case {3 + s} needs finite bounds lo < hi")
    g = AmcSurfaceGrid()
    g.struct_size, g.nbins = C.sizeof(AmcSurfaceGrid), nbins
    for s in range(AMC_SURFACE_CASES):
        g.lo[s], g.hi[s] = lo[s], hi[s]
    return g


def default_ranges(params):
    """{case: (lo, hi)} from the constants behind the masks (Temp:708-751, temp_mask): the plates 3 / 4 over r in
    [R_p, R_oa] (their masks ask for r^2 > R_p^2), the gap floor / ceiling 6 / 7 over r in [R_p_c, R_g] (r0^2 >= R_p_c^2),
    the gap side wall 5 over z in [t_zgap_lo, t_zgap_hi], the pore walls 8 over [t_z3_hot, t_zgap_lo] and 9 over
    [t_zgap_hi, t_z3_cold].  A contact point is where the particle's CENTRE was; one traced back beyond a range (a
    plate hit whose contact lies inside r < R_p, say) lands in the case's outside bin."""
    p = params
    return {3: (p.R_p, p.R_oa), 4: (p.R_p, p.R_oa), 5: (p.t_zgap_lo, p.t_zgap_hi), 6: (p.R_p_c, p.R_g), 7: (p.R_p_c, p.R_g),
            8: (p.t_z3_hot, p.t_zgap_lo), 9: (p.t_zgap_hi, p.t_z3_cold)}


def default_grid(params, nbins=32):
    r = default_ranges(params)
    return make_grid(nbins, [r[c][0] for c in CASES], [r[c][1] for c in CASES])


def copy_grid(g):
    return AmcSurfaceGrid.from_buffer_copy(g)


def grid_to_array(g):
    """float64[15] for a checkpoint: nbins, lo[7], hi[7]."""
    return np.array([g.nbins] + list(g.lo) + list(g.hi), dtype=np.float64)


def grid_from_array(a):
    a = np.asarray(a, dtype=np.float64)
    return make_grid(int(a[0]), a[1:8], a[8:15])


def edges(g):
    """float64[7, nbins + 1]: bin edges per case, np.linspace(lo, hi, nbins + 1)."""
    return np.stack([np.linspace(g.lo[s], g.hi[s], int(g.nbins) + 1) for s in range(AMC_SURFACE_CASES)])


def wall_radius(params, case):
    """Radius of the cylinder a cylinder case's bins lie on: the gap's wall (case 5), the coated pore's (8, 9)."""
    return float(params.R_g) if case == 5 else float(params.R_p)


def bin_areas(g, params):
    """float64[7, nbins]: pi (r2^2 - r1^2) for the rings of the plane cases, 2 pi R w for the bands of the cylinders."""
    e = edges(g)
    nb = int(g.nbins)
    out = np.empty((AMC_SURFACE_CASES, nb))
    for s, case in enumerate(CASES):
        if case in PLANE_CASES:
            out[s] = [math.pi * (e[s, i + 1] * e[s, i + 1] - e[s, i] * e[s, i]) for i in range(nb)]
        else:
            w = (g.hi[s] - g.lo[s]) / nb
            out[s] = 2 * math.pi * wall_radius(params, case) * w
    return out


def _mean(total, scale, n_steps):
    """total / scale per step as ONE correctly rounded int / int; NaN without steps."""
    return int(total) / (scale * n_steps) if n_steps > 0 else math.nan


def derive(totals, n_steps, dt, grid, params, n_failed=None):
    """Per case and bin, from the integer totals: ``hit_rate`` (hits / s / m^2), ``momentum_rate`` (gas-side z-momentum per
    time and area, Pa: the sum of the particles' dp_z) and ``energy_rate`` (gas-side energy per time and area, W / m^2),
    float64[7, nbins]; and per case over ALL its hits, the outside bin included: ``case_count``, ``case_outside``,
    ``case_hit_rate`` (1 / s), ``case_momentum_rate`` (N), ``case_energy_rate`` (W).  Exact integers until the one
    correctly rounded int / int per value (sum / (scale * n_steps)), then divided by dt and the bin's area.
    ``n_steps == 0`` gives NaN rates."""
    nb = int(grid.nbins)
    n_steps, dt = int(n_steps), float(dt)
    words = np.asarray(totals, dtype=np.int64).reshape(AMC_SURFACE_CASES, nb + 1, 3, 2)
    tot = words_to_ints(words)
    area = bin_areas(grid, params)
    scales = (1, DPZ_SCALE, DE_SCALE)
    per_bin = np.full((3, AMC_SURFACE_CASES, nb), np.nan)
    per_case = np.full((3, AMC_SURFACE_CASES), np.nan)
    for q in range(3):
        for s in range(AMC_SURFACE_CASES):
            for b in range(nb):
                per_bin[q, s, b] = _mean(tot[s, b, q], scales[q], n_steps) / (dt * area[s, b])
            per_case[q, s] = _mean(sum(int(v) for v in tot[s, :, q]), scales[q], n_steps) / dt
    count = np.array([[int(v) for v in tot[s, :nb, 0]] for s in range(AMC_SURFACE_CASES)], dtype=np.int64)
    return {"count": count, "hit_rate": per_bin[0], "momentum_rate": per_bin[1], "energy_rate": per_bin[2],
            "case_count": np.array([sum(int(v) for v in tot[s, :, 0]) for s in range(AMC_SURFACE_CASES)], dtype=np.int64),
            "case_outside": np.array([int(tot[s, nb, 0]) for s in range(AMC_SURFACE_CASES)], dtype=np.int64),
            "case_hit_rate": per_case[0], "case_momentum_rate": per_case[1], "case_energy_rate": per_case[2],
            "edges": edges(grid), "bin_area": area, "n_steps": n_steps, "dt": dt, "cases": np.array(CASES),
            "n_failed": np.zeros(AMC_SURFACE_CASES, dtype=np.int64) if n_failed is None else np.asarray(n_failed, dtype=np.int64),
            "totals": words, "grid": grid_to_array(grid)}
