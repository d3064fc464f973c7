"""Sampled transits (include/argonmc_transit.h): the zones, the default zones per geometry and the derived
quantities — transmission and return probabilities, residence times, entry and exit rates, occupancy — computed on the host
from the exact integer totals the device accumulates.  Nothing here needs a GPU.

A zone is a half-open interval [lo, hi) of one Cartesian coordinate.  Totals come as int64[n_zones][263][2]: per zone 263
columns, each a signed 128-bit number stored as (low 64 bits, high 64 bits signed):
  0, 1, 2   entries from below, from above, already inside when first seen
  3         skipped (a crossing no sample saw)
  4         inside_sum (particles inside, summed over the samples)
  5 + 43 * (2 * e + x) + q   the exit class (entry side e = 0, 1, 2; exit side x = 0 below, 1 above):
            q = 0 count, 1 sum of tau, 2 sum of tau^2, 3 + j the residences with floor(log2(tau)) == j (j = 39: and beyond),
            tau the residence in samples."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from ._abi import (AMC_GEOM_CUBE, AMC_TRANSIT_CLASS_COLUMNS, AMC_TRANSIT_COLUMNS, AMC_TRANSIT_HIST, AMC_TRANSIT_MAX_SAMPLES,
                   AMC_TRANSIT_MAX_ZONES, AmcTransitGrid)
from .totals import ints_to_words, words_to_ints  # noqa: F401

ENTRY_SIDES = ("below", "above", "inside")      # the side a particle entered from (inside: it was there when first seen)
EXIT_SIDES = ("below", "above")
COL_ENTRIES, COL_SKIPPED, COL_INSIDE_SUM, COL_CLASSES = 0, 3, 4, 5
# the position of a particle relative to a zone, two bits of its state word
UNKNOWN, BELOW, INSIDE, ABOVE = 0, 1, 2, 3


def class_column(e, x, q=0):
    """column of quantity q (0 count, 1 sum tau, 2 sum tau^2, 3 + j histogram) of the exit class (entry side e, exit side x)"""
    return COL_CLASSES + AMC_TRANSIT_CLASS_COLUMNS * (2 * int(e) + int(x)) + int(q)


def make_grid(zones, every=1, step_offset=0, reserved=(0, 0)):
    """An ``AmcTransitGrid``, validated like ``amc_transit_config`` (ValueError instead of AMC_ERR_INVALID).  ``zones``: 1 .. 8
    triples (axis, lo, hi), axis 0, 1, 2 (or "x", "y", "z"), finite lo < hi."""
    zones = list(zones)
    if not 1 <= len(zones) <= AMC_TRANSIT_MAX_ZONES:
        raise ValueError(f"{len(zones)} zones: 1 .. {AMC_TRANSIT_MAX_ZONES}")
    every, step_offset = int(every), int(step_offset)
    if every < 0 or step_offset < 0:
        raise ValueError("every and step_offset must be >= 0")
    if any(int(r) != 0 for r in reserved):
        raise ValueError("reserved words must be 0")
    g = AmcTransitGrid()
    g.struct_size = C.sizeof(AmcTransitGrid)
    g.n_zones, g.every, g.step_offset = len(zones), every, step_offset
    for k, (axis, lo, hi) in enumerate(zones):
        axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
        if axis not in (0, 1, 2):
            raise ValueError(f"zone {k}: axis {axis!r} (0, 1 or 2)")
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f"zone {k} needs finite bounds lo < hi")
        g.axis[k], g.lo[k], g.hi[k] = int(axis), lo, hi
    return g


def copy_grid(g, every=None, step_offset=None):
    out = AmcTransitGrid.from_buffer_copy(g)
    if every is not None:
        if int(every) < 0:
            raise ValueError("every must be >= 0")
        out.every = int(every)
    if step_offset is not None:
        out.step_offset = int(step_offset)
    return out


def zones(g):
    """[(axis, lo, hi)] of the grid"""
    return [(int(g.axis[k]), float(g.lo[k]), float(g.hi[k])) for k in range(int(g.n_zones))]


def default_grid(params, every=1):
    """The geometry's natural zones.  Pore, specular or energised, along z: the whole coated section [h_oa, z_cold), the hot
    coating [h_oa, z_gap_bottom), the gap [z_gap_bottom, z_gap_top) and the cold coating [z_gap_top, z_cold).  Cube: the three
    thirds of x over [0, cube_x].  A sample after every step."""
    if int(params.geometry) == AMC_GEOM_CUBE:
        L = float(params.cube_x)
        a, b = L / 3.0, 2.0 * L / 3.0
        return make_grid([(0, 0.0, a), (0, a, b), (0, b, L)], every=every)
    p = params
    return make_grid([(2, p.h_oa, p.z_cold), (2, p.h_oa, p.z_gap_bottom), (2, p.z_gap_bottom, p.z_gap_top), (2, p.z_gap_top, p.z_cold)],
                     every=every)


def totals_shape(g):
    return (int(g.n_zones), AMC_TRANSIT_COLUMNS, 2)


def grid_to_array(g):
    """float64[3 + 24] for a checkpoint: n_zones, every, step_offset, axis[8], lo[8], hi[8]."""
    return np.array([g.n_zones, g.every, g.step_offset] + list(g.axis) + list(g.lo) + list(g.hi), dtype=np.float64)


def grid_from_array(a):
    """the inverse of ``grid_to_array``"""
    a = np.asarray(a, dtype=np.float64)
    n, Z = int(a[0]), AMC_TRANSIT_MAX_ZONES
    return make_grid([(int(a[3 + k]), float(a[3 + Z + k]), float(a[3 + 2 * Z + k])) for k in range(n)], int(a[1]), int(a[2]))


def hist_edges():
    """the residence histogram's edges in samples: column j holds 2^j <= tau < 2^(j+1), the last one everything from 2^39"""
    return np.array([2.0 ** j for j in range(AMC_TRANSIT_HIST)] + [math.inf])


def split(g, words):
    """the totals by name, as exact Python ints (object arrays): entries [zones, 3], skipped [zones], inside_sum [zones],
    count, sum_tau, sum_tau2 [zones, 3, 2] and hist [zones, 3, 2, 40] (entry side, exit side)"""
    Z = int(g.n_zones)
    t = words_to_ints(np.asarray(words, dtype=np.int64).reshape(Z, AMC_TRANSIT_COLUMNS, 2))
    cls = t[:, COL_CLASSES:].reshape(Z, 3, 2, AMC_TRANSIT_CLASS_COLUMNS)
    return {"entries": t[:, 0:3], "skipped": t[:, COL_SKIPPED], "inside_sum": t[:, COL_INSIDE_SUM], "count": cls[..., 0],
            "sum_tau": cls[..., 1], "sum_tau2": cls[..., 2], "hist": cls[..., 3:]}


def _ratio(a, b):
    return float(Fraction(int(a), int(b))) if int(b) > 0 else math.nan


def derive(g, words, n_samples, dt, every=None):
    """Per zone from the integer totals.  One sample interval lasts ``interval = every * dt`` seconds (``every``: the grid's
    unless given; 0, samples on demand only, counts as 1), the sampled time is T = n_samples * interval.  With c[e][x] the
    exits of class (entry side e, exit side x):
      transmission[z, 0]     c[0][1] / (c[0][0] + c[0][1])   of the particles that came in from below, the share that left above
      transmission[z, 1]     c[1][0] / (c[1][0] + c[1][1])   ... from above, the share that left below
      return_probability     1 - transmission (the same Fractions' complements)
      transmission_err       sqrt(p (1 - p) / n), the binomial standard error of both
      residence_mean[z,e,x]  sum_tau / c * interval                                   s
      residence_var[z,e,x]   (sum_tau2 / c - (sum_tau / c)^2) * interval^2            s^2
      entry_rate[z, e]       entries[e] / T                                           per s
      exit_rate[z, x]        (c[0][x] + c[1][x] + c[2][x]) / T                        per s
      occupancy[z]           inside_sum / n_samples                                   particles
      little_residence[z]    occupancy / (exit_rate[z, 0] + exit_rate[z, 1])          s   (Little's law)
      inside_now[z]          entries - exits: the particles inside after the last sample
      hist[z, e, x, 40]      the residence histogram, hist_edges_s its 41 edges in seconds (the last one inf)
    Ratios of totals are formed exactly, as ``Fraction``s of Python ints, and rounded to a float once; what is multiplied by
    the interval is float arithmetic in the order written.  An empty class has NaN probabilities, means and variances."""
    Z = int(g.n_zones)
    s = split(g, words)
    every = int(g.every) if every is None else int(every)
    interval = float(max(every, 1)) * float(dt)
    n_samples = int(n_samples)
    T = n_samples * interval
    count = np.array([[[int(v) for v in r] for r in zc] for zc in s["count"]], dtype=np.int64).reshape(Z, 3, 2)
    entries = np.array([[int(v) for v in r] for r in s["entries"]], dtype=np.int64).reshape(Z, 3)
    trans = np.full((Z, 2), np.nan)
    ret = np.full((Z, 2), np.nan)
    err = np.full((Z, 2), np.nan)
    mean = np.full((Z, 3, 2), np.nan)
    var = np.full((Z, 3, 2), np.nan)
    entry_rate = np.full((Z, 3), np.nan)
    exit_rate = np.full((Z, 2), np.nan)
    occ = np.full(Z, np.nan)
    little = np.full(Z, np.nan)
    inside_now = np.zeros(Z, dtype=np.int64)
    for z in range(Z):
        for e in range(2):
            through, back = int(count[z, e, 1 - e]), int(count[z, e, e])
            n = through + back
            if n > 0:
                p = Fraction(through, n)
                trans[z, e], ret[z, e] = float(p), float(1 - p)
                err[z, e] = math.sqrt(float(p * (1 - p) / n))
        for e in range(3):
            for x in range(2):
                n = int(count[z, e, x])
                if n < 1:
                    continue
                m = Fraction(int(s["sum_tau"][z, e, x]), n)
                mean[z, e, x] = float(m) * interval
                var[z, e, x] = float(Fraction(int(s["sum_tau2"][z, e, x]), n) - m * m) * interval * interval
        inside_now[z] = int(entries[z].sum()) - int(count[z].sum())
        if n_samples > 0:
            entry_rate[z] = entries[z] / T
            exit_rate[z] = count[z].sum(axis=0) / T
            occ[z] = _ratio(s["inside_sum"][z], n_samples)
            out = float(exit_rate[z].sum())
            if out > 0.0:
                little[z] = occ[z] / out
    hist = np.array([int(v) for v in s["hist"].ravel()], dtype=np.int64).reshape(Z, 3, 2, AMC_TRANSIT_HIST)
    return {"zones": np.array(zones(g), dtype=np.float64), "transmission": trans, "return_probability": ret, "transmission_err": err,
            "count": count, "entries": entries, "skipped": np.array([int(v) for v in s["skipped"]], dtype=np.int64),
            "residence_mean": mean, "residence_var": var, "entry_rate": entry_rate, "exit_rate": exit_rate, "occupancy": occ,
            "little_residence": little, "inside_now": inside_now, "hist": hist, "hist_edges": hist_edges(),
            "hist_edges_s": hist_edges() * interval, "interval": interval, "n_samples": n_samples,
            "totals": np.asarray(words, dtype=np.int64).reshape(Z, AMC_TRANSIT_COLUMNS, 2)}
