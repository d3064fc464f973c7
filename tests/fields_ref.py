"""NumPy reference of the sampled fields (include/argonmc.h "sampled fields"): bins, per-particle components and the
fixed-point quantisation, with the per-bin sums done exactly (32-bit halves in int64, recombined as Python ints)."""
import numpy as np

from argon_monte_carlo_amd import fields as FL


def _axis(u, lo, hi, w, n):
    with np.errstate(invalid="ignore"):
        f = np.floor((u - lo) / w)
        i = np.full(u.shape, -1, dtype=np.int64)
        ok = (f >= 0) & (f < n)
        i[ok] = f[ok].astype(np.int64)
        i[(f == n) & (u <= hi)] = n - 1
    return i


def bins_and_components(g, x, y, z, vx, vy, vz):
    """(linear bin or -1 outside, c1, c2, c3) per particle, evaluated like the device does."""
    x, y, z, vx, vy, vz = (np.asarray(a, dtype=np.float64) for a in (x, y, z, vx, vy, vz))
    w = FL.widths(g)
    if g.kind == FL.AMC_FIELDS_CARTESIAN:
        i1 = _axis(x, g.lo[0], g.hi[0], w[0], g.n1)
        i2 = _axis(y, g.lo[1], g.hi[1], w[1], g.n2)
        i3 = _axis(z, g.lo[2], g.hi[2], w[2], g.n3)
        c1, c2, c3 = vx.copy(), vy.copy(), vz.copy()
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt(x * x + y * y)
            i1 = _axis(r, g.lo[0], g.hi[0], w[0], g.n1)
            i2 = _axis(z, g.lo[1], g.hi[1], w[1], g.n2)
            i3 = np.zeros_like(i1)
            pos = r > 0
            c1 = np.where(pos, (x * vx + y * vy) / r, vx)
            c2 = np.where(pos, (x * vy - y * vx) / r, vy)
        c3 = vz.copy()
    inside = (i1 >= 0) & (i2 >= 0) & (i3 >= 0)
    b = np.where(inside, (i1 * g.n2 + i2) * g.n3 + i3, -1)
    return b, c1, c2, c3


def quantise(c):
    """q1(c) = rint(c * 2^24), q2(c) = rint((c * c) * 2^10) — round half to even, as llrint on the device."""
    c = np.asarray(c, dtype=np.float64)
    return np.rint(c * 2.0 ** 24).astype(np.int64), np.rint((c * c) * 2.0 ** 10).astype(np.int64)


def _exact_bin_sums(b, v, bins):
    lo = (v & 0xFFFFFFFF).astype(np.int64)
    hi = v >> 32
    s_lo = np.zeros(bins, dtype=np.int64)
    s_hi = np.zeros(bins, dtype=np.int64)
    np.add.at(s_lo, b, lo)
    np.add.at(s_hi, b, hi)
    return [int(s_hi[k]) * (1 << 32) + int(s_lo[k]) for k in range(bins)]


class RangeError(ValueError):
    def __init__(self, index):
        super().__init__(f"particle {index} has a velocity component outside |c| < 2^14")
        self.index = index


def sample(g, x, y, z, vx, vy, vz):
    """One sample: (object[bins, 7] exact Python-int sums, particles outside).  Raises RangeError like the device reports
    AMC_ERR_CAPACITY."""
    b, c1, c2, c3 = bins_and_components(g, x, y, z, vx, vy, vz)
    ins = b >= 0
    with np.errstate(invalid="ignore"):
        bad = ins & ~((np.abs(c1) < 2.0 ** 14) & (np.abs(c2) < 2.0 ** 14) & (np.abs(c3) < 2.0 ** 14))
    if bad.any():
        raise RangeError(int(np.flatnonzero(bad)[0]))
    bins = FL.grid_bins(g)
    bi = b[ins]
    out = np.empty((bins, 7), dtype=object)
    out[:, 0] = _exact_bin_sums(bi, np.ones(len(bi), dtype=np.int64), bins)
    for k, c in enumerate((c1, c2, c3)):
        q1, q2 = quantise(c[ins])
        out[:, 1 + k] = _exact_bin_sums(bi, q1, bins)
        out[:, 4 + k] = _exact_bin_sums(bi, q2, bins)
    return out, int((~ins).sum())


def sample_state(g, st, lo=0, hi=None):
    """``sample`` of a downloaded state dict (Engine.download()) over the index range [lo, hi)."""
    hi = len(st["x"]) if hi is None else hi
    return sample(g, *(st[k][lo:hi] for k in ("x", "y", "z", "vx", "vy", "vz")))


def as_words(sums):
    return FL.ints_to_words(sums)
