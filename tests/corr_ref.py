"""NumPy / Python-int reference of the sampled correlations (include/argonmc.h "sampled correlations"): the group of the
origin position, the fixed-point quantisation of the squared displacement components and of the velocity products, and the
per-group sums done exactly (Python ints).  ``Window`` follows the device's window over a sequence of samples."""
import numpy as np

from argon_monte_carlo_amd import correlations as CO
from tests import fields_ref as FREF

KEYS6 = ("x", "y", "z", "vx", "vy", "vz")
D_LIMIT = 2.0 ** -18
V_LIMIT = 2.0 ** 14


class RangeError(ValueError):
    def __init__(self, index):
        super().__init__(f"particle {index} is outside the quantisers' range")
        self.index = index


def groups_of(g, x, y, z):
    """Linear group (or -1 outside) of every position, by the bin rule of the sampled fields."""
    zero = np.zeros(len(x))
    return FREF.bins_and_components(g, x, y, z, zero, zero, zero)[0]


def quantise_m(d):
    """m = rint(ldexp(d * d, 74)) — round half to even, as llrint on the device."""
    d = np.asarray(d, dtype=np.float64)
    return [int(v) for v in np.rint(np.ldexp(d * d, 74))]


def quantise_c(v, v0):
    """c = rint((v * v0) * 2^10)."""
    v, v0 = np.asarray(v, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    return [int(a) for a in np.rint((v * v0) * 2.0 ** 10)]


def _speeds_ok(vx, vy, vz):
    with np.errstate(invalid="ignore"):
        return (np.abs(vx) < V_LIMIT) & (np.abs(vy) < V_LIMIT) & (np.abs(vz) < V_LIMIT)


def sample(g, origin, current):
    """One lag sample: ``origin`` and ``current`` are (x, y, z, vx, vy, vz) of the same particles.  Returns (object[groups, 7]
    exact Python-int sums: count, m_x m_y m_z, c_x c_y c_z; particles whose origin is outside the grid).  A participating
    particle out of range raises RangeError with the lowest such index, as the device reports AMC_ERR_CAPACITY."""
    o = [np.asarray(a, dtype=np.float64) for a in origin]
    c = [np.asarray(a, dtype=np.float64) for a in current]
    grp = groups_of(g, o[0], o[1], o[2])
    ins = grp >= 0
    with np.errstate(invalid="ignore"):
        d = [c[k] - o[k] for k in range(3)]
        d_ok = (np.abs(d[0]) < D_LIMIT) & (np.abs(d[1]) < D_LIMIT) & (np.abs(d[2]) < D_LIMIT)
    bad = ins & ~(d_ok & _speeds_ok(*c[3:]) & _speeds_ok(*o[3:]))
    if bad.any():
        raise RangeError(int(np.flatnonzero(bad)[0]))
    groups = CO.grid_groups(g)
    out = np.empty((groups, 7), dtype=object)
    out[:] = 0
    idx = np.flatnonzero(ins)
    gi = grp[idx]
    cols = [[1] * len(idx)] + [quantise_m(d[k][idx]) for k in range(3)] + [quantise_c(c[3 + k][idx], o[3 + k][idx]) for k in range(3)]
    for q, col in enumerate(cols):
        for b, v in zip(gi.tolist(), col):
            out[b, q] += v
    return out, int((~ins).sum())


def state6(st, lo=0, hi=None):
    """(x, y, z, vx, vy, vz) of a downloaded state dict (Engine.download()) over the index range [lo, hi)."""
    hi = len(st["x"]) if hi is None else hi
    return tuple(np.array(st[k][lo:hi], dtype=np.float64) for k in KEYS6)


class Window:
    """The device's window over a sequence of samples: totals object[groups, n_lags + 1, 7] and the counters."""

    def __init__(self, g):
        self.g = g
        self.n_lags = int(g.n_lags)
        self.totals = np.empty((CO.grid_groups(g), self.n_lags + 1, 7), dtype=object)
        self.totals[:] = 0
        self.pos, self.origin = 0, None
        self.n_origins = self.n_samples = self.n_outside = 0

    def add(self, current):
        """One sample of the state ``current`` = (x, y, z, vx, vy, vz)."""
        if self.pos > 0:
            s, _ = sample(self.g, self.origin, current)
            self.totals[:, self.pos] = self.totals[:, self.pos] + s
        if self.pos == 0 or self.pos == self.n_lags:
            s, outside = sample(self.g, current, current)
            self.totals[:, 0] = self.totals[:, 0] + s
            self.origin = tuple(a.copy() for a in current)
            self.n_origins += 1
            self.n_outside += outside
            self.pos = 1
        else:
            self.pos += 1
        self.n_samples += 1

    def counters(self):
        return (self.n_origins, self.n_samples, self.n_outside, self.pos)

    def words(self):
        return CO.ints_to_words(self.totals)
