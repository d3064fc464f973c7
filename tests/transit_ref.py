"""The sampled transits' mirror on the host, written from include/argonmc_transit.h: NumPy for the per-particle state, exact
Python ints for the totals.  ``Mirror.sample(x, y, z)`` is one sample of the particles it tracks; ``Mirror.words()`` the totals
in the layout ``amc_transit_read`` returns."""
import numpy as np

from argon_monte_carlo_amd.totals import ints_to_words

COLUMNS, CLASS_COLUMNS, HIST = 263, 43, 40
MAX_SAMPLES = 2 ** 32 - 1
UNKNOWN, BELOW, INSIDE, ABOVE = 0, 1, 2, 3


def class_column(e, x, q=0):
    return 5 + CLASS_COLUMNS * (2 * e + x) + q


def positions(u, lo, hi):
    """below 1 (u < lo), inside 2 (lo <= u < hi), above 3 (u >= hi): plain fp64 comparisons"""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u < lo, BELOW, np.where(u < hi, INSIDE, ABOVE)).astype(np.uint32)


class Mirror:
    def __init__(self, zones, n):
        """zones: [(axis, lo, hi)]; n: the particles tracked"""
        self.zones = [(int(a), float(lo), float(hi)) for a, lo, hi in zones]
        self.n = int(n)
        self.reset()

    def reset(self):
        self.state = np.zeros(self.n, dtype=np.uint32)
        self.entry = np.zeros((len(self.zones), self.n), dtype=np.uint32)
        self.tot = [[0] * COLUMNS for _ in self.zones]
        self.n_samples = 0
        self.bad = None             # the lowest particle (index into the tracked range) with a NaN coordinate
        self.over = False           # a sample beyond the limit was asked for
        self.inside_counts = []     # per sample, per zone: the particles inside after it (for the invariants)

    def load(self, words, n_samples, state=None, entry=None):
        from argon_monte_carlo_amd.totals import words_to_ints
        t = words_to_ints(np.asarray(words, dtype=np.int64).reshape(len(self.zones), COLUMNS, 2))
        self.tot = [[int(v) for v in row] for row in t]
        self.n_samples = int(n_samples)
        self.state = np.zeros(self.n, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32)
        self.entry = np.zeros((len(self.zones), self.n), dtype=np.uint32) if entry is None else np.array(entry, dtype=np.uint32)
        self.bad, self.over = None, False

    def sample(self, x, y, z):
        if self.bad is not None or self.over:
            return
        if self.n_samples >= MAX_SAMPLES:
            self.over = True
            return
        coords = [np.asarray(c, dtype=np.float64) for c in (x, y, z)]
        used = sorted({a for a, _, _ in self.zones})
        nan = np.zeros(self.n, dtype=bool)
        for a in used:
            nan |= np.isnan(coords[a])
        if nan.any():               # the sample adds nothing (the particles' state is unspecified from here on)
            self.bad = int(np.flatnonzero(nan)[0])
            return
        s = self.n_samples
        new_state = np.zeros(self.n, dtype=np.uint32)
        inside_now = []
        for k, (axis, lo, hi) in enumerate(self.zones):
            t = self.tot[k]
            a = (self.state >> np.uint32(4 * k)) & np.uint32(3)
            side = (self.state >> np.uint32(4 * k + 2)) & np.uint32(3)
            b = positions(coords[axis], lo, hi)
            enter = (b == INSIDE) & (a != INSIDE)
            leave = (a == INSIDE) & (b != INSIDE)
            stay = (a == INSIDE) & (b == INSIDE)
            skip = (a != UNKNOWN) & (a != INSIDE) & (b != INSIDE) & (a != b)
            new_side = np.where(a == UNKNOWN, 2, np.where(a == BELOW, 0, 1)).astype(np.uint32)
            for e in range(3):
                t[e] += int((enter & (new_side == e)).sum())
            t[3] += int(skip.sum())
            t[4] += int((b == INSIDE).sum())
            for p in np.flatnonzero(leave):
                tau = (s - int(self.entry[k, p])) & 0xFFFFFFFF
                c = class_column(int(side[p]), 0 if b[p] == BELOW else 1)
                t[c] += 1
                t[c + 1] += tau
                t[c + 2] += tau * tau
                t[c + 3 + min(tau.bit_length() - 1, HIST - 1)] += 1
            self.entry[k, enter] = np.uint32(s)
            nibble = b | (np.where(enter, new_side, np.where(stay, side, 0)).astype(np.uint32) << np.uint32(2))
            new_state |= nibble << np.uint32(4 * k)
            inside_now.append(int((b == INSIDE).sum()))
        self.state = new_state
        self.inside_counts.append(inside_now)
        self.n_samples += 1

    def words(self):
        return ints_to_words(np.array(self.tot, dtype=object).reshape(len(self.zones), COLUMNS))


def merge_words(words_list):
    """the exact sum of several ranks' totals"""
    from argon_monte_carlo_amd.totals import words_to_ints
    total = None
    for w in words_list:
        t = words_to_ints(w)
        total = t if total is None else total + t
    return ints_to_words(total)
