"""The samplers' 128-bit totals on the host (fields.py, surface.py, correlations.py): the conversions between the device's
(low, high) int64 words, exact Python ints and 32-bit limbs, and the one collective that sums them over the ranks of a sharded
run.  Nothing here needs a GPU."""
from __future__ import annotations

import re

import numpy as np

from ._abi import AMC_ERR_CAPACITY


def words_to_ints(words):
    """int64[..., 2] (low, high) words -> object array of exact Python ints (signed 128-bit values)."""
    words = np.asarray(words, dtype=np.int64)
    lo = words[..., 0].astype(np.uint64)
    hi = words[..., 1]
    out = np.empty(lo.shape, dtype=object)
    for idx in np.ndindex(lo.shape):
        out[idx] = (int(hi[idx]) << 64) + int(lo[idx])
    return out


def ints_to_words(values):
    """The inverse of ``words_to_ints``: signed 128-bit Python ints -> int64[..., 2] (low, high)."""
    values = np.asarray(values, dtype=object)
    out = np.empty(values.shape + (2,), dtype=np.int64)
    for idx in np.ndindex(values.shape):
        v = int(values[idx])
        if not -(1 << 127) <= v < (1 << 127):
            raise OverflowError("total outside the signed 128-bit range")
        u = v & ((1 << 128) - 1)
        lo, hi = u & ((1 << 64) - 1), u >> 64
        out[idx + (0,)] = lo - (1 << 64) if lo >= (1 << 63) else lo
        out[idx + (1,)] = hi - (1 << 64) if hi >= (1 << 63) else hi
    return out


def words_to_limbs(words):
    """int64[..., 2] words -> int64[..., 4] 32-bit limbs (the top one signed): a sum of limbs over ranks, recombined by
    ``limbs_to_words``, is the exact sum of the 128-bit values (no float, no overflow below 2^31 ranks)."""
    words = np.asarray(words, dtype=np.int64)
    lo = words[..., 0].astype(np.uint64)
    hi = words[..., 1]
    m = np.uint64(0xFFFFFFFF)
    return np.stack([(lo & m).astype(np.int64), (lo >> np.uint64(32)).astype(np.int64),
                     (hi.astype(np.uint64) & m).astype(np.int64), hi >> 32], axis=-1)


def limbs_to_words(limbs):
    limbs = np.asarray(limbs, dtype=np.int64)
    vals = np.empty(limbs.shape[:-1], dtype=object)
    for idx in np.ndindex(vals.shape):
        l0, l1, l2, l3 = (int(v) for v in limbs[idx])
        vals[idx] = l0 + (l1 << 32) + (l2 << 64) + (l3 << 96)
    return ints_to_words(vals)


def sum_over_ranks(comm, world, rank, err, arrays, counters, describe, own_if_all_failed=False):
    """A sampler's read summed over the ranks (a collective) -> (arrays, counters).  ``arrays``: this rank's int64[..., 2] word
    arrays, summed as 32-bit limbs; ``counters``: its plain integers; all in ONE ``comm.allreduce_sum_ints`` — exact, never
    through floats — whose first ``world`` entries carry every rank's status.  ``err``: the error this rank's read raised, or
    None (the caller then passes zeros): it still takes part, so that a read which fails on one rank fails on every rank, from
    this call.  Its status is the particle's index + 1 for an AMC_ERR_CAPACITY that names a particle, else the negative error
    code.  Every rank raises ``describe(r, status)`` for the first failing rank r; a single rank re-raises its own error, and
    with ``own_if_all_failed`` so do ranks that all failed.  A communicator of one rank with ``shortcut`` set skips the
    all-reduce."""
    status = [0] * world
    if err is not None:
        m = re.search(r"particle (\d+) ", str(err)) if err.code == AMC_ERR_CAPACITY else None
        status[rank] = int(m.group(1)) + 1 if m else min(int(err.code), -1)
    limbs = [words_to_limbs(a) for a in arrays]
    flat = status + [int(v) for l in limbs for v in l.ravel()] + [int(v) for v in counters]
    if world > 1 or not getattr(comm, "shortcut", True):
        flat = comm.allreduce_sum_ints(flat)
    failed = [(r, s) for r, s in enumerate(flat[:world]) if s != 0]
    if failed:
        if err is not None and len(failed) == world and (world == 1 or own_if_all_failed):
            raise err
        raise describe(*failed[0]) from err
    out, at = [], world
    for l in limbs:
        out.append(limbs_to_words(np.array(flat[at:at + l.size], dtype=np.int64).reshape(l.shape)))
        at += l.size
    return out, [int(v) for v in flat[at:]]
