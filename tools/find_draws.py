#!/usr/bin/env python3
"""Search the device draws of the energised pore for the table of chosen draws in tests/test_draws_host.py.

A draw is a function of (seed, particle, step, case, attempt) alone, and for the plane cases 3, 4, 6, 7 the normal is
(0, 0, +-1) exactly, so what a hit of such a case draws is known without running anything.  The search fixes the seed,
walks a fixed sequence of steps in [0, 2^30) (step_k = k * 2654435761 mod 2^30, k = 1, 2, ...) over the particles that
tests/edge_states.temp_draw_hits() gives to each plane case, evaluates every draw with the float64 mirror of
tests/draw_ref.py (NumPy only) and prints, as literals (kind, step, particle, case), the first two draws of each kind:

  u1_lo, u1_hi      the accepted attempt has u1 < 1e-6 / > 1 - 1e-6      (cos theta -> -1 / +1)
  u2_lo, u2_hi      the accepted attempt has u2 < 1e-6 / > 1 - 1e-6      (phi -> 0 / pi)
  redraws           five or more rejections in a row before the accepted attempt
  near_reject       an attempt rejected with cos85 - |d.n| in (1e-12, 1e-6)
  near_accept       accepted without a flip, |d.n| - cos85 in (1e-12, 1e-6)
  near_flip         accepted with a flip, |d.n| - cos85 in (1e-12, 1e-6)
  high_step         steps 2^29 and 0x3fffffff (the largest amc_set_step admits), whatever they draw

The committed table is the output of:   python tools/find_draws.py --seed 0x1234ABCD5678 --draws 8000000
(about 8 million draws per case, half a minute).  --skip-step S leaves a step out: for a step at which some OTHER hit of
the state breaks the margin condition of tests/test_draws_host.py."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import draw_ref as R  # noqa: E402
from tests import edge_states as E  # noqa: E402

PLANE_NORMAL = {3: (0.0, 0.0, 1.0), 4: (0.0, 0.0, -1.0), 6: (0.0, 0.0, 1.0), 7: (0.0, 0.0, -1.0)}
KINDS = ("u1_lo", "u1_hi", "u2_lo", "u2_hi", "redraws", "near_reject", "near_accept", "near_flip")
EDGE, BAND_LO, BAND_HI, STRIDE = 1.0e-6, 1.0e-12, 1.0e-6, 2654435761


def classify(m):
    """{kind: bool per hit} of a draw_ref.mirror() result"""
    n = len(m["attempts"])
    w = m["walked"]
    hit, d = w[:, 0].astype(np.int64), w[:, 4]
    gap = np.abs(d) - R.COS85
    last = w[:, 1].astype(np.int64) == m["attempts"][hit]
    band = (np.abs(gap) > BAND_LO) & (np.abs(gap) < BAND_HI)

    def any_of(rows):
        out = np.zeros(n, dtype=bool)
        out[hit[rows]] = True
        return out
    return {"u1_lo": m["u1"] < EDGE, "u1_hi": m["u1"] > 1.0 - EDGE, "u2_lo": m["u2"] < EDGE, "u2_hi": m["u2"] > 1.0 - EDGE,
            "redraws": m["attempts"] >= 5, "near_reject": any_of(band & (gap < 0.0)),
            "near_accept": any_of(band & last & (gap > 0.0)) & ~m["flip"], "near_flip": any_of(band & last & (gap > 0.0)) & m["flip"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda v: int(v, 0), required=True)
    ap.add_argument("--draws", type=int, default=8_000_000, help="draws per case")
    ap.add_argument("--skip-step", type=lambda v: int(v, 0), action="append", default=[])
    a = ap.parse_args()
    s = E.temp_draw_hits()
    found = {k: [] for k in KINDS}
    for case in sorted(PLANE_NORMAL):
        particles = np.array(s.cases[f"draw_case{case}"], dtype=np.uint64)
        nsteps = a.draws // len(particles)
        chunk = max(1, 1_000_000 // len(particles))
        for k0 in range(1, nsteps + 1, chunk):
            ks = np.arange(k0, min(k0 + chunk, nsteps + 1), dtype=np.uint64)
            steps = (ks * np.uint64(STRIDE)) & np.uint64(0x3FFFFFFF)
            P, S = np.meshgrid(particles, steps, indexing="ij")
            P, S = P.ravel(), S.ravel()
            m = R.mirror(a.seed, P, S, case, PLANE_NORMAL[case])
            for kind, mask in classify(m).items():
                for i in np.flatnonzero(mask):
                    if int(S[i]) not in a.skip_step:
                        found[kind].append((int(ks[i % len(steps)]), int(S[i]), int(P[i]), case))
    table = []
    for kind in KINDS:
        c = sorted(found[kind], key=lambda e: (e[0], e[3], e[2]))          # (in search order: by k, then case, then particle)
        assert len(c) >= 2, (kind, len(c))
        second = next((e for e in c[1:] if e[3] != c[0][3]), c[1])         # (two cases where the search found two)
        table += [(kind, e[1], e[2], e[3]) for e in (c[0], second)]
    table.append(("high_step", 1 << 29, s.cases["draw_case3"][0], 3))
    table.append(("high_step", 0x3FFFFFFF, s.cases["draw_case7"][0], 7))
    print(f"SEED = {a.seed:#x}")
    print("TABLE = (")
    for kind, step, particle, case in table:
        print(f"    ({kind!r}, {step:#010x}, {particle}, {case}),")
    print(")")
    print("# candidates found: " + ", ".join(f"{k} {len(v)}" for k, v in found.items()), file=sys.stderr)


if __name__ == "__main__":
    main()
