#!/usr/bin/env python3
"""Search the Maxwell wall law's draws for the table of chosen step words in tests/test_wall_law_host.py — the
sibling of tools/find_draws.py for include/argonmc-walllaw.h.

The law's four uniforms are a function of (seed, particle, step, case) alone, so what a hit draws is known without running
anything.  The search fixes the seed and the two alpha, walks find_draws.py's sequence of steps in [0, 2^30)
(step_k = k * 2654435761 mod 2^30, k = 1, 2, ...) over the particles tests/edge_states.temp_draw_hits() gives to each case and
prints, as literals (kind, step, particle, case), per kind the one draw that goes furthest:

  ua_lo, ua_hi      the smallest / largest ua of a diffuse hit          (vn -> 0 / the largest normal speed)
  ub_lo, ub_hi      the smallest / largest ub of a diffuse hit          (likewise the tangential speed)
  coated_below, coated_above    u0 closest to alpha_coated from below (the last diffuse hit) / from above or equal (the first
                                specular one), cases other than 5
  gap_below, gap_above          the same against alpha_gap, case 5
  high_step         steps 2^29 and 0x3fffffff (the largest amc_set_step admits), whatever they draw

The committed table is the output of:
    python tools/find_wall_law_draws.py --seed 0x1234ABCD5678 --alpha-coated 0.95 --alpha-gap 0.8 --draws 4000000"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import edge_states as E  # noqa: E402
from tests import wall_law_ref as W  # noqa: E402

STRIDE = 2654435761


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda v: int(v, 0), required=True)
    ap.add_argument("--alpha-coated", type=float, required=True)
    ap.add_argument("--alpha-gap", type=float, required=True)
    ap.add_argument("--draws", type=int, default=4_000_000, help="draws over all cases")
    a = ap.parse_args()
    s = E.temp_draw_hits()
    who = {case: list(s.cases[f"draw_case{case}"]) for case in range(3, 10)}
    who[5] += list(s.cases["draw_ladder"])
    nsteps = a.draws // sum(len(v) for v in who.values())
    ks = np.arange(1, nsteps + 1, dtype=np.uint64)
    steps = (ks * np.uint64(STRIDE)) & np.uint64(0x3FFFFFFF)
    best = {}           # kind -> (score, step, particle, case): the smallest score wins, ties by search order

    def offer(kind, score, S, P, case, mask):
        if not mask.any():
            return
        sc = np.where(mask, score, np.inf)
        i = int(np.argmin(sc))
        if kind not in best or sc[i] < best[kind][0]:
            best[kind] = (float(sc[i]), int(S[i]), int(P[i]), case)

    for case in sorted(who):
        P, S = np.meshgrid(np.array(who[case], dtype=np.uint64), steps, indexing="ij")
        P, S = P.ravel(), S.ravel()
        u0, ua, ub, _ = W.uniforms(a.seed, P, S, case)
        alpha = a.alpha_gap if case == 5 else a.alpha_coated
        diffuse = u0 < alpha
        offer("ua_lo", ua, S, P, case, diffuse)
        offer("ua_hi", 1.0 - ua, S, P, case, diffuse)
        offer("ub_lo", ub, S, P, case, diffuse)
        offer("ub_hi", 1.0 - ub, S, P, case, diffuse)
        name = "gap" if case == 5 else "coated"
        offer(name + "_below", alpha - u0, S, P, case, diffuse)
        offer(name + "_above", u0 - alpha, S, P, case, ~diffuse)
    kinds = ("ua_lo", "ua_hi", "ub_lo", "ub_hi", "coated_below", "coated_above", "gap_below", "gap_above")
    table = [(k,) + best[k][1:] for k in kinds]
    table.append(("high_step", 1 << 29, who[3][0], 3))
    table.append(("high_step", 0x3FFFFFFF, who[5][0], 5))
    print(f"SEED, ALPHA_COATED, ALPHA_GAP = {a.seed:#x}, {a.alpha_coated!r}, {a.alpha_gap!r}")
    print("TABLE = (")
    for kind, step, particle, case in table:
        print(f"    ({kind!r}, {step:#010x}, {particle}, {case}),")
    print(")")
    print("# scores: " + ", ".join(f"{k} {best[k][0]:.3g}" for k in kinds), file=sys.stderr)


if __name__ == "__main__":
    main()
