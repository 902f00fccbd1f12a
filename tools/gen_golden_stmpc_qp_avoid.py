#!/usr/bin/env python3
"""tests/golden/g22_stmpc_qp_avoid.npz: the exact optima of the dynamic QP's avoidance-row scenes (tests/stmpc_qp_avoid_scenes.py: 32 egos,
16 at the cap, for each of its horizons x M in {1, 4, 16}, and one batch with a margin) from the yardstick tests/stmpc_qp_avoid_ref.py -- not
from the reference.  The long horizons take minutes, too long for a unit test; the tests rebuild every problem and certify the recorded
points on it, and recompute the short horizons outright.  Asserted here: every recorded ego meets its family's definition, every slack
stays below 0.05 m, and at most 1 ego in 16 per shape lacks a certified exact optimum.  CPU only.

    python tools/gen_golden_stmpc_qp_avoid.py [T ...]      (the horizons to redo; the others are kept from the file)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stmpc_qp_avoid_scenes as SC  # noqa: E402


def main():
    path = os.path.join(ROOT, "tests", "golden", SC.GOLDEN_FILE)
    only = [int(a) for a in sys.argv[1:]]
    out = dict(np.load(path, allow_pickle=False)) if only else {}
    for T, M, margin in SC.SHAPES:
        if only and T not in only:
            continue
        if T not in SC.PREV:
            SC.PREV[T] = SC.compute_prev(T)
            out[f"T{T}_prev_oa"], out[f"T{T}_prev_odv"] = SC.PREV[T]
        x0, ref, oa, odv, obs, fam = SC.exact_scene(T, M)
        sols = SC.solve_scene(T, M, margin)
        SC.assert_families(T, M, margin, obs, sols, fam)
        bad = SC.uncertified(sols)
        assert 16 * bad <= len(sols), (T, M, margin, bad)              # a shape that breaks this: change the scene, not the cap
        for name, a in SC.pack(sols, T).items():
            out[SC._key(T, M, margin) + name] = a
        feas = [s for s in sols if s]
        print(T, M, margin, "solved", len(feas), "uncertified", bad, "degenerate", sum(s["degenerate"] for s in feas),
              "eps max %.4f" % max(s["eps"] for s in feas), "active rows", sum(int((s["avoid_lam"][:-1] > 1e-9).sum()) for s in feas), flush=True)
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
