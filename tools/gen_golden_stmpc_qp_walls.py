#!/usr/bin/env python3
"""tests/golden/g24_stmpc_qp_walls.npz: the previous solutions of the dynamic QP's wall-row scenes (tests/stmpc_qp_walls_scenes.py: the plain
QP's optimum plus noise, a solve per ego) and the exact optima of its long shapes (T >= 24, the cap's (40, 16) among them) as active sets, from
the yardstick tests/stmpc_qp_walls_ref.py -- not from the reference.  The long horizons take minutes, too long for a unit test; the tests
rebuild every problem and certify the recorded points on it, and solve the short horizons outright.  Asserted here: every ego meets its
family's definition, none is edge-sensitive, every feasible one has a certified exact optimum.  CPU only.

    python tools/gen_golden_stmpc_qp_walls.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import stmpc_qp_walls_scenes as SC  # noqa: E402


def main():
    out = {}
    for T, M in SC.shapes():
        if T not in SC.PREV:
            SC.PREV[T] = SC.compute_prev(T)
            out[f"T{T}_prev_oa"], out[f"T{T}_prev_odv"] = SC.PREV[T]
        sols = SC.solve_scene(T, M)
        SC.assert_families(T, M, sols)
        assert not SC.edge_sensitive(sols) and SC.uncertified(sols) == 0, (T, M, SC.edge_sensitive(sols), SC.uncertified(sols))
        if SC.RECORDED(T):
            for name, a in SC.pack(sols, T).items():
                out[f"T{T}_M{M}_" + name] = a
        feas = [s for s in sols if s]
        print(T, M, "solved", len(feas), "degenerate", sum(s["degenerate"] for s in feas), "eps max %.4f" % max(s["eps"] for s in feas),
              "wall rows", sum(int((s["planes"][:, :, 3] >= 16).sum()) for s in feas),
              "active rows", sum(int((s["avoid_lam"][:-1] > 1e-9).sum()) for s in feas), flush=True)
    path = os.path.join(ROOT, "tests", "golden", SC.GOLDEN_FILE)
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
