#!/usr/bin/env python3
"""tests/golden/g23_kmpc_qp_walls.npz: the exact optima of the T = 31 shape of the wall-row scenes (tests/kmpc_qp_walls_scenes.py: 65 egos,
M = 16) from tests/kmpc_qp_walls_ref.py.  That batch takes about a minute, too long for a unit test; the tests rebuild every problem and
certify the recorded points on it, and solve the short horizons outright.  CPU only.

    python tools/gen_golden_kmpc_qp_walls.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import kmpc_qp_walls_scenes as SC  # noqa: E402


def main():
    out = {}
    for T, M in SC.SHAPES:
        if T < 31:
            continue
        sols = SC.solve_scene(T, M)
        n, k = 2 * T, f"T{T}_M{M}_"
        out[k + "solved"] = np.array([s is not None for s in sols])
        out[k + "w"] = np.array([s["w"] if s else np.full(n + 1, np.nan) for s in sols])
        out[k + "lam"] = np.array([s["lam"][:8 * T - 2] if s else np.full(8 * T - 2, np.nan) for s in sols])
        out[k + "avoid_lam"] = np.array([s["avoid_lam"] if s else np.full(n + 1, np.nan) for s in sols])
        out[k + "degenerate"] = np.array([bool(s and s["degenerate"]) for s in sols])
        print(T, M, "solved", int(out[k + "solved"].sum()), "degenerate", int(out[k + "degenerate"].sum()), flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", SC.GOLDEN_FILE), **out)


if __name__ == "__main__":
    main()
