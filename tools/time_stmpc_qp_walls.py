#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_qp_plan_batch with the wall rows on (f1p_stmpc_qp_set_walls) at 1024 egos x T 40 and 4096 x
T 10, without discs (M = 0) and with M = 4 discs per ego, beside the avoidance variant (M = 4) and the plain QP in the same process: branch
split, reference extraction, linearisation, march, QP solve, output map, warm start -- one call.  States and discs are
tools/time_stmpc_qp_avoid.py's (every ego above V_KS: the dynamic branch).  The map is the synthetic track's corridor of 1.0 m half width --
narrower than the reach of 1.5 m -- with the right half of the image cleared, so about half the egos have walls in reach and the others none.
Each figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call, median and spread over the blocks; the
interior-point iteration counts and the status histogram come from the stateless entry points on the same first-call problem.  Prints one
JSON object; --out also writes it.  --merge-parent FILE adds, per shape under `parent_commit_avoid`, the avoidance figure of a
tools/time_stmpc_qp_avoid.py record taken with the PARENT commit's library in the same session: the baseline this tree's avoidance leg (the
same instructions) must sit on and the wall legs are compared with.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd._planner import qp_wall_samples  # noqa: E402
from f1tenth_planning_amd.runtime import (Context, stmpc_qp_avoid, stmpc_qp_set_avoid, stmpc_qp_set_walls, stmpc_qp_walls,  # noqa: E402
                                          stmpc_set_obstacles)
from time_kmpc_qp import _time  # noqa: E402
from time_stmpc_qp import _states  # noqa: E402
from time_stmpc_qp_avoid import _counts, discs  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--discs", type=int, default=4)
    ap.add_argument("--reach", type=float, default=1.5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--merge-parent", metavar="FILE", help="a tools/time_stmpc_qp_avoid.py record of the parent commit, same session: its avoidance figures are kept beside these")
    args = ap.parse_args()
    M = args.discs
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    resolution = 0.05
    img, origin = synth.make_grid(rl[:, :2], size=(900, 900), resolution=resolution, half_width=1.0)
    img = img.copy()
    img[:, img.shape[1] // 2:] = 255                             # the right half of the map: no wall anywhere
    walls = _abi.kmpc_qp_walls(n_samples=qp_wall_samples(args.reach, resolution))
    parent = {}
    if args.merge_parent:
        with open(args.merge_parent) as f:
            par = json.load(f)
        parent = {(r["egos"], r["horizon"]): r for r in par["shapes"]}
    res = {"tool": "tools/time_stmpc_qp_walls.py", "discs": M, "reach": args.reach, "n_samples": walls.n_samples, "calls": args.calls,
           "repeats": args.repeats, "warmup": args.warmup, "shapes": []}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        ctx.set_grid(img, resolution, origin, 128)
        for E, T in ((1024, 40), (4096, 10)):
            x0 = _states(rl, E, E + T, False)
            obs = discs(x0, M, x0[:, 3] * T * 0.025, seed=M + E)
            dcfg, kcfg = _abi.stmpc_cfg(horizon=T), _abi.kmpc_cfg(horizon=min(8, T))
            ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
            kw = dict(want_planes=True, want_avoid_duals=True)
            outs = {"plain": ctx.stmpc_qp(x0, ref, dcfg), "avoid": stmpc_qp_avoid(ctx, x0, ref, obs, dcfg, **kw),
                    "walls_m0": stmpc_qp_walls(ctx, x0, ref, None, dcfg, walls=walls, **kw),
                    "walls": stmpc_qp_walls(ctx, x0, ref, obs, dcfg, walls=walls, **kw)}
            row = {"egos": E, "horizon": T}
            for name, out in outs.items():
                row[name] = _counts(out)
                if name != "plain":
                    row[name]["egos_with_an_active_row"] = int((out["avoid_duals"][:, :-1] > 1e-6).any(axis=1).sum())
                    row[name]["egos_with_eps_above_1e-6"] = int((out["eps"] > 1e-6).sum())
                    row[name]["egos_with_a_wall_row"] = int((out["planes"][:, :, :, 3] >= 16).any(axis=(1, 2)).sum())

            def plan():
                ctx.stmpc_qp_plan(x0, dcfg, kcfg, want_u=False, want_obj=False)

            def timed(name, obstacles, avoid, wall):
                stmpc_set_obstacles(ctx, obstacles)
                stmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid() if avoid else None)
                stmpc_qp_set_walls(ctx, walls if wall else None)
                ctx.stmpc_qp_warm_reset()
                row[name].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
            timed("plain", None, False, False)
            timed("avoid", obs, True, False)
            timed("walls_m0", None, False, True)
            timed("walls", obs, True, True)
            stmpc_qp_set_walls(ctx, None)
            stmpc_qp_set_avoid(ctx, None)
            stmpc_set_obstacles(ctx, None)
            if (E, T) in parent:
                pr = parent[(E, T)]
                row["parent_commit_avoid"] = {"tool": par["tool"], "note": "the parent commit's library and package, timed in the same session just before",
                                              **{k: pr["avoid"][k] for k in ("ms_median", "ms_min", "ms_max", "blocks", "status_counts", "iters_mean")},
                                              "plain_ms_median": pr["plain"]["ms_median"]}
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
