#!/usr/bin/env python3
"""Device-event timing of f1p_kmpc_qp_plan_batch with the wall rows on (f1p_kmpc_qp_set_walls) at 4096 egos x T 8, without discs
(M = 0) and with M = 4 discs per ego, beside the avoidance variant (M = 4) and the plain QP in the same process: reference extraction +
linearisation + march + QP solve + output map, one call.  The map is the synthetic track's corridor of 1.0 m half width -- narrower than the
reach of 1.5 m -- with the right half of the image cleared, so about half the egos have walls in reach and the others none.  Each figure:
`--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call, median and spread over the blocks; the interior-point
iteration counts and the status histogram come from the stateless entry points on the same first-call problem.  Prints one JSON object;
--out also writes it.  --merge-parent FILE adds, under `parent_commit_avoid`, the avoidance figure of a tools/time_kmpc_qp_avoid.py record
taken with the PARENT commit's library in the same session: the baseline the wall variant is compared with.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd._planner import qp_wall_samples  # noqa: E402
from f1tenth_planning_amd.runtime import (Context, kmpc_qp_avoid, kmpc_qp_set_avoid, kmpc_qp_set_walls, kmpc_qp_walls,  # noqa: E402
                                          kmpc_set_obstacles)
from time_kmpc_qp import _states, _time  # noqa: E402
from time_kmpc_qp_avoid import discs  # noqa: E402


def _stats(out):
    it = out["iters"][out["status"] == 0]
    return {"status_counts": {str(k): int(v) for k, v in zip(*np.unique(out["status"], return_counts=True))},
            "iters_mean": float(it.mean()), "iters_median": float(np.median(it)), "iters_max": int(it.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--discs", type=int, default=4)
    ap.add_argument("--reach", type=float, default=1.5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--merge-parent", metavar="FILE", help="a tools/time_kmpc_qp_avoid.py record of the parent commit, same session: its avoidance figure is kept beside these")
    args = ap.parse_args()
    E, T, M = args.egos, args.horizon, args.discs
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    resolution = 0.05
    img, origin = synth.make_grid(rl[:, :2], size=(900, 900), resolution=resolution, half_width=1.0)
    img = img.copy()
    img[:, img.shape[1] // 2:] = 255                             # the right half of the map: no wall anywhere
    walls = _abi.kmpc_qp_walls(n_samples=qp_wall_samples(args.reach, resolution))
    res = {"tool": "tools/time_kmpc_qp_walls.py", "egos": E, "horizon": T, "discs": M, "reach": args.reach, "n_samples": walls.n_samples,
           "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        ctx.set_grid(img, resolution, origin, 128)
        x0 = _states(rl, E, seed=E + T)
        obs = discs(x0, M, seed=M)
        cfg = _abi.kmpc_cfg(horizon=T)
        ref = ctx.kmpc_ref(x0, T)
        kw = dict(want_planes=True, want_avoid_duals=True)
        outs = {"plain": ctx.kmpc_qp(x0, ref, cfg), "avoid": kmpc_qp_avoid(ctx, x0, ref, obs, cfg, **kw),
                "walls_m0": kmpc_qp_walls(ctx, x0, ref, None, cfg, walls=walls, **kw), "walls": kmpc_qp_walls(ctx, x0, ref, obs, cfg, walls=walls, **kw)}
        for name, out in outs.items():
            res[name] = _stats(out)
            if name != "plain":
                res[name]["egos_with_an_active_row"] = int((out["avoid_duals"][:, :-1] > 1e-6).any(axis=1).sum())
                res[name]["egos_with_eps_above_1e-6"] = int((out["eps"] > 1e-6).sum())
                res[name]["egos_with_a_wall_row"] = int((out["planes"][:, :, :, 3] >= 16).any(axis=(1, 2)).sum())

        def plan():
            ctx.kmpc_qp_plan(x0, cfg, want_u=False, want_obj=False)

        def timed(name, obstacles, avoid, wall):
            kmpc_set_obstacles(ctx, obstacles)
            kmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid() if avoid else None)
            kmpc_qp_set_walls(ctx, walls if wall else None)
            ctx.kmpc_qp_warm_reset()
            res[name].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
        timed("plain", None, False, False)
        timed("avoid", obs, True, False)
        timed("walls_m0", None, False, True)
        timed("walls", obs, True, True)
        kmpc_qp_set_walls(ctx, None)
        kmpc_qp_set_avoid(ctx, None)
        kmpc_set_obstacles(ctx, None)
    if args.merge_parent:
        with open(args.merge_parent) as f:
            par = json.load(f)
        res["parent_commit_avoid"] = {"tool": par["tool"], "note": "the parent commit's library and package, timed in the same session just before",
                                      **{k: par["avoid"][k] for k in ("ms_median", "ms_min", "ms_max", "blocks", "status_counts", "iters_mean")},
                                      "plain_ms_median": par["plain"]["ms_median"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
