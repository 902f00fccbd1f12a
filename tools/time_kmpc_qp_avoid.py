#!/usr/bin/env python3
"""Device-event timing of f1p_kmpc_qp_plan_batch with the avoidance rows off and on (f1p_kmpc_qp_set_avoid) at 4096 egos x
T 8 x M 4 discs per ego: reference extraction + linearisation + QP solve + output map, one call.  The discs sit 1 .. 3 m ahead of each ego,
0.3 m beside its heading, so most egos carry active rows.  Each figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up,
ms per call, median and spread over the blocks; the interior-point iteration counts come from the stateless entry points on the same
first-call problem.  Prints one JSON object; --out also writes it.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context, kmpc_qp_avoid, kmpc_qp_set_avoid, kmpc_set_obstacles  # noqa: E402
from time_kmpc_qp import _states, _time  # noqa: E402


def discs(x0, M, seed):
    rng = np.random.default_rng(seed)
    E = len(x0)
    ahead = rng.uniform(1.0, 3.0, (E, M))
    side = np.where(rng.random((E, M)) < 0.5, -0.3, 0.3)
    c, s = np.cos(x0[:, 3])[:, None], np.sin(x0[:, 3])[:, None]
    v = rng.uniform(0.0, 1.5, (E, M))
    return np.stack([x0[:, :1] + ahead * c - side * s, x0[:, 1:2] + ahead * s + side * c, v * c, v * s, np.full((E, M), 0.35)], 2)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--discs", type=int, default=4)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    E, T, M = args.egos, args.horizon, args.discs
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    res = {"tool": "tools/time_kmpc_qp_avoid.py", "egos": E, "horizon": T, "discs": M, "calls": args.calls, "repeats": args.repeats,
           "warmup": args.warmup}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        x0 = _states(rl, E, seed=E + T)
        obs = discs(x0, M, seed=M)
        cfg = _abi.kmpc_cfg(horizon=T)
        ref = ctx.kmpc_ref(x0, T)
        plain = ctx.kmpc_qp(x0, ref, cfg)
        avoid = kmpc_qp_avoid(ctx, x0, ref, obs, cfg, want_avoid_duals=True)
        for name, out in (("plain", plain), ("avoid", avoid)):
            it = out["iters"][out["status"] == 0]
            res[name] = {"status_counts": {str(k): int(v) for k, v in zip(*np.unique(out["status"], return_counts=True))},
                         "iters_mean": float(it.mean()), "iters_median": float(np.median(it)), "iters_max": int(it.max())}
        res["avoid"]["egos_with_an_active_row"] = int((avoid["avoid_duals"][:, :-1] > 1e-6).any(axis=1).sum())
        res["avoid"]["egos_with_eps_above_1e-6"] = int((avoid["eps"] > 1e-6).sum())

        def plan():
            ctx.kmpc_qp_plan(x0, cfg, want_u=False, want_obj=False)
        ctx.kmpc_qp_warm_reset()
        res["plain"].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
        kmpc_set_obstacles(ctx, obs)
        kmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid())
        ctx.kmpc_qp_warm_reset()
        res["avoid"].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
        kmpc_qp_set_avoid(ctx, None)
        kmpc_set_obstacles(ctx, None)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
