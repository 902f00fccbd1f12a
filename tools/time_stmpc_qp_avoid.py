#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_qp_plan_batch with the avoidance rows off and on (f1p_stmpc_qp_set_avoid), in the same run
of the same tree, at 1 ego x T 40, 1024 x T 40 and 4096 x T 10, M = 4 discs per ego: branch split, reference extraction, linearisation, the
QP solve, output map, warm start -- one call.  Every ego is above V_KS (the dynamic branch); the discs sit 0.3 .. 1.0 horizon lengths ahead
of each ego, 0.35 m beside its heading, so that many egos carry active rows without being squeezed.  Each figure: `--repeats` timed blocks
of `--calls` chained calls after a warm-up, ms per call, median and spread over the blocks; the interior-point iteration counts come from
the stateless entry points on the same first-call problem.  Prints one JSON object; --out also writes it.  A record, not a gate."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context, stmpc_qp_avoid, stmpc_qp_set_avoid, stmpc_set_obstacles  # noqa: E402
from time_kmpc_qp import _time  # noqa: E402
from time_stmpc_qp import _states  # noqa: E402


def discs(x0, M, reach, seed):
    rng = np.random.default_rng(seed)
    E = len(x0)
    ahead = rng.uniform(0.3, 1.0, (E, M)) * reach[:, None]
    side = np.where(rng.random((E, M)) < 0.5, -0.35, 0.35)
    hd = x0[:, 4] + x0[:, 6]
    c, s = np.cos(hd)[:, None], np.sin(hd)[:, None]
    v = rng.uniform(0.0, 1.0, (E, M))
    return np.stack([x0[:, :1] + ahead * c - side * s, x0[:, 1:2] + ahead * s + side * c, v * c, v * s, np.full((E, M), 0.30)], 2)


def _counts(out):
    it = out["iters"][out["status"] == 0]
    return {"status_counts": {str(k): int(v) for k, v in zip(*np.unique(out["status"], return_counts=True))},
            "iters_mean": float(it.mean()), "iters_median": float(np.median(it)), "iters_max": int(it.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--discs", type=int, default=4)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    M = args.discs
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    res = {"tool": "tools/time_stmpc_qp_avoid.py", "discs": M, "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "shapes": []}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        for E, T in ((1, 40), (1024, 40), (4096, 10)):
            x0 = _states(rl, E, E + T, False)
            obs = discs(x0, M, x0[:, 3] * T * 0.025, seed=M + E)
            dcfg, kcfg = _abi.stmpc_cfg(horizon=T), _abi.kmpc_cfg(horizon=min(8, T))
            ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
            plain = ctx.stmpc_qp(x0, ref, dcfg)
            avoid = stmpc_qp_avoid(ctx, x0, ref, obs, dcfg, want_avoid_duals=True)
            row = {"egos": E, "horizon": T, "plain": _counts(plain), "avoid": _counts(avoid)}
            row["avoid"]["egos_with_an_active_row"] = int((avoid["avoid_duals"][:, :-1] > 1e-6).any(axis=1).sum())
            row["avoid"]["egos_with_eps_above_1e-6"] = int((avoid["eps"] > 1e-6).sum())

            def plan():
                ctx.stmpc_qp_plan(x0, dcfg, kcfg, want_u=False, want_obj=False)
            ctx.stmpc_qp_warm_reset()
            row["plain"].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
            stmpc_set_obstacles(ctx, obs)
            stmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid())
            ctx.stmpc_qp_warm_reset()
            row["avoid"].update(_time(ctx, plan, args.calls, args.repeats, args.warmup))
            stmpc_qp_set_avoid(ctx, None)
            stmpc_set_obstacles(ctx, None)
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
