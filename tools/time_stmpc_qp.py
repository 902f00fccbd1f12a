#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_qp_plan_batch (STMPCPlanner.plan with the QP solver for E egos: branch split, reference extraction,
linearisation, the branch's QP solve, output map, warm start -- one call) next to the shooting solver (f1p_stmpc_shoot_dev, 512
rollouts, controls already on the device) at the same shapes: 1 ego x T 40, 1024 x T 40, 4096 x T 10, and 1024 egos half below V_KS
(a 50/50 mixed-branch batch, T 40 / TK 8).  Each figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per
call, median and spread (min, max) over the blocks.  Prints one JSON object; --out also writes it.

The kernel-only time comes from a separate run under `rocprofv3 --kernel-trace --stats` (k_stmpc_qp, k_kmpc_qp<16>, k_stmpc_ref, ...)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402
from time_kmpc_qp import _time  # noqa: E402


def _states(rl, E, seed, mixed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(rl) - 1, E)
    v = rng.uniform(2.1, 5.5, E)
    if mixed:
        v[: E // 2] = rng.uniform(0.5, 2.0, E // 2)
    return np.column_stack([rl[k, 0] + rng.normal(0, 0.2, E), rl[k, 1] + rng.normal(0, 0.2, E), rng.uniform(-0.2, 0.2, E), v,
                            rl[k, 3] + rng.normal(0, 0.2, E), rng.normal(0, 0.2, E), rng.normal(0, 0.02, E)])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rollouts", type=int, default=512, help="shooting: candidate sequences per ego")
    ap.add_argument("--out")
    args = ap.parse_args()
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    res = {"tool": "tools/time_stmpc_qp.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "shapes": []}
    R = args.rollouts
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        for E, T, mixed in ((1, 40, False), (1024, 40, False), (4096, 10, False), (1024, 40, True)):
            x0 = _states(rl, E, E + T, mixed)
            dcfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=min(8, T))
            row = {"egos": E, "horizon": T, "mixed_branches": mixed}
            ctx.stmpc_qp_warm_reset()
            probe = ctx.stmpc_qp_plan(x0, dcfg, kcfg)
            row["qp"] = _time(ctx, lambda: ctx.stmpc_qp_plan(x0, dcfg, kcfg, want_u=False, want_obj=False), args.calls, args.repeats, args.warmup)
            row["qp"]["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(probe["status"], return_counts=True))}
            row["qp"]["dynamic_egos"] = int(probe["branch"].sum())
            rng = np.random.default_rng(E)
            ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
            ctrl = np.empty((E, T, 2, R), np.float32)
            ctrl[:, :, 0, :] = np.clip(rng.normal(0, 1.0, (E, T, R)), -3.2, 3.2)
            ctrl[:, :, 1, :] = np.clip(rng.normal(0, 1.5, (E, T, R)), -3.0, 3.0)
            d_x0, d_ref, d_ctrl = ctx.to_device(x0), ctx.to_device(ref), ctx.to_device(ctrl)
            d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E))
            row["shooting"] = _time(ctx, lambda: ctx.stmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, dcfg, *d), args.calls, args.repeats, args.warmup)
            row["shooting"]["rollouts"] = R
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
