#!/usr/bin/env python3
"""Device-event timing of f1p_kmpc_qp_plan_batch (reference extraction + linearisation + QP solve + output map, one call) next to the
shooting f1p_kmpc_plan_batch at the same shapes: 4096 egos x T 8, 1024 x T 30, 1 x T 8.  At T = 8 both packings of the QP kernel
(1 and 4 egos per wave) are timed.  Each figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call,
median and spread (min, max) over the blocks.  Prints one JSON object; --out also writes it.

The kernel-only time comes from a separate run under `rocprofv3 --kernel-trace --stats` (k_kmpc_qp<16|64>, k_kmpc_ref, k_kmpc_plan_gen)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402


def _states(rl, E, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(rl) - 1, E)
    return np.column_stack([rl[k, 0] + rng.normal(0, 0.2, E), rl[k, 1] + rng.normal(0, 0.2, E), rng.uniform(0.5, 5.5, E),
                            rl[k, 3] + rng.normal(0, 0.2, E)])


def _time(ctx, fn, calls, repeats, warmup):
    for _ in range(warmup):
        fn()
    ctx.sync()
    per = []
    for _ in range(repeats):
        ctx.timer_begin()
        for _ in range(calls):
            fn()
        per.append(ctx.timer_end() / calls)
    per = np.array(per)
    return dict(ms_median=float(np.median(per)), ms_min=float(per.min()), ms_max=float(per.max()), blocks=per.round(5).tolist())


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=512, help="shooting: candidate sequences per ego")
    ap.add_argument("--out")
    args = ap.parse_args()
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    res = {"tool": "tools/time_kmpc_qp.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "shapes": []}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        for E, T in ((4096, 8), (1024, 30), (1, 8)):
            x0 = _states(rl, E, seed=E + T)
            cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=args.rollouts)
            row = {"egos": E, "horizon": T}
            for pack in ((4, 1) if T <= 8 else (1,)):
                ctx.kmpc_qp_set_pack(pack)
                ctx.kmpc_qp_warm_reset()
                probe = ctx.kmpc_qp_plan(x0, cfg)
                row[f"qp_pack{pack}"] = _time(ctx, lambda: ctx.kmpc_qp_plan(x0, cfg, want_u=False, want_obj=False), args.calls, args.repeats,
                                              args.warmup)
                row[f"qp_pack{pack}"]["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(probe["status"], return_counts=True))}
            ctx.kmpc_qp_set_pack(0)
            calls = [0]

            def shoot():
                smp = _abi.kmpc_sampler(seed=1, call=calls[0])
                calls[0] += 1
                ctx.kmpc_plan(x0, cfg, smp, want_seq=False, want_cost=False)
            ctx.kmpc_warm_reset()
            row["shooting"] = _time(ctx, shoot, args.calls, args.repeats, args.warmup)
            row["shooting"]["rollouts"] = args.rollouts
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
