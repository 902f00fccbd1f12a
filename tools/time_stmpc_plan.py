#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_plan_dev (the dynamic MPC's shooting plan with the controls generated in the kernels around the
device-resident warm start) next to the streamed f1p_stmpc_shoot_dev with its controls already on the device, at the same shapes:
1024 egos x 512 rollouts x T 40, 4096 x 256 x 40, one ego x 512 x 40 (speeds 2.5-5.5 m/s, bench.py's regime) and 1024 x 512 x 40 with
speeds from 2.1 m/s (egos near the filter's trust speed, which the all-fp64 loop decides) -- and f1p_stmpc_plan_batch (host call: branch split, reference
extraction, both branches' plans, results back) on 1024 egos, all above V_KS and half of them below it (T 40 / TK 8).  Each figure:
`--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call, median and spread (min, max) over the blocks.  Prints
one JSON object; --out also writes it.

The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` (k_stmpc_filter_gen, k_stmpc_refine_tp_gen,
k_stmpc_decide_gen against k_stmpc_filter, k_stmpc_refine_tp, k_stmpc_decide)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402
from time_kmpc_qp import _time  # noqa: E402
from time_stmpc_qp import _states  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    cl = synth.make_centerline(seed=2)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    res = {"tool": "tools/time_stmpc_plan.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "shapes": [], "host_calls": []}
    c = dict(sigma_steer_v=1.0, sigma_accel=1.5, sigma_steer=0.15)
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl)
        for E, R, T, vlo in ((1024, 512, 40, 2.5), (4096, 256, 40, 2.5), (1, 512, 40, 2.5), (1024, 512, 40, 2.1)):
            x0 = _states(rl, E, E + T, False)
            x0[:, 3] = np.random.default_rng(E).uniform(vlo, 5.5, E)     # 2.5: bench.py's regime; 2.1: egos near the trust speed, decided by the all-fp64 loop
            cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
            ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
            d_x0, d_ref, d_ctrl = ctx.to_device(x0), ctx.to_device(ref), ctx.alloc(4 * E * T * 2 * R)
            d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E))
            ctx.stmpc_warm_reset()
            ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, _abi.stmpc_sampler(seed=1, call=0, **c), *d)      # a warm start to generate around
            smp = _abi.stmpc_sampler(seed=1, call=1, **c)
            ctx.stmpc_gen_controls_dev(d_ctrl, E, cfg, smp)                                            # the streamed path's resident controls: the same ones
            row = {"egos": E, "rollouts": R, "horizon": T, "v_min": vlo}
            row["streamed"] = _time(ctx, lambda: ctx.stmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, *d), args.calls, args.repeats, args.warmup)
            row["generated"] = _time(ctx, lambda: ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d), args.calls, args.repeats, args.warmup)
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
            for b in (d_x0, d_ref, d_ctrl) + d:
                b.free()
        for mixed in (False, True):
            E, R, T = 1024, 512, 40
            x0 = _states(rl, E, E + T, mixed)
            dcfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=8, n_rollouts=R)
            smp = _abi.stmpc_sampler(seed=1, call=1, **c)
            ctx.stmpc_warm_reset()
            probe = ctx.stmpc_plan(x0, dcfg, kcfg, smp)
            row = {"egos": E, "rollouts": R, "horizon": T, "horizon_kinematic": 8, "dynamic_egos": int(probe["branch"].sum())}
            row["plan_batch"] = _time(ctx, lambda: ctx.stmpc_plan(x0, dcfg, kcfg, smp, want_seq=False, want_cost=False), args.calls, args.repeats, args.warmup)
            res["host_calls"].append(row)
            print(json.dumps(row), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
