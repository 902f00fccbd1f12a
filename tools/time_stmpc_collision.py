#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_plan_dev with the occupancy test of f1p_stmpc_set_collision: per shape (1024 egos x 512 rollouts x T 40
and x T 12) and scene of tests/stmpc_collision_ref.py (B open space, D parked obstacles, the narrow corridor) the test off (the yardstick
of the same process), then on at n_sub 1 and 4, each in the mixed mode (filter -> refinement -> decision) and in plain fp64
(f1p_stmpc_set_mode(0): k_stmpc_shoot_gen / k_stmpc_shoot_gen_col).  Each figure: `--repeats` timed blocks of `--calls` chained calls after
a warm-up, ms per call, median and spread (min, max) over the blocks; next to it the mean size of the refined set over the egos that were
refined and the share of egos decided entirely in fp64 (n_refined -1) and of all-blocked egos, from one more mixed call with the d_n_refined
hook.  Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stmpc_collision_ref as S  # noqa: E402
from f1tenth_planning_amd import _abi  # noqa: E402
from f1tenth_planning_amd.runtime import Context  # noqa: E402
from time_kmpc_qp import _time  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--egos", type=int, default=1024)
    ap.add_argument("--rollouts", type=int, default=512)
    ap.add_argument("--horizons", type=int, nargs="+", default=[40, 12])
    ap.add_argument("--out")
    args = ap.parse_args()
    E, R = args.egos, args.rollouts
    res = {"tool": "tools/time_stmpc_collision.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        for T in args.horizons:
            cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
            smp = _abi.stmpc_sampler(seed=1, call=1, use_warm=True, **S.SIG)
            for name, make in (("B open space", S.scene_b), ("D obstacles", S.scene_d), ("corridor", S.scene_corridor)):
                s = make(E)
                img, r_, ox, oy, occ = s["grid"]
                ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
                ctx.set_grid(img, r_, (ox, oy), occ)
                d_x0, d_ref = ctx.to_device(s["x0"]), ctx.to_device(ctx.stmpc_ref(s["x0"][:, [0, 1, 3, 4]], T))
                d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E))
                d_nref = ctx.alloc(4 * E)
                for n_sub in (0, 1, 4):                                  # 0: the test off
                    ctx.stmpc_set_collision(n_sub > 0, max(n_sub, 1))
                    ctx.stmpc_warm_set(S.warm_start(E, T), np.full(E, 2), T)
                    d_nref.upload(np.full(E, -1, np.int32))
                    ctx.stmpc_set_mode(True, None, d_nref)
                    ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d)
                    ctx.sync()
                    n, bi = d_nref.download(np.int32, (E,)), d[2].download(np.int32, (E,))
                    row = {"egos": E, "rollouts": R, "horizon": T, "scene": name, "n_sub": n_sub,
                           "mean_n_refined": float(n[n > 0].mean()) if (n > 0).any() else 0.0, "share_all_fp64": float((n == -1).mean()),
                           "share_all_blocked": float((bi == -1).mean())}
                    for mode, mixed in (("mixed", True), ("fp64", False)):
                        ctx.stmpc_set_mode(mixed)
                        row[mode] = _time(ctx, lambda: ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d), args.calls, args.repeats, args.warmup)
                    ctx.stmpc_set_mode(True)
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                ctx.stmpc_set_collision(False)
                for b in (d_x0, d_ref, d_nref) + d:
                    b.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
