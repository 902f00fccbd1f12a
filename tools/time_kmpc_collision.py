#!/usr/bin/env python3
"""Device-event timing of f1p_kmpc_plan_dev with the occupancy test of f1p_kmpc_set_collision: per shape (1024 egos x 512 rollouts x T 30
and x T 8) the test off (k_kmpc_plan_gen, the yardstick of the same process), then on at n_sub 1 and 4 (k_kmpc_plan_gen_col) in open space
(scene B), on the track with parked obstacles (scene A) and in the narrow corridor -- the scenes of tests/kmpc_collision_ref.py.  Each
figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call, median and spread (min, max) over the blocks;
next to it the mean size of the refined set over the egos that were refined and the share of egos decided entirely in fp64 (n_refined -1)
and of all-blocked egos, from one more call with the d_n_refined hook.  Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmpc_collision_ref as K  # noqa: E402
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
    ap.add_argument("--cells", type=int, default=2000, help="the occupancy image is cells x cells (2000 x 0.02 m: a 504 KB bitmap)")
    ap.add_argument("--out")
    args = ap.parse_args()
    E, R = args.egos, args.rollouts
    res_m = 40.0 / args.cells
    res = {"tool": "tools/time_kmpc_collision.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "cells": args.cells,
           "resolution": res_m, "rows": []}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        for T in (30, 8):
            cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
            smp = _abi.kmpc_sampler(seed=1, call=1, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
            for name, make in (("B open space", K.scene_b), ("A obstacles", K.scene_a), ("corridor", K.scene_corridor)):
                s = make(E, T, size=args.cells, res=res_m)
                img, r_, ox, oy, occ = s["grid"]
                ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
                ctx.set_grid(img, r_, (ox, oy), occ)
                d_x0, d_ref = ctx.to_device(s["x0"]), ctx.to_device(ctx.kmpc_ref(s["x0"], T))
                d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E))
                d_nref = ctx.alloc(4 * E)
                for n_sub in (0, 1, 4):                                  # 0: the test off
                    ctx.kmpc_set_collision(n_sub > 0, max(n_sub, 1))
                    ctx.kmpc_warm_set(K.warm_start(E, T))
                    ctx.kmpc_set_mode(True, None, d_nref)
                    ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d)
                    ctx.sync()
                    n, bi = d_nref.download(np.int32, (E,)), d[2].download(np.int32, (E,))
                    ctx.kmpc_set_mode(True)
                    row = {"egos": E, "rollouts": R, "horizon": T, "scene": name, "n_sub": n_sub,
                           "mean_n_refined": float(n[n > 0].mean()) if (n > 0).any() else 0.0, "share_all_fp64": float((n == -1).mean()),
                           "share_all_blocked": float((bi == -1).mean())}
                    row["plan_dev"] = _time(ctx, lambda: ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d), args.calls, args.repeats, args.warmup)
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                ctx.kmpc_set_collision(False)
                for b in (d_x0, d_ref, d_nref) + d:
                    b.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
