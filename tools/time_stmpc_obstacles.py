#!/usr/bin/env python3
"""Device-event timing of f1p_stmpc_plan_dev with the moving obstacles of f1p_stmpc_set_obstacles: per shape (1024 egos x
512 rollouts x T 40 and x T 12) and n_sub (1 and 4), all rows from this one process:
    off          the test off (k_stmpc_filter_gen -> refine -> decide, the yardstick)
    grid open    the occupancy test in open space (the _gen_col kernels on scene B's grid)
    obs empty    obstacles set, every slot empty, no grid (the _gen_obs kernels doing the _col kernels' work minus the map reads)
    traffic 4    scene "traffic" of tests/stmpc_obstacle_ref.py, M = 4
    crowd16      M = 16, every slot live: traffic's discs and bystanders (crowd16)
Each figure: `--repeats` timed blocks of `--calls` chained calls after a warm-up, ms per call, median and spread (min, max) over the
blocks; next to it the mean size of the refined set over the egos that were refined and the shares of egos decided entirely in fp64
(n_refined -1) and of all-blocked egos, from one more call with the d_n_refined hook.
THE BAR: "obs empty" may not exceed "grid open" of the same shape and n_sub by more than 5 % (medians); exit status 1 when it does.
Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stmpc_obstacle_ref as O  # noqa: E402
from f1tenth_planning_amd import _abi  # noqa: E402
from f1tenth_planning_amd.runtime import Context, stmpc_set_obstacles  # noqa: E402
from time_kmpc_qp import _time  # noqa: E402

BAR = 1.05
ROWS = ("off", "grid open", "obs empty", "traffic 4", "crowd16")


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
    res = {"tool": "tools/time_stmpc_obstacles.py", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "bar": BAR,
           "rows": [], "bar_rows": []}
    ok = True
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        s = O.S.scene_b(E)                                              # scene D's egos on an all-free image
        img, r_, ox, oy, occ = s["grid"]
        ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
        for T in args.horizons:
            cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
            smp = _abi.stmpc_sampler(seed=1, call=1, use_warm=True, **O.SIG)
            empty = np.empty((E, 4, 5)); empty[:] = O.EMPTY
            obstacles = {"obs empty": empty, "traffic 4": O.traffic(s["x0"], T, M=4), "crowd16": O.crowd16(s["x0"], T)}
            d_x0, d_ref = ctx.to_device(s["x0"]), ctx.to_device(ctx.stmpc_ref(O.xy4(s["x0"]), T))
            d = (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E))
            d_nref = ctx.alloc(4 * E)
            for n_sub in (1, 4):
                med = {}
                for name in ROWS:
                    grid = name == "grid open"
                    if grid:
                        ctx.set_grid(img, r_, (ox, oy), occ)
                    else:
                        ctx.set_grid(None, 0, (0, 0), 0)
                    ctx.stmpc_set_collision(grid, n_sub)
                    stmpc_set_obstacles(ctx, obstacles.get(name))
                    ctx.stmpc_warm_set(O.warm_start(E, T), np.full(E, 2), T)
                    d_nref.upload(np.full(E, -1, np.int32))
                    ctx.stmpc_set_mode(True, None, d_nref)
                    ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d)
                    ctx.sync()
                    n, bi = d_nref.download(np.int32, (E,)), d[2].download(np.int32, (E,))
                    ctx.stmpc_set_mode(True)
                    row = {"egos": E, "rollouts": R, "horizon": T, "row": name, "n_sub": n_sub,
                           "mean_n_refined": float(n[n > 0].mean()) if (n > 0).any() else 0.0, "share_all_fp64": float((n == -1).mean()),
                           "share_all_blocked": float((bi == -1).mean())}
                    row["plan_dev"] = _time(ctx, lambda: ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, *d), args.calls, args.repeats, args.warmup)
                    med[name] = row["plan_dev"]["ms_median"]
                    row["ratio_to_off"] = med[name] / med["off"]
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                bar = {"horizon": T, "n_sub": n_sub, "obs_empty_over_grid_open": med["obs empty"] / med["grid open"]}
                bar["ok"] = bar["obs_empty_over_grid_open"] <= BAR
                ok &= bar["ok"]
                res["bar_rows"].append(bar)
                print(json.dumps(bar), flush=True)
            stmpc_set_obstacles(ctx, None)
            ctx.stmpc_set_collision(False)
            for b in (d_x0, d_ref, d_nref) + d:
                b.free()
    res["bar_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
