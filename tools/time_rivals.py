#!/usr/bin/env python3
"""What it costs to make the vehicles of a batch each other's obstacles, E = 4096 egos, M = 4, as one race of all and as 512
races of 8, all rows from this one process:
    device   state upload + f1p_rivals_dev + f1p_kmpc_set_obstacles_dev        (what planner.rivals does per plan)
    host     the numpy construction of examples/common.py opponent_runs (distance matrix, argsort, gather, trig, stack; for the races a
             +inf mask between different groups) + f1p_kmpc_set_obstacles      (what a user had to do before)
    kernel   k_rivals alone, device events around `--calls` chained launches
device and host: a host clock around the work and a final synchronise, the two ALTERNATED block by block after a warm-up, `--repeats` blocks
of `--dev-calls` / `--host-calls` calls, ms per call, median and spread (min, max) over the blocks.  The two paths' slots are compared first
(same vehicles; vx, vy to 1e-12).  THE EXPECTATION: device faster than host by more than the host path's own block-to-block spread, in both
shapes; "expected" in the record says whether it held.  Prints one JSON object; --out also writes it.

--predict: the rivals predicted along the raceline, same shapes, same protocol, the vehicles on a synthetic raceline:
    predict  state upload + f1p_rivals_predict_dev + f1p_kmpc_set_obstacles_dev  (what Rivals(predict="track") does per plan)
    device   the constant-velocity path above, same run
    parent   (--parent-lib PATH: libf1p.so of the parent commit) the constant-velocity path through THAT library, on a context of its own
    kernels  device events around chained launches: k_rivals alone, and k_rivals + k_rivals_frenet + k_rivals_predict; "new_kernels_ms" is the difference
The paths are ALTERNATED block by block.  Compared first: the constant-velocity slots of both libraries bit for bit, and idx, x, y of the predicted
slots against them.  THE EXPECTATION: the constant-velocity path's median stays inside the parent's own block-to-block band (its kernel is unchanged,
only the launch path gained a branch).  The prediction's own cost is reported, not judged.

--predict --speed profile: the rivals predicted with the raceline's speed profile beside the constant-speed prediction, same process, same
shapes, same protocol -- the paths "profile", "predict" and "device" ALTERNATED block by block, the kernels' row "kernel_profile" (k_rivals + k_rivals_frenet
+ k_rivals_predict<CourseTime>; the time table is built once, before the clock) next to "kernel_predict".  Compared first: idx, x, y, pace of the profile
slots against the constant-speed ones, bit for bit.  Reported, not judged: "profile_ms" = profile - predict medians, "profile_kernels_ms" likewise."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from f1tenth_planning_amd import _abi, synth  # noqa: E402
from f1tenth_planning_amd.runtime import (Context, kmpc_set_obstacles, kmpc_set_obstacles_dev, rivals_dev, rivals_predict_dev,  # noqa: E402
                                          rivals_set_groups)
from time_kmpc_qp import _time  # noqa: E402

RADIUS = 0.45


def host_obstacles(st, M, groups):
    """examples/common.py:153-160, with the races kept apart by a +inf mask"""
    E = st.shape[0]
    d = np.hypot(st[:, None, 0] - st[None, :, 0], st[:, None, 1] - st[None, :, 1]) + np.diag(np.full(E, np.inf))
    if groups is not None:
        d = d + np.where(groups[:, None] != groups[None, :], np.inf, 0.0)
    near = np.argsort(d, axis=1)[:, :M]
    o = st[near]
    return np.stack([o[:, :, 0], o[:, :, 1], o[:, :, 2] * np.cos(o[:, :, 3]), o[:, :, 2] * np.sin(o[:, :, 3]), np.full((E, M), RADIUS)], 2), near


def _blocks(per):
    per = np.array(per)
    return dict(ms_median=float(np.median(per)), ms_min=float(per.min()), ms_max=float(per.max()), blocks=per.round(5).tolist())


def other_library_context(path):
    """a Context on another build of the library (the parent commit's: it exports fewer symbols)"""
    lib = C.CDLL(path, mode=os.RTLD_NOW | os.RTLD_LOCAL | getattr(os, "RTLD_DEEPBIND", 0))
    for name, (res, args) in _abi.PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    mine, _abi._lib = _abi.load_library(), lib
    try:
        return Context(0)
    finally:
        _abi._lib = mine


def predict_main(args):
    E, M, H, K = args.egos, args.slots, 0.8, 8
    rng = np.random.default_rng(0)
    rl = synth.make_raceline(seed=0)
    res = {"tool": "tools/time_rivals.py --predict" + (" --speed profile" if args.speed == "profile" else ""), "egos": E, "slots": M, "horizon_s": H, "knots": K, "raceline_points": int(rl.shape[0]),
           "repeats": args.repeats, "dev_calls": args.dev_calls, "kernel_calls": args.calls, "parent_lib": bool(args.parent_lib), "rows": []}
    ok = True
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctxs = [ctx] + ([other_library_context(args.parent_lib)] if args.parent_lib else [])
        bufs = [(c.alloc(32 * E), c.alloc(40 * E * M), c.alloc(4 * E * M)) for c in ctxs]
        for c in ctxs:
            c.set_waypoints(rl)
        for name, groups in (("one race", None), (f"{E // args.race} races of {args.race}", (np.arange(E) % (E // args.race)).astype(np.int32))):
            k = rng.integers(0, rl.shape[0] - 1, E)                 # on the raceline, up to 0.4 m to either side, roughly along it
            lat = rng.uniform(-0.4, 0.4, E)
            st = np.column_stack([rl[k, 0] - lat * np.sin(rl[k, 3]), rl[k, 1] + lat * np.cos(rl[k, 3]), rng.uniform(0.5, 6.0, E),
                                  rl[k, 3] + rng.uniform(-0.2, 0.2, E)])
            for c in ctxs:
                rivals_set_groups(c, groups)

            def velocity(c, b):
                b[0].upload(st)
                rivals_dev(c, b[0], "xyvyaw", E, M, RADIUS, b[1])
                kmpc_set_obstacles_dev(c, b[1], E, M)
                c.sync()

            def predict():
                d_st, d_obs, _ = bufs[0]
                d_st.upload(st)
                rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K)
                kmpc_set_obstacles_dev(ctx, d_obs, E, M)
                ctx.sync()

            def profile():
                d_st, d_obs, _ = bufs[0]
                d_st.upload(st)
                rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K, speed="profile")
                kmpc_set_obstacles_dev(ctx, d_obs, E, M)
                ctx.sync()

            outs = []
            for c, b in zip(ctxs, bufs):
                rivals_dev(c, b[0].upload(st), "xyvyaw", E, M, RADIUS, b[1], None, b[2])
                outs.append((b[1].download(np.float64, (E, M, 5)), b[2].download(np.int32, (E, M))))
            d_st, d_obs, d_idx = bufs[0]
            rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K, d_idx=d_idx)
            pobs, pidx = d_obs.download(np.float64, (E, M, 5)), d_idx.download(np.int32, (E, M))
            same = bool(all(o.tobytes() == outs[0][0].tobytes() and i.tobytes() == outs[0][1].tobytes() for o, i in outs)
                        and (pidx == outs[0][1]).all() and pobs[..., :2].tobytes() == outs[0][0][..., :2].tobytes())
            moved = float((np.abs(pobs[..., 2:4] - outs[0][0][..., 2:4]).max(axis=2)[pidx >= 0] > 0.05).mean())
            if args.speed == "profile":
                rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K, d_idx=d_idx, speed="profile")
                qobs, qidx = d_obs.download(np.float64, (E, M, 5)), d_idx.download(np.int32, (E, M))
                same = bool(same and (qidx == pidx).all() and qobs[..., :2].tobytes() == pobs[..., :2].tobytes() and np.isfinite(qobs).all())
                moved_profile = float((np.abs(qobs[..., 2:4] - pobs[..., 2:4]).max(axis=2)[pidx >= 0] > 0.05).mean())
            paths = ([("profile", profile)] if args.speed == "profile" else []) + [("predict", predict), ("device", lambda: velocity(ctx, bufs[0]))] + ([("parent", lambda: velocity(ctxs[1], bufs[1]))] if args.parent_lib else [])
            for _, fn in paths * 2:                                  # warm-up of every path
                fn()
            per = {key: [] for key, _ in paths}
            for _ in range(args.repeats):
                for key, fn in paths:
                    t0 = time.perf_counter()
                    for _ in range(args.dev_calls):
                        fn()
                    per[key].append(1e3 * (time.perf_counter() - t0) / args.dev_calls)
            row = {"shape": name, "same_slots": same, "slots_moved_by_prediction": moved}
            row.update({key: _blocks(v) for key, v in per.items()})
            row["kernel_velocity"] = _time(ctx, lambda: rivals_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs), args.calls, args.repeats, 3)
            row["kernel_predict"] = _time(ctx, lambda: rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K), args.calls, args.repeats, 3)
            row["new_kernels_ms"] = row["kernel_predict"]["ms_median"] - row["kernel_velocity"]["ms_median"]
            row["prediction_ms"] = row["predict"]["ms_median"] - row["device"]["ms_median"]
            if args.speed == "profile":
                row["slots_moved_by_profile"] = moved_profile
                row["kernel_profile"] = _time(ctx, lambda: rivals_predict_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs, H, 0.0, K, speed="profile"), args.calls,
                                              args.repeats, 3)
                row["profile_kernels_ms"] = row["kernel_profile"]["ms_median"] - row["kernel_predict"]["ms_median"]
                row["profile_ms"] = row["profile"]["ms_median"] - row["predict"]["ms_median"]
            row["expected"] = same
            if args.parent_lib:
                row["expected"] = bool(same and row["device"]["ms_median"] <= row["parent"]["ms_max"])
            ok &= row["expected"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            for c in ctxs:
                kmpc_set_obstacles_dev(c, None)
                rivals_set_groups(c, None)
        for c, b in zip(ctxs, bufs):
            for x in b:
                x.free()
        for c in ctxs[1:]:
            c.close()
    res["expected"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--egos", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--race", type=int, default=8, help="vehicles per race of the grouped shape")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dev-calls", type=int, default=50)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--calls", type=int, default=50, help="chained launches per block of the kernel-only row")
    ap.add_argument("--out")
    ap.add_argument("--predict", action="store_true", help="time the prediction along the raceline (DESIGN.md 5n) instead")
    ap.add_argument("--speed", choices=("constant", "profile"), default="constant", help="--predict: 'profile' also times the prediction with the raceline's "
                    "speed profile (DESIGN.md 5u), alternated with the constant-speed one")
    ap.add_argument("--parent-lib", help="--predict: libf1p.so of the parent commit, its constant-velocity path alternated with this tree's")
    args = ap.parse_args()
    if args.speed != "constant" and not args.predict:
        ap.error("--speed profile needs --predict")
    if args.predict:
        predict_main(args)
    E, M = args.egos, args.slots
    rng = np.random.default_rng(0)
    res = {"tool": "tools/time_rivals.py", "egos": E, "slots": M, "repeats": args.repeats, "dev_calls": args.dev_calls, "host_calls": args.host_calls,
           "kernel_calls": args.calls, "rows": []}
    ok = True
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        d_st, d_obs, d_idx = ctx.alloc(32 * E), ctx.alloc(40 * E * M), ctx.alloc(4 * E * M)
        for name, groups in (("one race", None), (f"{E // args.race} races of {args.race}", (np.arange(E) % (E // args.race)).astype(np.int32))):
            # one race: a field of 100 m x 100 m; the races: every race a pack of its own 20 m x 20 m, the packs on top of each other
            side = 100.0 if groups is None else 20.0
            st = np.column_stack([rng.uniform(0.0, side, (E, 2)), rng.uniform(0.5, 6.0, E), rng.uniform(-3.0, 3.0, E)])
            rivals_set_groups(ctx, groups)

            def device():
                d_st.upload(st)
                rivals_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs)
                kmpc_set_obstacles_dev(ctx, d_obs, E, M)
                ctx.sync()

            def host():
                kmpc_set_obstacles(ctx, host_obstacles(st, M, groups)[0])
                ctx.sync()

            # the same slots both ways
            want, near = host_obstacles(st, M, groups)
            rivals_dev(ctx, d_st.upload(st), "xyvyaw", E, M, RADIUS, d_obs, None, d_idx)
            got, idx = d_obs.download(np.float64, (E, M, 5)), d_idx.download(np.int32, (E, M))
            same = bool((idx == near).all() and np.abs(got - want).max() <= 1e-12 * 6.0)
            device(); host(); device()                                              # warm-up of both
            per = {"device": [], "host": []}
            for _ in range(args.repeats):
                for key, fn, n in (("device", device, args.dev_calls), ("host", host, args.host_calls)):
                    t0 = time.perf_counter()
                    for _ in range(n):
                        fn()
                    per[key].append(1e3 * (time.perf_counter() - t0) / n)
            row = {"shape": name, "same_slots": same, "device": _blocks(per["device"]), "host": _blocks(per["host"]),
                   "kernel": _time(ctx, lambda: rivals_dev(ctx, d_st, "xyvyaw", E, M, RADIUS, d_obs), args.calls, args.repeats, 3)}
            row["host_over_device"] = row["host"]["ms_median"] / row["device"]["ms_median"]
            row["expected"] = bool(same and row["device"]["ms_median"] < row["host"]["ms_median"] - (row["host"]["ms_max"] - row["host"]["ms_min"]))
            ok &= row["expected"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            kmpc_set_obstacles_dev(ctx, None)
        rivals_set_groups(ctx, None)
        for b in (d_st, d_obs, d_idx):
            b.free()
    res["expected"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
