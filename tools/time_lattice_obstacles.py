#!/usr/bin/env python3
"""Device-event timing of the lattice plan with the moving discs of f1p_lattice_set_obstacles at the steady state of the headline
shape, 4096 egos x 256 candidates x 50 stations, on one box.

    python tools/time_lattice_obstacles.py --ab PARENT_TREE [--out FILE]
        (a) NO obstacles set, this tree against a checkout of the parent commit (built: PARENT_TREE/f1tenth_planning_amd/csrc/libf1p.so):
            `--alternations` (3) alternations of fresh child processes, parent then this tree, in the manner of tools/ab_plan.sh.  The acceptable
            difference is the spread of the parent's own alternations on this box.
        (b) the scene's four slots per ego (tests/lattice_obstacle_ref.py: parked on the obstacle-free winner, oncoming, empty, crossing; pace
            1 / max(v, 0.5)): the mixed schedule (f1p_lattice_set_mode 1) against the all-fp64 kernel (mode 0), ms per plan, queue entries per
            ego with and without the discs, and the share of candidates the filter's proof cannot clear (its inequality evaluated in fp64 on a
            256-ego sample of the device's own candidates: an estimate of the never_free flag's share, not a read-out of the kernel).
    python tools/time_lattice_obstacles.py --one --tree TREE     one child: the plan without obstacles with TREE's package and library, one JSON line

Each figure: `--repeats` timed blocks of `--calls` chained f1p_lattice_plan_dev calls after a warm-up, ms per call, median and spread."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E_, C_, S_ = 4096, 256, 50
M_SLOTS, MIN_SPEED, RES = 4, 0.5, 0.058


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


def _scene(synth, E):
    rl = synth.make_raceline(seed=0)
    img, origin = synth.make_grid(rl[:, :2], size=(2000, 2000), resolution=RES)
    poses = synth.make_egos(rl, E, seed=1)
    cfg = synth.bench_lattice_cfg(n_cand=C_, n_stations=S_)
    return rl, img, origin, poses, cfg


def _slots(poses, best_traj):
    """the four slots per ego of tests/lattice_obstacle_ref.make_scene, from the obstacle-free winners' rows"""
    E = poses.shape[0]
    rng = np.random.default_rng(7)
    noise = rng.normal(0.0, 0.3, (E, 2))
    x, y, th = poses[:, 0], poses[:, 1], poses[:, 2]
    ct, st = np.cos(th), np.sin(th)
    j = min(12, best_traj.shape[1] - 1)
    qx, qy = best_traj[:, j, 0], best_traj[:, j, 1]
    obs = np.zeros((E, M_SLOTS, 5))
    obs[:, 0] = np.column_stack([x + ct * qx - st * qy, y + st * qx + ct * qy, 0 * x, 0 * x, 0 * x + 0.25])
    obs[:, 1] = np.column_stack([x + 3.0 * ct + noise[:, 0], y + 3.0 * st + noise[:, 1], -2.0 * ct, -2.0 * st, 0 * x + 0.3])
    obs[:, 2] = (np.nan, np.nan, np.nan, np.nan, -1.0)
    obs[:, 3] = np.column_stack([x + 1.5 * ct + 1.5 * st, y + 1.5 * st - 1.5 * ct, -1.5 * st, 1.5 * ct, 0 * x + 0.3])
    return obs, 1.0 / np.maximum(np.abs(poses[:, 3]), MIN_SPEED)


def _buffers(ctx, E):
    return (ctx.alloc(8 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(8 * E), ctx.alloc(4 * E), ctx.alloc(4 * E), ctx.alloc(8 * E * S_ * 4))


def one(args):
    """the plan without obstacles, with the package and library of args.tree"""
    sys.path.insert(0, os.path.abspath(args.tree))
    from f1tenth_planning_amd import synth
    from f1tenth_planning_amd.runtime import Context
    rl, img, origin, poses, cfg = _scene(synth, E_)
    with Context(0) as ctx:
        ctx.set_waypoints(rl); ctx.set_grid(img, RES, origin, 206)
        d_p, b = ctx.to_device(poses), _buffers(ctx, E_)
        t = _time(ctx, lambda: ctx.lattice_plan_dev(d_p, E_, cfg, *b), args.calls, args.repeats, args.warmup)
    print(json.dumps(dict(tree=os.path.abspath(args.tree), **t)), flush=True)


def part_a(args, res):
    rows = {"parent": [], "this": []}
    for rep in range(args.alternations):
        for name, tree in (("parent", args.ab), ("this", ROOT)):
            env = dict(os.environ)
            env.pop("F1P_LIBRARY", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--tree", tree, "--calls", str(args.calls), "--repeats", str(args.repeats),
                                  "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=300, check=True).stdout
            row = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            rows[name].append(row["ms_median"])
            print(json.dumps(dict(part="a", alternation=rep, tree=name, ms_per_plan=row["ms_median"], blocks=row["blocks"])), flush=True)
    p, t = np.array(rows["parent"]), np.array(rows["this"])
    res["a"] = dict(parent_ms=p.tolist(), this_ms=t.tolist(), parent_median=float(np.median(p)), this_median=float(np.median(t)),
                    parent_spread=float(p.max() - p.min()), difference=float(np.median(t) - np.median(p)),
                    within_parent_spread=bool(abs(np.median(t) - np.median(p)) <= p.max() - p.min()))


def _not_provably_clear(poses, obs, pace, all_traj):
    """the filter's proof in fp64 on the candidates' own rows: |a| + |a - g| - 2 |u| L |pace| > L + 2 r fails for a live slot"""
    E, C = all_traj.shape[:2]
    g = all_traj[:, :, -1, :2]
    L = np.sqrt((np.diff(all_traj[:, :, :, :2], axis=2) ** 2).sum(-1)).sum(-1) * 1.001      # the polyline, rounded up: about the arc length
    ok = L > 0
    flagged = np.zeros((E, C), bool)
    ct, st = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    for m in range(obs.shape[1]):
        x, y, vx, vy, r = (obs[:, m, k] for k in range(5))
        live = r >= 0
        dx, dy = x - poses[:, 0], y - poses[:, 1]
        ax, ay = ct * dx + st * dy, ct * dy - st * dx
        nu = np.hypot(vx, vy)
        lhs = np.hypot(ax, ay)[:, None] + np.hypot(ax[:, None] - g[:, :, 0], ay[:, None] - g[:, :, 1]) - 2.0 * (nu * np.abs(pace))[:, None] * L
        with np.errstate(invalid="ignore"):
            flagged |= live[:, None] & ~(lhs > L + 2.0 * r[:, None])
    return float(flagged[ok].mean())


def part_b(args, res):
    sys.path.insert(0, ROOT)
    from f1tenth_planning_amd import synth
    from f1tenth_planning_amd.runtime import Context, lattice_set_obstacles
    rl, img, origin, poses, cfg = _scene(synth, E_)
    out = {}
    with Context(0) as ctx:
        res["device"] = ctx.device_info()
        ctx.set_waypoints(rl); ctx.set_grid(img, RES, origin, 206)
        free = ctx.lattice_plan(poses, cfg)
        out["queue_entries_per_ego_without_discs"] = float(ctx.lattice_debug_queue(E_).mean())
        obs, pace = _slots(poses, free["best_traj"])
        n = 256
        sample = ctx.lattice_plan(poses[:n], cfg, want_all=True)
        out["share_not_provably_clear_fp64_estimate"] = _not_provably_clear(poses[:n], obs[:n], pace[:n], sample["all_traj"])
        lattice_set_obstacles(ctx, obs, pace)
        with_discs = ctx.lattice_plan(poses, cfg)
        out["queue_entries_per_ego"] = float(ctx.lattice_debug_queue(E_).mean())
        out["share_winners_changed"] = float((with_discs["best_idx"] != free["best_idx"]).mean())
        out["share_all_blocked"] = float((with_discs["status"] == 3).mean())
        d_p, b = ctx.to_device(poses), _buffers(ctx, E_)
        for mode, name in ((1, "mixed"), (0, "all_fp64")):
            ctx.lattice_set_mode(mode)
            out[name] = _time(ctx, lambda: ctx.lattice_plan_dev(d_p, E_, cfg, *b), args.calls, args.repeats, args.warmup)
        ctx.lattice_set_mode(1)
        ctx.lattice_profile(True)
        acc = np.zeros(4)
        for _ in range(args.calls):
            ctx.lattice_plan_dev(d_p, E_, cfg, *b)
            acc += np.array(ctx.lattice_profile(True, read=True))
        ctx.lattice_profile(False)
        out["mixed_kernel_us"] = dict(zip(("prologue", "filter3", "refine", "select"), (1e3 * acc / args.calls).round(2).tolist()))
        lattice_set_obstacles(ctx, None)
        out["mixed_without_discs"] = _time(ctx, lambda: ctx.lattice_plan_dev(d_p, E_, cfg, *b), args.calls, args.repeats, args.warmup)
    out["mixed_over_all_fp64"] = out["mixed"]["ms_median"] / out["all_fp64"]["ms_median"]
    res["b"] = out
    print(json.dumps(dict(part="b", **out)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--ab", metavar="PARENT_TREE", help="part (a): a built checkout of the parent commit")
    ap.add_argument("--one", action="store_true", help="child process of part (a)")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.one:
        return one(args)
    res = {"tool": "tools/time_lattice_obstacles.py", "shape": [E_, C_, S_], "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup}
    if args.ab:                             # (first: this process has not touched the GPU yet when it starts the children)
        part_a(args, res)
    if not args.skip_b:
        part_b(args, res)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
