"""Shared driver code of the examples: scene set-up, the closed loop, and the lap report."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from f1tenth_planning_amd import io, sim, synth  # noqa: E402


def parser(description, steps=1500):
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--raceline", help="';'-delimited waypoint CSV (reference formats); default: seeded synthetic track")
    ap.add_argument("--envs", type=int, default=1, help="independent vehicles driven in parallel (one batched plan per step)")
    ap.add_argument("--steps", type=int, default=steps, help="simulation steps of 0.01 s")
    ap.add_argument("--start", type=float, nargs=3, metavar=("X", "Y", "THETA"), help="start pose of vehicle 0")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def raceline(args, centerline=False):
    """[N, 5] rows (x, y, v, psi, kappa) whatever the source."""
    if args.raceline:
        arr = io.load_raceline(args.raceline)
        c = io.raceline_columns(arr)
        cols = [arr[:, c[0]], arr[:, c[1]], arr[:, c[2]], arr[:, c[3]] if c[3] >= 0 else np.zeros(len(arr)),
                arr[:, c[4]] if c[4] >= 0 else np.zeros(len(arr))]
        return np.ascontiguousarray(np.column_stack(cols))
    if centerline:
        cl = synth.make_centerline(seed=2 + args.seed)
        return np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    return synth.make_raceline(seed=args.seed)


def start_poses(args, rl, avoid_heading_wrap=False):
    """Random start poses on the line.  avoid_heading_wrap: only where the heading column stays inside +-2.5 rad for the next
    stretch -- the MPCs' reference extraction inherits the reference's |.| yaw fix-up (kinematic_mpc.py:198-203), which is only
    right on one side of the +-pi seam."""
    rng = np.random.default_rng(100 + args.seed)
    ok = np.arange(len(rl) - 1)
    if avoid_heading_wrap:
        win = min(len(rl) // 3, 600)
        bad = np.abs(rl[:, 3]) > 2.5
        near_bad = np.convolve(np.concatenate([bad, bad[:win]]).astype(float), np.ones(win), mode="valid")[1:len(rl)] > 0
        if (~near_bad).any():
            ok = np.nonzero(~near_bad)[0]
    k = rng.choice(ok, args.envs)
    poses = np.column_stack([rl[k, 0] + rng.normal(0, 0.05, args.envs), rl[k, 1] + rng.normal(0, 0.05, args.envs),
                             rl[k, 3] + rng.normal(0, 0.05, args.envs)])
    if args.start:
        poses[0] = args.start
    return poses


def run(args, rl, plan, speed_scale=1.0, report_every=500, avoid_heading_wrap=False):
    """`plan(obs, env) -> actions [E, 2]` (steer, speed).  Returns the per-vehicle maximum cross-track error and progress."""
    env = sim.make("f110_gym:f110-v0", num_agents=args.envs)
    obs, _, done, _ = env.reset(start_poses(args, rl, avoid_heading_wrap))
    max_cte = np.zeros(args.envs)
    travelled = np.zeros(args.envs)
    t_plan = 0.0
    for it in range(args.steps):
        t0 = time.perf_counter()
        act = np.asarray(plan(obs, env), dtype=np.float64).reshape(args.envs, 2)
        t_plan += time.perf_counter() - t0
        act[:, 1] *= speed_scale
        obs, dt, done, _ = env.step(act)
        travelled += np.abs(obs["linear_vels_x"]) * dt
        if it % 10 == 0:
            max_cte = np.maximum(max_cte, sim.cross_track_error(np.column_stack([obs["poses_x"], obs["poses_y"]]), rl[:, :2]))
        if report_every and (it + 1) % report_every == 0:
            print(f"t = {env.current_time:6.2f} s   v0 = {obs['linear_vels_x'][0]:5.2f} m/s   max cross-track error = {max_cte.max():.3f} m")
    print(f"{args.envs} vehicle(s), {args.steps} steps: travelled {travelled.mean():.1f} m on average, "
          f"max cross-track error {max_cte.max():.3f} m, {1e3 * t_plan / args.steps:.3f} ms per batched plan() call")
    return max_cte, travelled


def obstacle_runs(args, rl, waypoints, cfg, make_planner, batch_states, set_substeps, resolution=0.05, cells=900, inflate=0.15):
    """the synthetic grid of the track + parked obstacles; one closed loop per setting of the occupancy test (mpc_config.COLLISION), the same
    start poses.  make_planner(waypoints, cfg) -> an MPC planner with set_map / plan / plan_batch; batch_states(env) -> plan_batch's states;
    set_substeps(cfg, n) sets the tested points per step"""
    from f1tenth_planning_amd import sim, synth
    if args.solver == "qp":
        raise SystemExit("--obstacles needs the shooting solver (the QP has no rollouts to test)")
    img, origin = synth.make_grid(rl[:, :2], size=(cells, cells), resolution=resolution)
    length = float(np.hypot(np.diff(rl[:, 0]), np.diff(rl[:, 1])).sum())
    img, centres = synth.stamp_obstacles(img, origin, resolution, rl, spacing=length / args.obstacles, radius=0.30)
    occupied = img[::-1] < 128                                          # [gy][gx], the uninflated map: what counts as a hit
    print(f"{len(centres)} obstacles on {length:.1f} m of track, {args.envs} vehicle(s), {args.steps} steps")
    poses = start_poses(args, rl, avoid_heading_wrap=True)
    for p in poses:                                                     # nobody starts inside or right behind an obstacle
        k = int(np.argmin(np.hypot(rl[:, 0] - p[0], rl[:, 1] - p[1])))
        while np.hypot(centres[:, 0] - rl[k, 0], centres[:, 1] - rl[k, 1]).min() < 1.5:
            k = (k + 5) % (len(rl) - 1)
            p[:] = (rl[k, 0], rl[k, 1], rl[k, 3])
    hits = {}
    for on in (False, True):
        cfg.COLLISION = on
        set_substeps(cfg, args.substeps)
        planner = make_planner([w.copy() for w in waypoints], cfg)
        planner.set_map(img, resolution, (origin[0], origin[1], 0.0), inflate=inflate)
        env = sim.make("f110_gym:f110-v0", num_agents=args.envs)
        obs, _, done, _ = env.reset(poses)
        n_hit = n_stop = 0
        for it in range(args.steps):
            if args.envs == 1:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)      # (an all-blocked plan warns and returns (0, 0): the vehicle brakes)
                    act = np.array([planner.plan(env.sim.agents[0].state)])
            else:
                out = planner.plan_batch(batch_states(env))
                act = np.column_stack([out["steer"], out["speed"]])
                n_stop += int((out["best_idx"] < 0).sum())
            obs, dt, done, _ = env.step(act)
            gx = np.floor((np.asarray(obs["poses_x"]) - origin[0]) / resolution).astype(int)
            gy = np.floor((np.asarray(obs["poses_y"]) - origin[1]) / resolution).astype(int)
            inside = (gx >= 0) & (gx < cells) & (gy >= 0) & (gy < cells)
            n_hit += int((~inside).sum() + occupied[gy[inside], gx[inside]].sum())
        hits[on] = n_hit
        print(f"occupancy test {'on ' if on else 'off'}: {n_hit} of {args.steps * args.envs} vehicle-steps ended in an occupied cell"
              + (f" ({n_stop} plans had every rollout blocked)" if on and args.envs > 1 else ""))
    return hits


def add_rival_flags(ap):
    ap.add_argument("--rivals", action="store_true", help="with --opponents M: the M opponents are found on the device from each call's states "
                    "(planner.rivals) instead of built on the host")
    ap.add_argument("--groups", type=int, default=0, help="with --rivals: split the pack into G independent races (vehicle e in race e %% G)")
    ap.add_argument("--predict", choices=("velocity", "track"), default="velocity", help="with --rivals: 'track' predicts each rival along the raceline "
                    "over the planner's horizon instead of at constant velocity (Rivals(predict='track'))")
    ap.add_argument("--rival-speed", choices=("constant", "profile"), default="constant", help="with --predict track: 'profile' moves each rival with the "
                    "raceline's speed profile, scaled by its speed now -- it brakes into the bends -- instead of at its current speed "
                    "(Rivals(predict='track', speed='profile'))")


def rival_groups(args, E):
    """-> (group id per vehicle or None, [E, E] +inf where two vehicles are not each other's business -- the diagonal, another race -- else 0)"""
    if args.groups > 0 and not args.rivals:
        raise SystemExit("--groups needs --rivals (the host construction of --opponents knows one race of all)")
    if args.predict != "velocity" and not args.rivals:
        raise SystemExit("--predict needs --rivals (the host construction of --opponents moves every opponent at constant velocity)")
    if args.rival_speed != "constant" and args.predict != "track":
        raise SystemExit("--rival-speed profile needs --predict track (the speed profile is the one of the course the rival is predicted along)")
    if args.groups <= 0:
        return None, np.diag(np.full(E, np.inf))
    groups = (np.arange(E) % args.groups).astype(np.int32)
    return groups, np.where((groups[:, None] != groups[None, :]) | np.eye(E, dtype=bool), np.inf, 0.0)


def opponent_runs(args, rl, waypoints, cfg, make_planner, batch_states, gap=1.5, radius=0.45):
    """E vehicles as a pack on one course, the fast ones behind the slow ones; one closed loop with each vehicle planning as if it were alone,
    one with its M nearest other vehicles as moving obstacles predicted at constant velocity (planner.obstacles), the same start poses.
    make_planner(waypoints, cfg) -> an MPC planner with the attribute `obstacles` and plan_batch; batch_states(env) -> plan_batch's states.
    radius: the two vehicles' radii folded into the obstacle's (a point-against-disc test).  -> the smallest distance between two vehicles
    over each run.  args.rivals: the opponents are found on the device from the call's own states (planner.rivals) instead of built here;
    with args.groups = G the pack is G independent races (vehicle e in race e % G) and distances count within a race."""
    from f1tenth_planning_amd import Rivals, sim
    E, M = args.envs, min(args.opponents, args.envs - 1, 16)
    if (args.solver == "qp" and not getattr(args, "avoid", False)) or E < 2:
        raise SystemExit("--opponents needs the shooting solver (or --solver qp --avoid) and --envs >= 2")
    groups, apart = rival_groups(args, E)
    seg = np.hypot(np.diff(rl[:, 0]), np.diff(rl[:, 1]))
    k0 = int(np.argmin(np.abs(rl[:, 3])))                                # start where the heading is far from the +-pi seam
    k = k0 + np.searchsorted(np.cumsum(np.concatenate([seg[k0:], seg[:k0]])), gap * np.arange(E))
    k %= len(rl) - 1
    poses = np.column_stack([rl[k, 0], rl[k, 1], rl[k, 3]])
    scale = np.linspace(1.0, 0.5, E)                                    # vehicle 0 is last in line and the fastest
    print(f"{E} vehicles {gap} m apart on one course, speed scales 1.0 (rear) .. 0.5 (front), {args.steps} steps, {M} opponents each")
    closest = {}
    for on in (False, True):
        planner = make_planner([w.copy() for w in waypoints], cfg)
        if on and args.rivals:
            planner.rivals = Rivals(count=M, radius=radius, groups=groups, predict=args.predict, speed=args.rival_speed)      # every plan_batch finds them itself, on the device
        env = sim.make("f110_gym:f110-v0", num_agents=E)
        env.reset(poses)
        d_min, n_stop = np.inf, 0
        for it in range(args.steps):
            st = env.state[:, [0, 1, 3, 4]]                             # (x, y, v, yaw)
            d = np.hypot(st[:, None, 0] - st[None, :, 0], st[:, None, 1] - st[None, :, 1]) + apart
            d_min = min(d_min, float(d.min()))
            obs = None
            if on and not args.rivals:
                near = np.argsort(d, axis=1)[:, :M]                     # [E, M] the nearest other vehicles
                o = st[near]
                obs = np.stack([o[:, :, 0], o[:, :, 1], o[:, :, 2] * np.cos(o[:, :, 3]), o[:, :, 2] * np.sin(o[:, :, 3]), np.full((E, M), radius)], 2)
            planner.obstacles = obs
            out = planner.plan_batch(batch_states(env))
            n_stop += int((out["best_idx"] < 0).sum()) if "best_idx" in out else 0      # (the QP solver has no rollouts to block)
            env.step(np.column_stack([out["steer"], out["speed"] * scale]))
        closest[on] = d_min
        print(f"obstacle test {'on ' if on else 'off'}: smallest distance between two vehicles {d_min:.3f} m"
              + (f" ({n_stop} plans had every rollout blocked)" if on else ""))
    return closest
