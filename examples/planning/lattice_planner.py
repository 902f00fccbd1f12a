"""Lattice planner in closed loop: device-sampled goal grid -> clothoids -> occupancy check -> cost -> argmin -> pure
pursuit on the winner (the flow LatticePlanner.plan intends, planning/lattice_planner/lattice_planner.py:174-214).

--opponents M (with --envs E >= 2) starts the E vehicles as a pack on one course, the fast ones behind the slow ones, and drives the loop twice:
each vehicle planning as if it were alone, then with its M nearest other vehicles as moving discs of its candidates (LatticePlanner.obstacles,
predicted at constant velocity; f1p_lattice_set_obstacles) -- and prints the smallest distance between two vehicles over each run.  With --rivals
the opponents are not built here but found on the device by every plan (LatticePlanner.rivals = Rivals(count=M, radius=...)); --groups G then
splits the pack into G independent races.  --predict track predicts each rival along the raceline over the planner's
horizon instead of at constant velocity (Rivals(predict="track")); --rival-speed profile then moves it with the raceline's speed profile instead of at
its current speed (Rivals(predict="track", speed="profile"))."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import common  # noqa: E402

from f1tenth_planning.planning.lattice_planner.lattice_planner import LatticePlanner  # noqa: E402
from f1tenth_planning_amd import synth  # noqa: E402


def make_planner(args, waypoints):
    planner = LatticePlanner(waypoints=waypoints)
    planner.configure(lookahead_distances=np.linspace(0.8, 2.4, 8), widths=np.linspace(-0.6, 0.6, 9), num_stations=50,
                      generator=args.generator)
    img, origin = synth.make_grid(waypoints[:, :2], size=(2000, 2000), resolution=0.058)
    planner.set_map(img, 0.058, origin, occupied_thresh=0.2)
    return planner


def opponent_runs(args, waypoints, gap=1.5, radius=0.45):
    """E vehicles as a pack on one course (examples/common.py opponent_runs, for the lattice planner): radius folds both vehicles' radii into the disc's"""
    from f1tenth_planning_amd import Rivals, sim
    E, M = args.envs, min(args.opponents, args.envs - 1, 16)
    if E < 2:
        raise SystemExit("--opponents needs --envs >= 2")
    groups, apart = common.rival_groups(args, E)
    seg = np.hypot(np.diff(waypoints[:, 0]), np.diff(waypoints[:, 1]))
    k0 = int(np.argmin(np.abs(waypoints[:, 3])))
    k = (k0 + np.searchsorted(np.cumsum(np.concatenate([seg[k0:], seg[:k0]])), gap * np.arange(E))) % (len(waypoints) - 1)
    poses0 = np.column_stack([waypoints[k, 0], waypoints[k, 1], waypoints[k, 3]])
    scale = 0.6 * np.linspace(1.0, 0.5, E)                             # vehicle 0 is last in line and the fastest
    print(f"{E} vehicles {gap} m apart on one course, {args.steps} steps, {M} opponents each")
    closest = {}
    for on in (False, True):
        planner = make_planner(args, waypoints)
        if on and args.rivals:
            planner.rivals = Rivals(count=M, radius=radius, groups=groups, predict=args.predict, speed=args.rival_speed)     # every plan_batch finds them itself, on the device
        env = sim.make("f110_gym:f110-v0", num_agents=E)
        env.reset(poses0)
        d_min, n_stop = np.inf, 0
        for it in range(args.steps):
            st = env.state[:, [0, 1, 3, 4]]                            # (x, y, v, yaw)
            d = np.hypot(st[:, None, 0] - st[None, :, 0], st[:, None, 1] - st[None, :, 1]) + apart
            d_min = min(d_min, float(d.min()))
            if on and not args.rivals:
                o = st[np.argsort(d, axis=1)[:, :M]]                   # [E, M] the nearest other vehicles
                planner.obstacles = np.stack([o[:, :, 0], o[:, :, 1], o[:, :, 2] * np.cos(o[:, :, 3]), o[:, :, 2] * np.sin(o[:, :, 3]), np.full((E, M), radius)], 2)
            out = planner.plan_batch(np.column_stack([st[:, 0], st[:, 1], st[:, 3], st[:, 2]]), want_traj=False)
            n_stop += int((out["status"] == 3).sum())
            env.step(np.column_stack([out["steer"], out["speed"] * scale]))
        closest[on] = d_min
        print(f"obstacle test {'on ' if on else 'off'}: smallest distance between two vehicles {d_min:.3f} m"
              + (f" ({n_stop} plans had every candidate blocked)" if on else ""))
    return closest


def main():
    ap = common.parser(__doc__, steps=1000)
    ap.add_argument("--map", help="ROS map_server yaml (e.g. Spielberg_map.yaml); default: synthetic corridor around the track")
    ap.add_argument("--generator", choices=["clothoid", "cubic"], default="clothoid")
    ap.add_argument("--tracks", type=int, default=0, help="N agents on N lanes offset sideways from the raceline, one track set")
    ap.add_argument("--opponents", type=int, default=0, help="with --envs E: each vehicle's M nearest other vehicles are moving obstacles of its candidates; compares the pack with the test off / on")
    common.add_rival_flags(ap)
    args = ap.parse_args()
    waypoints = common.raceline(args)
    if args.opponents > 0:
        return opponent_runs(args, waypoints)
    lanes = ids = None
    if args.tracks > 0:
        args.envs = args.tracks
        normal = waypoints[:, 3] + np.pi / 2
        lanes = []
        for k in range(args.tracks):                           # lanes 0.25 m apart, centred on the raceline
            lane = waypoints.copy()
            d = 0.25 * (k - (args.tracks - 1) / 2)
            lane[:, 0] += d * np.cos(normal)
            lane[:, 1] += d * np.sin(normal)
            lanes.append(lane)
        ids = np.arange(args.tracks, dtype=np.int32)           # agent i plans along lane i
    planner = LatticePlanner(waypoints=waypoints)
    planner.configure(lookahead_distances=np.linspace(0.8, 2.4, 8), widths=np.linspace(-0.6, 0.6, 9), num_stations=50,
                      generator=args.generator)
    if args.map:
        planner.load_map(args.map)
    else:
        img, origin = synth.make_grid(waypoints[:, :2], size=(2000, 2000), resolution=0.058)
        planner.set_map(img, 0.058, origin, occupied_thresh=0.2)

    def plan(obs, env):
        if lanes is not None:
            poses = np.column_stack([obs['poses_x'], obs['poses_y'], obs['poses_theta'], obs['linear_vels_x']])
            out = planner.plan_batch(poses, want_traj=False, tracks=lanes, track_ids=ids)
            return np.column_stack([out["steer"], out["speed"]])
        if args.envs == 1:
            steer, speed, _traj = planner.plan(obs['poses_x'][0], obs['poses_y'][0], obs['poses_theta'][0], obs['linear_vels_x'][0])
            return [[steer, speed]]
        poses = np.column_stack([obs['poses_x'], obs['poses_y'], obs['poses_theta'], obs['linear_vels_x']])
        out = planner.plan_batch(poses, want_traj=False)
        return np.column_stack([out["steer"], out["speed"]])

    common.run(args, waypoints, plan, speed_scale=0.6, report_every=250)


if __name__ == "__main__":
    main()
