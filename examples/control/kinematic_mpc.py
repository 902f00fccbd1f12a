"""Kinematic MPC (random shooting, or with --solver qp the reference's linearised QP, on the GPU) in closed loop (loop shape of the reference's
examples/control/kinematic_mpc.py:35-67): the planner gets the simulator's 7-state and the waypoints as [x, y, yaw, v].

--obstacles N parks N obstacles on the line of the synthetic track and drives the loop twice, without and with the occupancy test on the
rollouts (mpc_config.COLLISION), counting the vehicle-steps that ended in an occupied cell."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import common  # noqa: E402

from f1tenth_planning.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config  # noqa: E402


def obstacle_runs(args, rl, waypoints, cfg, resolution=0.05, cells=900, inflate=0.15):
    """the synthetic grid of the track + parked obstacles; one closed loop per setting of the test, the same start poses"""
    from f1tenth_planning_amd import sim, synth
    if args.solver == "qp":
        raise SystemExit("--obstacles needs the shooting solver (the QP has no rollouts to test)")
    img, origin = synth.make_grid(rl[:, :2], size=(cells, cells), resolution=resolution)
    length = float(np.hypot(np.diff(rl[:, 0]), np.diff(rl[:, 1])).sum())
    img, centres = synth.stamp_obstacles(img, origin, resolution, rl, spacing=length / args.obstacles, radius=0.30)
    occupied = img[::-1] < 128                                          # [gy][gx], the uninflated map: what counts as a hit
    print(f"{len(centres)} obstacles on {length:.1f} m of track, {args.envs} vehicle(s), {args.steps} steps")
    poses = common.start_poses(args, rl, avoid_heading_wrap=True)
    for p in poses:                                                     # nobody starts inside or right behind an obstacle
        k = int(np.argmin(np.hypot(rl[:, 0] - p[0], rl[:, 1] - p[1])))
        while np.hypot(centres[:, 0] - rl[k, 0], centres[:, 1] - rl[k, 1]).min() < 1.5:
            k = (k + 5) % (len(rl) - 1)
            p[:] = (rl[k, 0], rl[k, 1], rl[k, 3])
    hits = {}
    for on in (False, True):
        cfg.COLLISION, cfg.COLLISION_SUBSTEPS = on, args.substeps
        planner = KMPCPlanner(waypoints=[w.copy() for w in waypoints], config=cfg)
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
                out = planner.plan_batch(env.state[:, [0, 1, 3, 4]], want_seq=False)
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


def main():
    ap = common.parser(__doc__, steps=600)
    ap.add_argument("--rollouts", type=int, default=512)
    ap.add_argument("--solver", choices=["shooting", "qp"], default="shooting")
    ap.add_argument("--obstacles", type=int, default=0, help="park N obstacles (discs of 0.3 m) on the line and compare the loop with the occupancy test off / on")
    ap.add_argument("--substeps", type=int, default=4, help="tested points per time step of a rollout (mpc_config.COLLISION_SUBSTEPS)")
    args = ap.parse_args()
    rl = common.raceline(args, centerline=True)
    waypoints = [rl[:, 0], rl[:, 1], rl[:, 3], rl[:, 2]]          # [x, y, yaw, v]
    cfg = mpc_config()
    cfg.N_ROLLOUTS = args.rollouts
    cfg.SOLVER = args.solver
    if args.obstacles > 0:
        return obstacle_runs(args, rl, waypoints, cfg)
    planner = KMPCPlanner(waypoints=waypoints, config=cfg)

    def plan(obs, env):
        if args.envs == 1:
            steer, speed = planner.plan(env.sim.agents[0].state)
            return [[steer, speed]]
        out = planner.plan_batch(env.state[:, [0, 1, 3, 4]])
        return np.column_stack([out["steer"], out["speed"]])

    common.run(args, rl, plan, report_every=200, avoid_heading_wrap=True)


if __name__ == "__main__":
    main()
