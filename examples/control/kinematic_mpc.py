"""Kinematic MPC (random shooting, or with --solver qp the reference's linearised QP, on the GPU) in closed loop (loop shape of the reference's
examples/control/kinematic_mpc.py:35-67): the planner gets the simulator's 7-state and the waypoints as [x, y, yaw, v].

--obstacles N parks N obstacles on the line of the synthetic track and drives the loop twice, without and with the occupancy test on the
rollouts (mpc_config.COLLISION), counting the vehicle-steps that ended in an occupied cell.

--opponents M (with --envs E >= 2) starts the E vehicles as a pack on one course, the fast ones behind the slow ones, and drives the loop
twice: each vehicle planning as if it were alone, then with its M nearest other vehicles as moving obstacles, predicted at constant
velocity (planner.obstacles).  It reports the smallest distance between two vehicles over each run.  With --rivals the opponents are not
built here but found on the device by every plan (planner.rivals = Rivals(count=M, radius=...)); --groups G then splits the pack into G
independent races.  --predict track predicts each rival along the raceline over the planner's
horizon instead of at constant velocity (Rivals(predict="track")); --rival-speed profile then moves it with the raceline's speed profile
instead of at its current speed (Rivals(predict="track", speed="profile")).

--solver qp --avoid (mpc_config.QP_AVOID) lets the QP take the same obstacles and rivals as soft half-plane rows; without
--avoid the QP takes none and --opponents with it is an error.

--solver qp --walls (mpc_config.QP_WALLS) lets the QP see the synthetic track's occupancy grid, inflated by --inflate R metres: the walls within
--reach M metres of the previous solution's path become soft half-plane rows beside the discs' (DESIGN.md 5s).  Combinable with --avoid,
--envs and --opponents (not --obstacles, the shooting solver's comparison); the plain loop reports the vehicle-steps that ended in an
occupied cell of the map."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import common  # noqa: E402

from f1tenth_planning.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config  # noqa: E402


def obstacle_runs(args, rl, waypoints, cfg):
    return common.obstacle_runs(args, rl, waypoints, cfg, lambda wp, c: KMPCPlanner(waypoints=wp, config=c),
                                lambda env: env.state[:, [0, 1, 3, 4]], lambda c, n: setattr(c, "COLLISION_SUBSTEPS", n))


def opponent_runs(args, rl, waypoints, cfg, make_planner):
    cfg.COLLISION_SUBSTEPS = args.substeps
    return common.opponent_runs(args, rl, waypoints, cfg, make_planner, lambda env: env.state[:, [0, 1, 3, 4]])


def wall_map(args, rl, resolution=0.05, cells=900):
    """the synthetic track's occupancy image for --walls: (img, resolution, origin)"""
    from f1tenth_planning_amd import synth
    img, origin = synth.make_grid(rl[:, :2], size=(cells, cells), resolution=resolution)
    return img, resolution, (origin[0], origin[1], 0.0)


def main():
    ap = common.parser(__doc__, steps=600)
    ap.add_argument("--rollouts", type=int, default=512)
    ap.add_argument("--solver", choices=["shooting", "qp"], default="shooting")
    ap.add_argument("--obstacles", type=int, default=0, help="park N obstacles (discs of 0.3 m) on the line and compare the loop with the occupancy test off / on")
    ap.add_argument("--opponents", type=int, default=0, help="with --envs E: each vehicle's M nearest other vehicles are moving obstacles of its rollouts; compares the pack with the test off / on")
    common.add_rival_flags(ap)
    ap.add_argument("--avoid", action="store_true", help="with --solver qp: the opponents / rivals as soft half-plane rows of the QP (mpc_config.QP_AVOID)")
    ap.add_argument("--walls", action="store_true", help="with --solver qp: the occupancy grid's walls as soft half-plane rows of the QP (mpc_config.QP_WALLS)")
    ap.add_argument("--inflate", type=float, default=0.15, help="with --walls: the map is inflated by this many metres (set_map(inflate=...))")
    ap.add_argument("--reach", type=float, default=1.5, help="with --walls: how far to each side a wall is looked for [m] (mpc_config.QP_WALL_REACH)")
    ap.add_argument("--substeps", type=int, default=4, help="tested points per time step of a rollout (mpc_config.COLLISION_SUBSTEPS)")
    args = ap.parse_args()
    if args.avoid and args.solver != "qp":
        ap.error("--avoid adds rows to the QP: use it with --solver qp")
    if args.walls and args.solver != "qp":
        ap.error("--walls adds rows to the QP: use it with --solver qp")
    if args.walls and args.obstacles > 0:
        ap.error("--obstacles compares the shooting solver's occupancy test; --walls is the QP's (drop one of them)")
    rl = common.raceline(args, centerline=True)
    waypoints = [rl[:, 0], rl[:, 1], rl[:, 3], rl[:, 2]]          # [x, y, yaw, v]
    cfg = mpc_config()
    cfg.N_ROLLOUTS = args.rollouts
    cfg.SOLVER = args.solver
    cfg.QP_AVOID = args.avoid
    cfg.QP_WALLS, cfg.QP_WALL_REACH = args.walls, args.reach
    grid = wall_map(args, rl) if args.walls else None

    def make_planner(wp, c):
        pl = KMPCPlanner(waypoints=wp, config=c)
        if grid is not None:
            pl.set_map(*grid, inflate=args.inflate)
        return pl

    if args.obstacles > 0:
        return obstacle_runs(args, rl, waypoints, cfg)
    if args.opponents > 0:
        return opponent_runs(args, rl, waypoints, cfg, make_planner)
    planner = make_planner(waypoints, cfg)
    in_wall = [0]
    occupied = None if grid is None else grid[0][::-1] < 128           # [gy][gx], the map as given: what counts as a hit

    def count_in_wall(env):
        """vehicles standing in an occupied cell of the map, or off it"""
        if occupied is None:
            return
        gx = np.floor((env.state[:, 0] - grid[2][0]) / grid[1]).astype(int)
        gy = np.floor((env.state[:, 1] - grid[2][1]) / grid[1]).astype(int)
        ok = (gx >= 0) & (gy >= 0) & (gx < occupied.shape[1]) & (gy < occupied.shape[0])
        in_wall[0] += int((~ok).sum() + occupied[gy[ok], gx[ok]].sum())

    def plan(obs, env):
        count_in_wall(env)
        if args.envs == 1:
            steer, speed = planner.plan(env.sim.agents[0].state)
            return [[steer, speed]]
        out = planner.plan_batch(env.state[:, [0, 1, 3, 4]])
        return np.column_stack([out["steer"], out["speed"]])

    common.run(args, rl, plan, report_every=200, avoid_heading_wrap=True)
    if args.walls:
        print(f"wall rows on (inflate {args.inflate} m, reach {args.reach} m): {in_wall[0]} of {args.steps * args.envs} vehicle-steps ended in an occupied cell of the map")


if __name__ == "__main__":
    main()
