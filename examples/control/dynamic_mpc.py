"""Single-track MPC (random shooting, or with --solver qp the reference's linearised QPs; kinematic model below V_KS, dynamic model above) in closed loop
(loop shape of the reference's examples/control/dynamic_mpc.py).

--obstacles N parks N obstacles on the line of the synthetic track and drives the loop twice, without and with the occupancy test on the
rollouts (mpc_config.COLLISION), counting the vehicle-steps that ended in an occupied cell.

--opponents M (with --envs E >= 2) starts the E vehicles as a pack on one course, the fast ones behind the slow ones, and drives the loop
twice: each vehicle planning as if it were alone, then with its M nearest other vehicles as moving obstacles, predicted at constant
velocity (planner.obstacles; both branches of the model test them).  It reports the smallest distance between two vehicles over each run.
With --rivals the opponents are not built here but found on the device by every plan (planner.rivals = Rivals(count=M, radius=...));
--groups G then splits the pack into G independent races.  --predict track predicts each rival along the raceline over the planner's
horizon instead of at constant velocity (Rivals(predict="track")); --rival-speed profile then moves it with the raceline's speed profile
instead of at its current speed (Rivals(predict="track", speed="profile")).

--solver qp --avoid (mpc_config.QP_AVOID) lets the QPs of both branches take the same obstacles and rivals as soft half-plane rows
(DESIGN.md 5r); without --avoid the QP takes none and --opponents with it is an error.

--solver qp --walls (mpc_config.QP_WALLS_ST) lets the QPs of both branches see the synthetic track's occupancy grid, inflated by --inflate R metres:
the walls within --reach M metres of the previous solution's path become soft half-plane rows beside the discs', kept --margin M metres off the
contact.  Combinable with --avoid, --envs / --opponents and --tracks (not --obstacles, the shooting solver's comparison); the
plain loop reports the vehicle-steps that ended in an occupied cell of the map."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import common  # noqa: E402

from f1tenth_planning.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config  # noqa: E402


def main():
    ap = common.parser(__doc__, steps=600)
    ap.add_argument("--solver", choices=["shooting", "qp"], default="shooting")
    ap.add_argument("--tracks", type=int, default=0, help="N agents on N lanes offset sideways from the centreline, one track set (--solver qp)")
    ap.add_argument("--obstacles", type=int, default=0, help="park N obstacles (discs of 0.3 m) on the line and compare the loop with the occupancy test off / on")
    ap.add_argument("--opponents", type=int, default=0, help="with --envs E: each vehicle's M nearest other vehicles are moving obstacles of its rollouts; compares the pack with the test off / on")
    common.add_rival_flags(ap)
    ap.add_argument("--avoid", action="store_true", help="with --solver qp: the opponents / rivals as soft half-plane rows of the QPs (mpc_config.QP_AVOID)")
    ap.add_argument("--walls", action="store_true", help="with --solver qp: the occupancy grid's walls as soft half-plane rows of the QPs (mpc_config.QP_WALLS_ST)")
    ap.add_argument("--inflate", type=float, default=0.15, help="with --walls: the map is inflated by this many metres (set_map(inflate=...))")
    ap.add_argument("--reach", type=float, default=1.5, help="with --walls: how far to each side a wall is looked for [m] (mpc_config.QP_WALL_REACH)")
    ap.add_argument("--margin", type=float, default=0.05, help="with --walls: the rows keep this far off the contact [m] (mpc_config.QP_WALL_MARGIN)")
    ap.add_argument("--substeps", type=int, default=1, help="tested points per step of the dynamic model (mpc_config.COLLISION_SUBSTEPS; the kinematic branch tests twice as many)")
    args = ap.parse_args()
    if args.avoid and args.solver != "qp":
        ap.error("--avoid adds rows to the QP: use it with --solver qp")
    if args.walls and args.solver != "qp":
        ap.error("--walls adds rows to the QP: use it with --solver qp")
    if args.walls and args.obstacles > 0:
        ap.error("--obstacles compares the shooting solver's occupancy test; --walls is the QP's (drop one of them)")
    lanes = ids = None
    if args.tracks > 0:
        if args.solver != "qp":
            raise SystemExit("--tracks plans with STMPCPlanner.plan_batch, which needs --solver qp")
        args.envs = args.tracks
    if args.envs != 1 and args.tracks == 0 and args.solver != "shooting" and not (args.avoid and args.opponents > 0):
        raise SystemExit("--envs N drives N vehicles with the shooting solver's plan_batch; with --solver qp use --tracks N")
    rl = common.raceline(args, centerline=True)
    grid = None
    if args.walls:
        from kinematic_mpc import wall_map                        # the synthetic track's occupancy image: (img, resolution, origin)
        grid = wall_map(args, rl)

    def make_planner(wp, c):
        c.QP_WALLS_ST, c.QP_WALL_REACH, c.QP_WALL_MARGIN = args.walls, args.reach, args.margin
        pl = STMPCPlanner(waypoints=wp, config=c)
        if grid is not None:
            pl.set_map(*grid, inflate=args.inflate)
        return pl

    if args.obstacles > 0:
        if args.solver == "qp" or args.tracks > 0:
            raise SystemExit("--obstacles needs the shooting solver on the raceline (the QP has no rollouts to test)")

        def substeps(c, n):
            c.COLLISION_SUBSTEPS, c.COLLISION_SUBSTEPS_K = n, min(2 * n, 16)

        return common.obstacle_runs(args, rl, [rl[:, 0], rl[:, 1], rl[:, 3], rl[:, 2]], mpc_config(),
                                    lambda wp, c: STMPCPlanner(waypoints=wp, config=c), lambda env: env.state, substeps)
    if args.opponents > 0:
        if args.tracks > 0:
            raise SystemExit("--opponents drives the pack on the raceline with the shooting solver")
        cfg = mpc_config(SOLVER=args.solver, QP_AVOID=args.avoid)
        cfg.COLLISION_SUBSTEPS, cfg.COLLISION_SUBSTEPS_K = args.substeps, min(2 * args.substeps, 16)
        return common.opponent_runs(args, rl, [rl[:, 0], rl[:, 1], rl[:, 3], rl[:, 2]], cfg, make_planner, lambda env: env.state)
    planner = make_planner([rl[:, 0], rl[:, 1], rl[:, 3], rl[:, 2]], mpc_config(SOLVER=args.solver))
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
    if args.tracks > 0:
        normal = rl[:, 3] + np.pi / 2
        lanes = []
        for k in range(args.tracks):                           # lanes 0.25 m apart, centred on the centreline
            d = 0.25 * (k - (args.tracks - 1) / 2)
            lanes.append([rl[:, 0] + d * np.cos(normal), rl[:, 1] + d * np.sin(normal), rl[:, 3], rl[:, 2]])   # [x, y, yaw, v]
        ids = np.arange(args.tracks, dtype=np.int32)           # agent i follows lane i

    def plan(obs, env):
        count_in_wall(env)
        if lanes is not None:
            out = planner.plan_batch(env.state, tracks=lanes, track_ids=ids)
            return np.column_stack([out["steer"], out["speed"]])
        if args.envs > 1:                                      # one C call per step: controls generated on the GPU, one warm start per vehicle
            out = planner.plan_batch(env.state, want_u=False)
            return np.column_stack([out["steer"], out["speed"]])
        steer, speed = planner.plan(env.sim.agents[0].state)
        return [[steer, speed]]

    common.run(args, rl, plan, report_every=200, avoid_heading_wrap=True)
    if args.walls:
        print(f"wall rows on (inflate {args.inflate} m, reach {args.reach} m, margin {args.margin} m): {in_wall[0]} of {args.steps * args.envs} "
              f"vehicle-steps ended in an occupied cell of the map")


if __name__ == "__main__":
    main()
