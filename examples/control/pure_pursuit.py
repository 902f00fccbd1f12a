"""Pure-pursuit waypoint tracking in closed loop (loop shape of the reference's examples/control/pure_pursuit.py:35-58)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import common  # noqa: E402

from f1tenth_planning.control.pure_pursuit.pure_pursuit import PurePursuitPlanner  # noqa: E402


def main():
    ap = common.parser(__doc__)
    ap.add_argument("--lookahead", type=float, default=0.8)
    ap.add_argument("--tracks", type=int, default=0, help="N agents on N lanes offset sideways from the raceline, one track set")
    args = ap.parse_args()
    waypoints = common.raceline(args)
    planner = PurePursuitPlanner(waypoints=waypoints)
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
        ids = np.arange(args.tracks, dtype=np.int32)           # agent i follows lane i

    def plan(obs, env):
        if lanes is not None:
            out = planner.plan_batch(np.column_stack([obs['poses_x'], obs['poses_y'], obs['poses_theta']]), args.lookahead,
                                     tracks=lanes, track_ids=ids)
            return np.column_stack([out["steer"], out["speed"]])
        if args.envs == 1:      # the reference's call, one vehicle
            steer, speed = planner.plan(obs['poses_x'][0], obs['poses_y'][0], obs['poses_theta'][0], args.lookahead)
            return [[steer, speed]]
        out = planner.plan_batch(np.column_stack([obs['poses_x'], obs['poses_y'], obs['poses_theta']]), args.lookahead)
        return np.column_stack([out["steer"], out["speed"]])

    common.run(args, waypoints, plan)


if __name__ == "__main__":
    main()
