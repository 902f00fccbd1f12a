"""StanleyPlanner on the MI355X path.

Same class, constructor and `plan` signature as the reference (f1tenth_planning/control/stanley/stanley.py:37-139);
the front-axle nearest-point search and the control law run in libf1p.so (csrc/k_controllers.hip).
"""
import numpy as np

from ..._planner import Planner


class StanleyPlanner(Planner):
    """
    Front-wheel feedback (Stanley) path tracker.

    Args:
        wheelbase (float, optional, default=0.33)
        waypoints (numpy.ndarray [N, m >= 4], optional): columns [x, y, velocity, heading, ...]
    """

    def __init__(self, wheelbase=0.33, waypoints=None, device=None):
        self.wheelbase = wheelbase
        self.waypoints = waypoints
        self._device = device
        self._ctx = None

    def _bind(self, waypoints):
        return self._bind_waypoints(waypoints, 4, 'Waypoints needs to be a (Nxm), m >= 4, numpy array!')          # stanley.py:131-132

    def plan(self, pose_x, pose_y, pose_theta, velocity, k_path=5., waypoints=None):
        """Returns (steering_angle, speed) for one vehicle (stanley.py:114-139)."""
        ctx = self._bind(waypoints)
        out = ctx.stanley(np.array([[pose_x, pose_y, pose_theta, velocity]], dtype=np.float64), self.wheelbase, k_path)
        return float(out["steer"][0]), float(out["speed"][0])

    def plan_batch(self, states, k_path=5., waypoints=None, tracks=None, track_ids=None):
        """states [E, 4] = (x, y, theta, velocity) -> dict(steer [E], speed [E], near_idx [E]).
        tracks: K waypoint arrays [N_k x m], m >= 4, with track_ids [E]: ego e follows tracks[track_ids[e]] (an id outside [0, K):
        NaN steer / speed, near_idx -1); `waypoints` is then not used."""
        if tracks is not None:
            return self._bind_tracks(tracks, track_ids, 4).stanley_tracks(states, track_ids, self.wheelbase, k_path)
        return self._bind(waypoints).stanley(states, self.wheelbase, k_path)
