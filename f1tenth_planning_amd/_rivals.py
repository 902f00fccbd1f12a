"""planner.rivals: the vehicles of a batch as each other's moving obstacles, found on the device (include/f1p.h "Rivals").

`Rivals` is what a user assigns to the attribute `rivals` of KMPCPlanner, STMPCPlanner or LatticePlanner; `RivalFeed` is the device side one
planner keeps for it: the state, slot and pace buffers per (context, E, M) and the races on the context."""
from dataclasses import dataclass

import numpy as np

from .runtime import rivals_dev, rivals_predict_dev, rivals_set_course, rivals_set_groups


@dataclass(frozen=True, eq=False)
class Rivals:
    """planner.rivals = Rivals(count=M, radius=r): while set, every plan_batch (and the lattice's step_batch) tests each ego against its
    `count` nearest other vehicles of the call's own states, as discs of `radius` (both vehicles' radii folded in) at constant velocity.
    reach: vehicles farther than this [m] are left out.  groups: int [E], egos with the same id >= 0 are one race, an ego with a negative id
    has no rivals and is nobody's rival; None: one race of all.  Persistent, unlike `obstacles`: it stays until set to None.
    predict="track": each rival is predicted along the course it follows -- the call's tracks / track_ids where the planner takes them, else the
    planner's raceline -- and its slot carries the chord of that path over the planner's horizon, sampled at knots + 1 points; inflate: the radius
    grows by the path's largest distance from the chord; wrap: the courses are loops.  horizon [s]: overrides the planner's own.
    speed="profile" (with predict="track"): the rival follows its course's speed column, scaled by its speed now over the course's speed where it
    stands -- it brakes into the bend its raceline brakes into -- instead of keeping |v| along the course ("constant")."""
    count: int
    radius: float
    reach: float = float("inf")
    groups: object = None
    predict: str = "velocity"
    horizon: object = None
    knots: int = 8
    inflate: bool = True
    wrap: bool = True
    speed: str = "constant"


SINGLE_EGO = "plan() drives one ego, which has no rivals: set planner.rivals = None, or use plan_batch()"


def check_rivals(rivals, E, obstacles=None, solver=None, devices=None):
    """ValueError before anything touches the GPU"""
    if obstacles is not None:
        raise ValueError("planner.rivals and planner.obstacles in one call: the rivals fill the obstacle slots, set one of them to None")
    if solver == "qp":
        raise ValueError("rivals are tested on the shooting solver's rollouts; SOLVER='qp' takes none")
    if devices is not None:
        raise ValueError("rivals are per-ego arrays of one context: multi-GPU plans (devices=...) take none")
    if not 1 <= int(rivals.count) <= 16:
        raise ValueError(f"Rivals.count must be in [1, 16], not {rivals.count!r}")
    if not float(rivals.radius) >= 0.0 or not float(rivals.reach) >= 0.0:
        raise ValueError("Rivals.radius and Rivals.reach must be >= 0")
    if rivals.predict not in ("velocity", "track"):
        raise ValueError(f"Rivals.predict must be 'velocity' or 'track', not {rivals.predict!r}")
    if rivals.speed not in ("constant", "profile"):
        raise ValueError(f"Rivals.speed must be 'constant' or 'profile', not {rivals.speed!r}")
    if rivals.speed == "profile" and rivals.predict != "track":
        raise ValueError("Rivals.speed='profile' is a speed along the rival's course: it needs predict='track'")
    if not 1 <= int(rivals.knots) <= 16:
        raise ValueError(f"Rivals.knots must be in [1, 16], not {rivals.knots!r}")
    if rivals.horizon is not None and not float(rivals.horizon) > 0.0:
        raise ValueError(f"Rivals.horizon must be > 0 [s], not {rivals.horizon!r}")
    if rivals.groups is not None and np.asarray(rivals.groups).reshape(-1).shape[0] != E:
        raise ValueError(f"Rivals.groups must hold one id per ego ({E}), not {np.asarray(rivals.groups).reshape(-1).shape[0]}")


class RivalFeed:
    """layout: the planner's state layout ("xyvyaw", "pose", "st7"); clear(ctx): the planner's *_set_obstacles_dev(ctx, None) -- the context
    must stop borrowing the slot buffer before it is freed"""

    def __init__(self, layout, clear):
        self.layout, self.clear = layout, clear
        self.ncol = 7 if layout == "st7" else 4
        self._key, self._bufs, self._groups, self._course = None, None, None, None

    def run(self, ctx, rivals, states, min_speed=0.5, horizon=(0.0, 0.0), track_ids=None):
        """upload the call's states [E, ncol] and fill the slots (and paces) from them, asynchronously -> (d_obs, d_pace, E, M).
        predict="track": horizon = the planner's own (horizon_s, horizon_m); track_ids: the call's, the context then holds its track set, None:
        the context holds the raceline"""
        E, M = states.shape[0], int(rivals.count)
        key = (id(ctx), E, M)
        if self._key != key:
            if self._bufs is not None:
                if self._bufs[0].ctx is ctx:
                    self.clear(ctx)                          # first: the context borrows d_obs / d_pace
                for b in self._bufs:
                    b.free()
            self._bufs = (ctx.alloc(8 * self.ncol * E), ctx.alloc(40 * E * M), ctx.alloc(8 * E))
            self._key, self._groups, self._course = key, None, None
        g = None if rivals.groups is None else np.ascontiguousarray(rivals.groups, dtype=np.int32).reshape(-1)
        gkey = (id(ctx), None if g is None else g.tobytes())
        if self._groups != gkey:
            rivals_set_groups(ctx, g)
            self._groups = gkey
        d_states, d_obs, d_pace = self._bufs
        d_states.upload(states)
        if rivals.predict == "track":
            t = None if track_ids is None else np.ascontiguousarray(track_ids, dtype=np.int32).reshape(-1)
            ckey = (id(ctx), None if t is None else t.tobytes())
            if self._course != ckey:
                rivals_set_course(ctx, t)
                self._course = ckey
            hs, hm = (float(rivals.horizon), 0.0) if rivals.horizon is not None else horizon
            rivals_predict_dev(ctx, d_states, self.layout, E, M, float(rivals.radius), d_obs, hs, hm, int(rivals.knots), bool(rivals.inflate),
                               bool(rivals.wrap), d_pace, None, None, float(rivals.reach), float(min_speed), speed=rivals.speed)
            return d_obs, d_pace, E, M
        rivals_dev(ctx, d_states, self.layout, E, M, float(rivals.radius), d_obs, d_pace, None, float(rivals.reach), float(min_speed))
        return d_obs, d_pace, E, M
