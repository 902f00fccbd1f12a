"""Context's rivals: each ego's nearest other vehicles of its race as the moving discs the three sampling planners test
(csrc/f1p_rivals.hip, csrc/k_rivals.hip; the rule: include/f1p.h "Rivals").
Predicted along the course each rival follows: csrc/k_rivals_predict.hip; include/f1p.h "Rivals, predicted along the course", DESIGN.md 5n.
speed="profile": the rival moves along that course with the course's speed profile, scaled by its own speed now."""
import ctypes as C

import numpy as np

from .. import _abi
from .core import _dev, _f64, _ptr

LAYOUTS = {"xyvyaw": _abi.RIVALS_XYVYAW, "pose": _abi.RIVALS_POSE, "st7": _abi.RIVALS_ST7}
SPEEDS = {"constant": _abi.RIVALS_SPEED_CONSTANT, "profile": _abi.RIVALS_SPEED_PROFILE}


def rivals_set_groups(ctx, groups):
    """the races of the following rivals calls on Context `ctx` (f1p_rivals_set_groups): groups int32 [E], egos with the same id >= 0 are one
    race, an ego with a negative id has no rivals and is nobody's rival; None: one race of all.  (The public face of
    Context._rivals_set_groups: Context's public methods are a pinned record, tests/test_runtime_calls.py.)"""
    ctx._rivals_set_groups(groups)


def rivals(ctx, states, layout, M, radius, reach=np.inf, min_speed=0.5):
    """each ego's M nearest other vehicles of its race within `reach`, as discs of `radius` moving at constant velocity (f1p_rivals_batch):
    states [E, 4] = (x, y, v, yaw) for layout "xyvyaw" / RIVALS_XYVYAW, (x, y, theta, v) for "pose", [E, 7] for "st7" ->
    dict(obs [E, M, 5] = (x, y, vx, vy, r) with (0, 0, 0, 0, -1) in the empty slots, pace [E] = 1 / max(|v|, min_speed), idx int32 [E, M] = the
    chosen vehicles, -1 in the empty slots)"""
    return ctx._rivals(states, layout, M, radius, reach, min_speed)


def rivals_dev(ctx, d_states, layout, E, M, radius, d_obs, d_pace=None, d_idx=None, reach=np.inf, min_speed=0.5):
    """rivals on device buffers, asynchronous on the context's stream (f1p_rivals_dev): d_obs [E][M][5] fp64 (and d_pace [E]) may be the very
    arrays kmpc_set_obstacles_dev / stmpc_set_obstacles_dev / lattice_set_obstacles_dev borrow"""
    ctx._rivals_dev(d_states, layout, E, M, radius, d_obs, d_pace, d_idx, reach, min_speed)


def rivals_set_course(ctx, track_ids):
    """the course each vehicle of the following rivals_predict calls follows (f1p_rivals_set_course): track_ids int32 [E], vehicle j follows
    track track_ids[j] of the context's track set; None: every vehicle follows the context's raceline"""
    ctx._rivals_set_course(track_ids)


def rivals_predict(ctx, states, layout, M, radius, horizon_s, horizon_m=0.0, knots=8, inflate=True, wrap=True, reach=np.inf, min_speed=0.5,
                   speed="constant"):
    """rivals() with every live slot predicted along the course its vehicle follows (f1p_rivals_predict_batch): (vx, vy) is the chord of the
    vehicle's path along its course over H_i = horizon_s + horizon_m * pace_i, sampled at `knots` + 1 points, and with `inflate` the radius
    grows by the path's largest distance from that chord; wrap: the course is a loop; speed: "constant" / RIVALS_SPEED_CONSTANT, the vehicle keeps
    |v| along its course, or "profile", it follows the course's speed column scaled by |v| over the course's speed where it stands, floored at
    min_speed -> dict(obs, pace, idx as rivals(), frenet [E, 3] = (s0, d, dir) per vehicle, a NaN row for one that keeps the
    constant-velocity slot)"""
    return ctx._rivals_predict(states, layout, M, radius, reach, min_speed,
                               _abi.rivals_predict(horizon_s, horizon_m, knots, inflate, wrap, _speed(speed)))


def rivals_predict_dev(ctx, d_states, layout, E, M, radius, d_obs, horizon_s, horizon_m=0.0, knots=8, inflate=True, wrap=True, d_pace=None,
                       d_idx=None, d_frenet=None, reach=np.inf, min_speed=0.5, speed="constant"):
    """rivals_predict on device buffers, asynchronous on the context's stream (f1p_rivals_predict_dev); d_frenet [E][3] fp64, nullable"""
    ctx._rivals_predict_dev(d_states, layout, E, M, radius, d_obs, d_pace, d_idx, d_frenet, reach, min_speed,
                            _abi.rivals_predict(horizon_s, horizon_m, knots, inflate, wrap, _speed(speed)))


def _layout(layout):
    return LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def _speed(speed):
    """a name of SPEEDS, or the C-ABI's integer as it is (the library rejects an unknown one)"""
    if isinstance(speed, str):
        if speed not in SPEEDS:
            raise ValueError(f"speed must be 'constant' or 'profile', not {speed!r}")
        return SPEEDS[speed]
    return int(speed)


class _Rivals:
    def _rivals_set_groups(self, groups):
        if groups is None:
            self._check(self.lib.f1p_rivals_set_groups(self.h, None, 0))
            return
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        self._check(self.lib.f1p_rivals_set_groups(self.h, _ptr(g), g.shape[0]))

    def _rivals(self, states, layout, M, radius, reach, min_speed):
        layout = _layout(layout)
        st = _f64(states, (-1, 7 if layout == _abi.RIVALS_ST7 else 4)); E = st.shape[0]; M = int(M)
        out = dict(obs=np.empty((E, max(M, 0), 5)), pace=np.empty(E), idx=np.empty((E, max(M, 0)), np.int32))
        self._check(self.lib.f1p_rivals_batch(self.h, _ptr(st), layout, E, M, float(radius), float(reach), float(min_speed), _ptr(out["obs"]),
                                              _ptr(out["pace"]), _ptr(out["idx"])))
        return out

    def _rivals_dev(self, d_states, layout, E, M, radius, d_obs, d_pace, d_idx, reach, min_speed):
        self._check(self.lib.f1p_rivals_dev(self.h, _dev(d_states), _layout(layout), int(E), int(M), float(radius), float(reach), float(min_speed),
                                            _dev(d_obs), _dev(d_pace), _dev(d_idx)))

    def _rivals_set_course(self, track_ids):
        if track_ids is None:
            self._check(self.lib.f1p_rivals_set_course(self.h, None, 0))
            return
        t = np.ascontiguousarray(track_ids, dtype=np.int32).reshape(-1)
        self._check(self.lib.f1p_rivals_set_course(self.h, _ptr(t), t.shape[0]))

    def _rivals_predict(self, states, layout, M, radius, reach, min_speed, pr):
        layout = _layout(layout)
        st = _f64(states, (-1, 7 if layout == _abi.RIVALS_ST7 else 4)); E = st.shape[0]; M = int(M)
        out = dict(obs=np.empty((E, max(M, 0), 5)), pace=np.empty(E), idx=np.empty((E, max(M, 0)), np.int32), frenet=np.empty((E, 3)))
        self._check(self.lib.f1p_rivals_predict_batch(self.h, _ptr(st), layout, E, M, float(radius), float(reach), float(min_speed), C.byref(pr),
                                                      _ptr(out["obs"]), _ptr(out["pace"]), _ptr(out["idx"]), _ptr(out["frenet"])))
        return out

    def _rivals_predict_dev(self, d_states, layout, E, M, radius, d_obs, d_pace, d_idx, d_frenet, reach, min_speed, pr):
        self._check(self.lib.f1p_rivals_predict_dev(self.h, _dev(d_states), _layout(layout), int(E), int(M), float(radius), float(reach),
                                                    float(min_speed), C.byref(pr), _dev(d_obs), _dev(d_pace), _dev(d_idx), _dev(d_frenet)))
