"""Context's kinematic and dynamic MPC: references, rollouts, shooting and the linearised QPs (csrc/f1p_kmpc.hip, csrc/f1p_stmpc.hip)."""
import ctypes as C

import numpy as np

from .. import _abi
from .._abi import KmpcCfg
from .core import _dev, _f64, _pick, _ptr, _ref, _tid


def kmpc_set_obstacles(ctx, obs):
    """moving discs for the shooting solver's rollouts (f1p_kmpc_set_obstacles) on Context `ctx`: obs [E, M, 5] fp64 rows (x, y, vx, vy, r),
    map frame, M <= 16, a row with r < 0 or NaN is empty; they stay in force for kmpc_plan* / kmpc_shoot* of E egos until the next set.
    None clears.  (The public face of Context._kmpc_set_obstacles: Context's public methods are a pinned record, tests/test_runtime_calls.py.)"""
    ctx._kmpc_set_obstacles(obs)


def kmpc_set_obstacles_dev(ctx, d_obs, E=None, M=None):
    """kmpc_set_obstacles on a device buffer [E][M][5] fp64 that the context BORROWS: keep it alive, rewrite it in place between plans.
    E and M are required with a buffer; d_obs None clears."""
    ctx._kmpc_set_obstacles_dev(d_obs, E, M)


def stmpc_set_obstacles(ctx, obs):
    """kmpc_set_obstacles for the dynamic MPC's shooting solver (f1p_stmpc_set_obstacles), a state of its own: obs [E, M, 5] fp64 rows in the
    CALLER's ego order; in force for stmpc_plan / stmpc_plan_dev / stmpc_shoot* of E egos until the next set.  None clears."""
    ctx._stmpc_set_obstacles(obs)


def stmpc_set_obstacles_dev(ctx, d_obs, E=None, M=None):
    """stmpc_set_obstacles on a device buffer [E][M][5] fp64 that the context BORROWS: keep it alive, rewrite it in place between plans.
    E and M are required with a buffer; d_obs None clears."""
    ctx._stmpc_set_obstacles_dev(d_obs, E, M)


def kmpc_qp_avoid(ctx, x0, ref, obs, cfg, avoid=None, oa_prev=None, od_prev=None, opts=None, want_u=True, want_xk=False, want_obj=True,
                  want_duals=False, want_iters=True, want_eps=True, want_planes=False, want_avoid_duals=False):
    """Context.kmpc_qp with moving-disc avoidance rows (f1p_kmpc_qp_avoid_batch) on Context `ctx`: obs [E, M, 5] fp64 rows
    (x, y, vx, vy, r), M in 1..16, r < 0 or NaN = an empty slot; avoid: _abi.kmpc_qp_avoid(margin, rho, lin) (None: the defaults).  A soft,
    linearised avoidance term, not a guarantee.  -> kmpc_qp's dict[, eps [E], planes [E, T, 2, 4] = (n_x, n_y, right-hand side, slot; -1 and
    zeros: absent), avoid_duals [E, 2T+1]: the 2T avoidance rows in step order, then -eps <= 0]; obj includes the slack's cost.
    (A module function: Context's public methods are a pinned record, tests/test_runtime_calls.py.)"""
    return _mpc_qp(ctx, ctx.lib.f1p_kmpc_qp_avoid_batch, 4, "xk", 8, x0, ref, cfg, oa_prev, od_prev, opts, want_u, want_xk, want_obj, want_duals,
                   want_iters, (obs, avoid, want_eps, want_planes, want_avoid_duals))


def kmpc_qp_set_avoid(ctx, avoid):
    """f1p_kmpc_qp_set_avoid on Context `ctx`: while on, kmpc_qp_plan and kmpc_qp_dev take the discs of kmpc_set_obstacles[_dev] as soft
    half-plane rows of the QP; avoid: _abi.kmpc_qp_avoid(...), None (or on=False) turns it off"""
    ctx._check(ctx.lib.f1p_kmpc_qp_set_avoid(ctx.h, _ref(avoid)))


def kmpc_qp_walls(ctx, x0, ref, obs, cfg, avoid=None, walls=None, oa_prev=None, od_prev=None, opts=None, want_u=True, want_xk=False, want_obj=True,
                  want_duals=False, want_iters=True, want_eps=True, want_planes=False, want_avoid_duals=False):
    """kmpc_qp_avoid with wall rows from the context's ACTIVE occupancy bitmap (f1p_kmpc_qp_walls_batch): per step the two
    nearest of {the two nearest live discs, the wall to the left of the previous solution's path, the wall to its right} become the step's
    rows.  obs [E, M, 5] with M in 0..16, or None (no discs); walls: _abi.kmpc_qp_walls(n_samples, margin) (None: the defaults) -- n_samples
    steps of res / 2 per side.  Needs set_grid and no oriented footprint.  A soft, linearised avoidance term, not a guarantee.  -> kmpc_qp_avoid's
    dict; planes' slot 16 / 17: the left / right wall.  (A module function: Context's public methods are a pinned record.)"""
    if obs is None:
        obs = np.zeros((_f64(x0, (-1, 4)).shape[0], 0, 5))
    return _mpc_qp(ctx, ctx.lib.f1p_kmpc_qp_walls_batch, 4, "xk", 8, x0, ref, cfg, oa_prev, od_prev, opts, want_u, want_xk, want_obj, want_duals,
                   want_iters, (obs, avoid, want_eps, want_planes, want_avoid_duals), walls=(_ref(walls),))


def kmpc_qp_set_walls(ctx, walls):
    """f1p_kmpc_qp_set_walls on Context `ctx`: while on, kmpc_qp_plan and kmpc_qp_dev solve kmpc_qp_walls' problem on the grid the context
    holds at each call, with the discs of kmpc_set_obstacles[_dev] while kmpc_qp_set_avoid is on as well (else none) and its rho / lin;
    walls: _abi.kmpc_qp_walls(...), None (or on=False) turns it off"""
    ctx._check(ctx.lib.f1p_kmpc_qp_set_walls(ctx.h, _ref(walls)))


def stmpc_qp_avoid(ctx, x0, ref, obs, cfg, avoid=None, oa_prev=None, od_v_prev=None, opts=None, want_u=True, want_x=False, want_obj=True,
                   want_duals=False, want_iters=True, want_eps=True, want_planes=False, want_avoid_duals=False):
    """Context.stmpc_qp with moving-disc avoidance rows (f1p_stmpc_qp_avoid_batch) on Context `ctx`: obs [E, M, 5] fp64 rows
    (x, y, vx, vy, r), M in 1..16, r < 0 or NaN = an empty slot; avoid: _abi.kmpc_qp_avoid(margin, rho, lin) (None: the defaults); horizon
    <= _abi.STMPC_QP_AVOID_MAX_T.  A soft, linearised avoidance term, not a guarantee.  -> stmpc_qp's dict[, eps [E], planes [E, T, 2, 4] =
    (n_x, n_y, right-hand side, slot; -1 and zeros: absent), avoid_duals [E, 2T+1]: the 2T avoidance rows in step order, then -eps <= 0];
    obj includes the slack's cost.  (A module function: Context's public methods are a pinned record, tests/test_runtime_calls.py.)"""
    return _mpc_qp(ctx, ctx.lib.f1p_stmpc_qp_avoid_batch, 7, "x", 10, x0, ref, cfg, oa_prev, od_v_prev, opts, want_u, want_x, want_obj, want_duals,
                   want_iters, (obs, avoid, want_eps, want_planes, want_avoid_duals))


def stmpc_qp_set_avoid(ctx, avoid):
    """f1p_stmpc_qp_set_avoid on Context `ctx`, a switch of its own beside kmpc_qp_set_avoid: while on, stmpc_qp_plan, stmpc_qp_plan_tracks
    and stmpc_qp_dev take the discs of stmpc_set_obstacles[_dev] (the caller's ego order) as soft half-plane rows of both branches' QPs;
    avoid: _abi.kmpc_qp_avoid(...), None (or on=False) turns it off"""
    ctx._check(ctx.lib.f1p_stmpc_qp_set_avoid(ctx.h, _ref(avoid)))


def stmpc_qp_walls(ctx, x0, ref, obs, cfg, avoid=None, walls=None, oa_prev=None, od_v_prev=None, opts=None, want_u=True, want_x=False, want_obj=True,
                   want_duals=False, want_iters=True, want_eps=True, want_planes=False, want_avoid_duals=False):
    """stmpc_qp_avoid with wall rows from the context's ACTIVE occupancy bitmap (f1p_stmpc_qp_walls_batch): per step the two
    nearest of {the two nearest live discs, the wall to the left of the previous solution's path, the wall to its right} become the step's
    rows; left and right of the direction of travel yaw + beta.  obs [E, M, 5] with M in 0..16, or None (no discs); walls:
    _abi.kmpc_qp_walls(n_samples, margin) (None: the defaults).  Needs set_grid and no oriented footprint; horizon <=
    _abi.STMPC_QP_AVOID_MAX_T.  -> stmpc_qp_avoid's dict; planes' slot 16 / 17: the left / right wall.  (A module function, as kmpc_qp_walls.)"""
    if obs is None:
        obs = np.zeros((_f64(x0, (-1, 7)).shape[0], 0, 5))
    return _mpc_qp(ctx, ctx.lib.f1p_stmpc_qp_walls_batch, 7, "x", 10, x0, ref, cfg, oa_prev, od_v_prev, opts, want_u, want_x, want_obj, want_duals,
                   want_iters, (obs, avoid, want_eps, want_planes, want_avoid_duals), walls=(_ref(walls),))


def stmpc_qp_set_walls(ctx, walls):
    """f1p_stmpc_qp_set_walls on Context `ctx`, a switch of its own beside kmpc_qp_set_walls: while on, stmpc_qp_plan, stmpc_qp_plan_tracks
    and stmpc_qp_dev solve the wall problem in both branches on the grid the context holds at each call, with the discs of
    stmpc_set_obstacles[_dev] while stmpc_qp_set_avoid is on as well (else none) and its rho / lin; walls: _abi.kmpc_qp_walls(...), None (or
    on=False) turns it off"""
    ctx._check(ctx.lib.f1p_stmpc_qp_set_walls(ctx.h, _ref(walls)))


def _mpc_qp(ctx, fn, n, xname, duals_per_step, x0, ref, cfg, oa_prev, od_prev, opts, want_u, want_x, want_obj, want_duals, want_iters, av=None,
            walls=()):
    """the stateless QP calls (Context.kmpc_qp / stmpc_qp, kmpc_qp_avoid / stmpc_qp_avoid, kmpc_qp_walls / stmpc_qp_walls).  n: the state width; xname: the key
    of the predicted states [E, n, T+1]; duals [E, duals_per_step * T - 2]; av: None, or the avoidance rows' (obs, avoid, want_eps,
    want_planes, want_avoid_duals); walls: the arguments that follow `avoid` (kmpc_qp_walls / stmpc_qp_walls: the struct), where obs may be [E, 0, 5]"""
    x0 = _f64(x0, (-1, n)); E = x0.shape[0]; T = cfg.horizon
    ref = _f64(ref, (E, n, T + 1))
    wants = [("u", want_u, (E, T, 2), np.float64), (xname, want_x, (E, n, T + 1), np.float64), ("obj", want_obj, (E,), np.float64),
             ("duals", want_duals, (E, duals_per_step * T - 2), np.float64), ("iters", want_iters, (E,), np.int32)]
    av_in, av_keys = (), ()
    if av is not None:
        obs, avoid, want_eps, want_planes, want_avoid_duals = av
        o = _f64(obs)
        if o.ndim != 3 or o.shape[0] != E or o.shape[2] != 5:
            raise ValueError(f"obstacles must be [E={E}, M, 5] = (x, y, vx, vy, r)")
        wants += [("eps", want_eps, (E,), np.float64), ("planes", want_planes, (E, T, 2, 4), np.float64),
                  ("avoid_duals", want_avoid_duals, (E, 2 * T + 1), np.float64)]
        av_in, av_keys = (None if walls and not o.size else _ptr(o), o.shape[1], _ref(avoid), *walls), ("eps", "planes", "avoid_duals")
    oa = None if oa_prev is None else _f64(oa_prev, (E, T))
    od = None if od_prev is None else _f64(od_prev, (E, T))
    out = dict(steer=np.empty(E), speed=np.empty(E), status=np.empty(E, np.int32))
    for k, want, shape, dt in wants:
        if want:
            out[k] = np.empty(shape, dt)
    ctx._check(fn(ctx.h, _ptr(x0), _ptr(ref), _ptr(oa), _ptr(od), E, C.byref(cfg), _ref(opts), *av_in, _ptr(out["steer"]), _ptr(out["speed"]),
                  _ptr(out["status"]), _ptr(out.get("u")), _ptr(out.get(xname)), _ptr(out.get("obj")), _ptr(out.get("duals")),
                  _ptr(out.get("iters")), *(_ptr(out.get(k)) for k in av_keys)))
    return out


class _Mpc:
    # ---- MPC: the kinematic (kmpc_*, state width 4) and the dynamic (stmpc_*, 7) wrappers share their bodies -----------------------
    def kmpc_ref(self, states, horizon, dt=0.1, dl=0.03):
        return self._kmpc_ref(states, horizon, dt, dl)

    def kmpc_ref_tracks(self, states, track_ids, horizon, dt=0.1, dl=0.03):
        return self._kmpc_ref(states, horizon, dt, dl, _tid(track_ids))

    def stmpc_ref(self, states, horizon, dt=0.025, dl=0.03):
        return self._stmpc_ref(states, horizon, dt, dl)

    def stmpc_ref_tracks(self, states, track_ids, horizon, dt=0.025, dl=0.03):
        """stmpc_ref on each ego's track -> ref [E, 7, T+1] (a bad id: NaN rows).  With (TK, DTK, dlk), rows [0, 1, 3, 4] are STMPC's
        kinematic reference, for kmpc_shoot; the full rows go to stmpc_shoot."""
        return self._stmpc_ref(states, horizon, dt, dl, _tid(track_ids))

    def _kmpc_ref(self, states, horizon, dt, dl, ids=None):
        return self._mpc_ref(self.lib.f1p_kmpc_ref_batch, self.lib.f1p_kmpc_ref_tracks_batch, 4, states, horizon, dt, dl, ids)

    def _stmpc_ref(self, states, horizon, dt, dl, ids=None):
        return self._mpc_ref(self.lib.f1p_stmpc_ref_batch, self.lib.f1p_stmpc_ref_tracks_batch, 7, states, horizon, dt, dl, ids)

    def _mpc_ref(self, plain, tracks, n, states, horizon, dt, dl, ids):
        st = _f64(states, (-1, 4)); E = st.shape[0]; ids = None if ids is None else self._ids(ids, E)
        ref = np.empty((E, n, horizon + 1))
        fn, tid = _pick(plain, tracks, ids)
        self._check(fn(self.h, _ptr(st), *tid, E, int(horizon), float(dt), float(dl), _ptr(ref)))
        return ref

    def kmpc_ref_tracks_dev(self, d_states, d_track_ids, E, horizon, d_ref, dt=0.1, dl=0.03):
        self._mpc_ref_tracks_dev(self.lib.f1p_kmpc_ref_tracks_dev, d_states, d_track_ids, E, horizon, d_ref, dt, dl)

    def stmpc_ref_tracks_dev(self, d_states, d_track_ids, E, horizon, d_ref, dt=0.025, dl=0.03):
        self._mpc_ref_tracks_dev(self.lib.f1p_stmpc_ref_tracks_dev, d_states, d_track_ids, E, horizon, d_ref, dt, dl)

    def _mpc_ref_tracks_dev(self, fn, d_states, d_track_ids, E, horizon, d_ref, dt, dl):
        self._check(fn(self.h, _dev(d_states), _dev(d_track_ids), int(E), int(horizon), float(dt), float(dl), _dev(d_ref)))

    def kmpc_set_mode(self, mixed=True, d_cost32=None, d_n_refined=None):
        """mixed: f32 filter + fp64 refinement (default) or plain fp64; optional device buffers receive the filter diagnostics"""
        self._check(self.lib.f1p_kmpc_set_mode(self.h, 1 if mixed else 0, None if d_cost32 is None else d_cost32.ptr,
                                               None if d_n_refined is None else d_n_refined.ptr))

    def stmpc_set_mode(self, mixed=True, d_cost32=None, d_n_refined=None):
        """f32 filter + fp64 decision (default) or plain fp64 for the dynamic single-track shooting; the buffers are test hooks"""
        self._check(self.lib.f1p_stmpc_set_mode(self.h, 1 if mixed else 0, None if d_cost32 is None else d_cost32.ptr,
                                                None if d_n_refined is None else d_n_refined.ptr))

    def kmpc_predict(self, x0, oa, od, cfg: KmpcCfg):
        """predict_motion_kinematic (kinematic_mpc.py:208-221) for E egos -> path [E, 4, T+1]"""
        return self._mpc_predict(self.lib.f1p_kmpc_predict_batch, 4, x0, oa, od, cfg)

    def stmpc_predict(self, x0, oa, od_v, cfg):
        """predict_motion (dynamic_mpc.py:280-300) for E egos -> path [E, 7, T+1]"""
        return self._mpc_predict(self.lib.f1p_stmpc_predict_batch, 7, x0, oa, od_v, cfg)

    def _mpc_predict(self, fn, n, x0, oa, od, cfg):
        x0 = _f64(x0, (-1, n)); E = x0.shape[0]; T = cfg.horizon
        oa = _f64(oa, (E, T)); od = _f64(od, (E, T))
        path = np.empty((E, n, T + 1))
        self._check(fn(self.h, _ptr(x0), _ptr(oa), _ptr(od), E, C.byref(cfg), _ptr(path)))
        return path

    # ---- MPC, random shooting (the dynamic single-track model: SURVEY 8f rank 2) -----------------------------------------------------
    def kmpc_shoot(self, x0, ref, controls, cfg: KmpcCfg, want_seq=True):
        return self._mpc_shoot(self.lib.f1p_kmpc_shoot_batch, 4, x0, ref, controls, cfg, want_seq)

    def stmpc_shoot(self, x0, ref, controls, cfg, want_seq=True):
        return self._mpc_shoot(self.lib.f1p_stmpc_shoot_batch, 7, x0, ref, controls, cfg, want_seq)

    def _mpc_shoot(self, fn, n, x0, ref, controls, cfg, want_seq):
        x0 = _f64(x0, (-1, n)); E = x0.shape[0]; T = cfg.horizon; R = cfg.n_rollouts
        ref = _f64(ref, (E, n, T + 1))
        controls = np.ascontiguousarray(controls, dtype=np.float32)
        if controls.shape != (E, T, 2, R):
            raise ValueError(f"controls must be f32 [E={E}, T={T}, 2, R={R}]")
        out = dict(steer=np.empty(E), speed=np.empty(E), best_idx=np.empty(E, np.int32), best_cost=np.empty(E))
        if want_seq:
            out["best_seq"] = np.empty((E, T, 2))
        self._check(fn(self.h, _ptr(x0), _ptr(ref), _ptr(controls), E, C.byref(cfg), _ptr(out["steer"]), _ptr(out["speed"]),
                       _ptr(out["best_idx"]), _ptr(out["best_cost"]), _ptr(out.get("best_seq"))))
        return out

    def kmpc_shoot_dev(self, d_x0, d_ref, d_controls, E, cfg: KmpcCfg, d_steer, d_speed, d_best_idx, d_best_cost=None,
                       d_best_seq=None):
        self._mpc_shoot_dev(self.lib.f1p_kmpc_shoot_dev, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq)

    def stmpc_shoot_dev(self, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost=None, d_best_seq=None):
        """Asynchronous launch on HBM-resident buffers: x0 [E][7], ref [E][7][T+1], controls f32 [E][T][2][R]."""
        self._mpc_shoot_dev(self.lib.f1p_stmpc_shoot_dev, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq)

    def _mpc_shoot_dev(self, fn, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq):
        self._check(fn(self.h, _dev(d_x0), _dev(d_ref), _dev(d_controls), int(E), C.byref(cfg), _dev(d_steer), _dev(d_speed),
                       _dev(d_best_idx), _dev(d_best_cost), _dev(d_best_seq)))

    # in-kernel control generation + device-resident warm start (f1p_kmpc_plan_*)
    def kmpc_plan(self, x0, cfg: KmpcCfg, sampler, dl=0.03, want_seq=True, want_cost=True):
        """KMPCPlanner.plan for E egos in ONE call: reference extraction, sampling around the ctx's warm start, rollouts,
        argmin, new warm start -- nothing but x0 goes up and the winners come down."""
        x0 = _f64(x0, (-1, 4)); E = x0.shape[0]; T = cfg.horizon
        out = dict(steer=np.empty(E), speed=np.empty(E), best_idx=np.empty(E, np.int32))
        if want_cost:
            out["best_cost"] = np.empty(E)
        if want_seq:
            out["best_seq"] = np.empty((E, T, 2))
        self._check(self.lib.f1p_kmpc_plan_batch(self.h, _ptr(x0), E, C.byref(cfg), float(dl), C.byref(sampler), _ptr(out["steer"]),
                                                 _ptr(out["speed"]), _ptr(out["best_idx"]), _ptr(out.get("best_cost")), _ptr(out.get("best_seq"))))
        return out

    def stmpc_plan(self, x0, dcfg, kcfg: KmpcCfg, sampler, v_ks=2.0, dl=0.03, dlk=0.03, want_seq=True, want_cost=True):
        """STMPCPlanner.plan with the shooting solver for E egos in ONE call: x0 [E, 7]; per ego the kinematic model at v <= v_ks, the
        dynamic one above; reference extraction, generation around the ego's warm start, rollouts, argmin, new warm start ->
        dict(steer, speed, best_idx, branch (1 dynamic, 0 kinematic)[, best_cost][, best_seq [E, max(T, TK), 2] in the branch's channel
        order, NaN past its horizon])"""
        x0 = _f64(x0, (-1, 7)); E = x0.shape[0]; W = max(dcfg.horizon, kcfg.horizon)
        out = dict(steer=np.empty(E), speed=np.empty(E), best_idx=np.empty(E, np.int32), branch=np.empty(E, np.int32))
        if want_cost:
            out["best_cost"] = np.empty(E)
        if want_seq:
            out["best_seq"] = np.empty((E, W, 2))
        self._check(self.lib.f1p_stmpc_plan_batch(self.h, _ptr(x0), E, C.byref(dcfg), C.byref(kcfg), float(v_ks), float(dl), float(dlk),
                                                  C.byref(sampler), _ptr(out["steer"]), _ptr(out["speed"]), _ptr(out["best_idx"]),
                                                  _ptr(out.get("best_cost")), _ptr(out["branch"]), _ptr(out.get("best_seq"))))
        return out

    def kmpc_plan_dev(self, d_x0, d_ref, E, cfg: KmpcCfg, sampler, d_steer, d_speed, d_best_idx, d_best_cost=None, d_best_seq=None):
        self._mpc_plan_dev(self.lib.f1p_kmpc_plan_dev, d_x0, d_ref, E, cfg, sampler, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq)

    def stmpc_plan_dev(self, d_x0, d_ref, E, cfg, sampler, d_steer, d_speed, d_best_idx, d_best_cost=None, d_best_seq=None):
        """Asynchronous: the dynamic model's shooting plan of E egos on a given reference (x0 [E][7], ref [E][7][T+1]), the controls
        generated in the kernels around the ctx's warm start, which it updates."""
        self._mpc_plan_dev(self.lib.f1p_stmpc_plan_dev, d_x0, d_ref, E, cfg, sampler, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq)

    def _mpc_plan_dev(self, fn, d_x0, d_ref, E, cfg, sampler, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq):
        self._check(fn(self.h, _dev(d_x0), _dev(d_ref), int(E), C.byref(cfg), C.byref(sampler), _dev(d_steer), _dev(d_speed),
                       _dev(d_best_idx), _dev(d_best_cost), _dev(d_best_seq)))

    def kmpc_gen_controls_dev(self, d_controls, E, cfg: KmpcCfg, sampler):
        self._check(self.lib.f1p_kmpc_gen_controls_dev(self.h, d_controls.ptr, int(E), C.byref(cfg), C.byref(sampler)))

    # in-kernel control generation + per-ego device-resident warm start (f1p_stmpc_plan_*)
    def stmpc_gen_controls_dev(self, d_controls, E, cfg, sampler):
        """The controls the next stmpc_plan_dev of this shape would evaluate, as the f32 [E][T][2][R] buffer stmpc_shoot_dev takes."""
        self._check(self.lib.f1p_stmpc_gen_controls_dev(self.h, d_controls.ptr, int(E), C.byref(cfg), C.byref(sampler)))

    def kmpc_sample_controls_dev(self, d_controls, E, cfg: KmpcCfg, seed, sigma_accel=1.5, sigma_steer=0.15):
        self._check(self.lib.f1p_kmpc_sample_controls_dev(self.h, d_controls.ptr, int(E), C.byref(cfg),
                                                          C.c_uint64(int(seed)), float(sigma_accel), float(sigma_steer)))

    def kmpc_warm_reset(self):
        self._check(self.lib.f1p_kmpc_warm_reset(self.h))

    def kmpc_warm_get(self, E, T):
        w = np.empty((int(E), int(T), 2), np.float32)
        self._check(self.lib.f1p_kmpc_warm_get(self.h, _ptr(w), int(E), int(T)))
        return w

    def kmpc_warm_set(self, warm):
        w = np.ascontiguousarray(warm, np.float32)
        self._check(self.lib.f1p_kmpc_warm_set(self.h, _ptr(w), w.shape[0], w.shape[1]))

    def kmpc_set_yaw_fixup(self, on=True):
        """k_kmpc_ref's per-ego heading fold (kinematic_mpc.py:198-203) on the gathered values; off = the caller maintains the array"""
        self._check(self.lib.f1p_kmpc_set_yaw_fixup(self.h, 1 if on else 0))

    def kmpc_set_groups(self, groups=0):
        self._check(self.lib.f1p_kmpc_set_groups(self.h, int(groups)))

    def kmpc_set_collision(self, on=True, n_sub=1):
        """test the shooting solver's rollouts against the occupancy grid at n_sub points per time step (f1p_kmpc_set_collision): a
        blocked rollout cannot win; an ego whose rollouts are all blocked gets best_idx -1, cost +inf, steer 0, speed 0"""
        self._check(self.lib.f1p_kmpc_set_collision(self.h, 1 if on else 0, int(n_sub)))

    def _set_obstacles(self, name, obs):
        fn = getattr(self.lib, name)
        if obs is None:
            self._check(fn(self.h, None, 0, 0))
            return
        o = _f64(obs)
        if o.ndim != 3 or o.shape[2] != 5:
            raise ValueError("obstacles must be [E, M, 5] = (x, y, vx, vy, r)")
        self._check(fn(self.h, _ptr(o), o.shape[0], o.shape[1]))

    def _set_obstacles_dev(self, name, d_obs, E, M):
        if d_obs is not None and (E is None or M is None):
            raise ValueError("a device array of obstacles needs its E and M")
        fn = getattr(self.lib, name)
        if d_obs is None:
            self._check(fn(self.h, None, 0, 0))
            return
        self._check(fn(self.h, _dev(d_obs), int(E), int(M)))

    def _kmpc_set_obstacles(self, obs):
        _Mpc._set_obstacles(self, "f1p_kmpc_set_obstacles", obs)

    def _kmpc_set_obstacles_dev(self, d_obs, E=None, M=None):
        _Mpc._set_obstacles_dev(self, "f1p_kmpc_set_obstacles_dev", d_obs, E, M)

    def _stmpc_set_obstacles(self, obs):
        _Mpc._set_obstacles(self, "f1p_stmpc_set_obstacles", obs)

    def _stmpc_set_obstacles_dev(self, d_obs, E=None, M=None):
        _Mpc._set_obstacles_dev(self, "f1p_stmpc_set_obstacles_dev", d_obs, E, M)

    def stmpc_set_collision(self, on=True, n_sub=1, n_sub_k=2):
        """test the dynamic MPC's shooting rollouts against the occupancy grid (f1p_stmpc_set_collision): n_sub points per step of the
        dynamic model, n_sub_k per step of stmpc_plan's kinematic branch; a blocked rollout cannot win; an ego whose rollouts are all
        blocked gets best_idx -1, cost +inf, steer 0, speed 0, a zero sequence and a zero warm start.  Separate from kmpc_set_collision."""
        self._check(self.lib.f1p_stmpc_set_collision(self.h, 1 if on else 0, int(n_sub), int(n_sub_k)))

    def stmpc_warm_reset(self):
        self._check(self.lib.f1p_stmpc_warm_reset(self.h))

    def stmpc_warm_get(self, E, T, TK=0):
        """-> (warm f32 [E, max(T, TK), 2], tag [E]: 0 none, 1 kinematic (accel, steer), 2 dynamic (steering speed, accel))"""
        w = np.empty((int(E), max(int(T), int(TK)), 2), np.float32); tag = np.empty(int(E), np.int32)
        self._check(self.lib.f1p_stmpc_warm_get(self.h, _ptr(w), _ptr(tag), int(E), int(T), int(TK)))
        return w, tag

    def stmpc_warm_set(self, warm, tags, T, TK=0):
        w = np.ascontiguousarray(warm, np.float32); tag = np.ascontiguousarray(tags, dtype=np.int32)
        if w.ndim != 3 or w.shape[1:] != (max(int(T), int(TK)), 2) or tag.shape != (w.shape[0],):
            raise ValueError("warm must be [E, max(T, TK), 2] and tags [E]")
        self._check(self.lib.f1p_stmpc_warm_set(self.h, _ptr(w), _ptr(tag), w.shape[0], int(T), int(TK)))

    # ---- MPC, the reference's linearised QPs (f1p_kmpc_qp_*, f1p_stmpc_qp_*) ---------------------------------------------------------
    def kmpc_qp(self, x0, ref, cfg: KmpcCfg, oa_prev=None, od_prev=None, opts=None, want_u=True, want_xk=False, want_obj=True,
                want_duals=False, want_iters=True):
        """linear_mpc_control_kinematic (kinematic_mpc.py:452-475) solved exactly for E egos: x0 [E, 4], ref [E, 4, T+1], the previous
        solution oa_prev / od_prev [E, T] (None: zeros) -> dict(steer, speed, status[, u [E, T, 2], xk [E, 4, T+1], obj, duals [E, 8T-2],
        iters]).  status: 0 solved, 1 infeasible, 2 not converged, 3 non-finite input (1 and 3: NaN outputs)."""
        return _mpc_qp(self, self.lib.f1p_kmpc_qp_batch, 4, "xk", 8, x0, ref, cfg, oa_prev, od_prev, opts, want_u, want_xk, want_obj, want_duals,
                       want_iters)

    def stmpc_qp(self, x0, ref, cfg: _abi.StmpcCfg, oa_prev=None, od_v_prev=None, opts=None, want_u=True, want_x=False, want_obj=True,
                 want_duals=False, want_iters=True):
        """linear_mpc_control (dynamic_mpc.py:995-1040) solved exactly for E egos: x0 [E, 7], ref [E, 7, T+1], the previous solution
        oa_prev / od_v_prev [E, T] (None: zeros) -> dict(steer, speed, status[, u [E, T, 2] (steering speed, accel), x [E, 7, T+1], obj,
        duals [E, 10T-2], iters]).  status: 0 solved, 1 infeasible, 2 not converged, 3 non-finite input or model data (1, 3: NaN outputs)."""
        return _mpc_qp(self, self.lib.f1p_stmpc_qp_batch, 7, "x", 10, x0, ref, cfg, oa_prev, od_v_prev, opts, want_u, want_x, want_obj,
                       want_duals, want_iters)

    def kmpc_qp_dev(self, d_x0, d_ref, E, cfg: KmpcCfg, d_steer, d_speed, d_status, d_oa_prev=None, d_od_prev=None, opts=None, d_u=None,
                    d_xk=None, d_obj=None, d_duals=None, d_iters=None):
        self._mpc_qp_dev(self.lib.f1p_kmpc_qp_dev, d_x0, d_ref, E, cfg, d_steer, d_speed, d_status, d_oa_prev, d_od_prev, opts, d_u, d_xk,
                         d_obj, d_duals, d_iters)

    def stmpc_qp_dev(self, d_x0, d_ref, E, cfg: _abi.StmpcCfg, d_steer, d_speed, d_status, d_oa_prev=None, d_od_v_prev=None, opts=None, d_u=None,
                     d_x=None, d_obj=None, d_duals=None, d_iters=None):
        self._mpc_qp_dev(self.lib.f1p_stmpc_qp_dev, d_x0, d_ref, E, cfg, d_steer, d_speed, d_status, d_oa_prev, d_od_v_prev, opts, d_u, d_x,
                         d_obj, d_duals, d_iters)

    def _mpc_qp_dev(self, fn, d_x0, d_ref, E, cfg, d_steer, d_speed, d_status, d_oa_prev, d_od_prev, opts, d_u, d_x, d_obj, d_duals, d_iters):
        self._check(fn(self.h, _dev(d_x0), _dev(d_ref), _dev(d_oa_prev), _dev(d_od_prev), int(E), C.byref(cfg), _ref(opts), _dev(d_steer),
                       _dev(d_speed), _dev(d_status), _dev(d_u), _dev(d_x), _dev(d_obj), _dev(d_duals), _dev(d_iters)))

    def kmpc_qp_plan(self, x0, cfg: KmpcCfg, dl=0.03, opts=None, want_u=True, want_obj=True):
        """KMPCPlanner.plan with the QP solver for E egos in ONE call: reference extraction, linearisation about the ctx's fp64 warm start
        (the previous call's solution, unshifted), solve, output map, new warm start -> dict(steer, speed, status[, u, obj])"""
        x0 = _f64(x0, (-1, 4)); E = x0.shape[0]; T = cfg.horizon
        out = dict(steer=np.empty(E), speed=np.empty(E), status=np.empty(E, np.int32))
        if want_u:
            out["u"] = np.empty((E, T, 2))
        if want_obj:
            out["obj"] = np.empty(E)
        self._check(self.lib.f1p_kmpc_qp_plan_batch(self.h, _ptr(x0), E, C.byref(cfg), float(dl), _ref(opts),
                                                    _ptr(out["steer"]), _ptr(out["speed"]), _ptr(out["status"]), _ptr(out.get("u")),
                                                    _ptr(out.get("obj"))))
        return out

    def stmpc_qp_plan(self, x0, dcfg: _abi.StmpcCfg, kcfg: KmpcCfg, v_ks=2.0, dl=0.03, dlk=0.03, opts=None, want_u=True, want_obj=True):
        """STMPCPlanner.plan with the QP solver for E egos in ONE call: x0 [E, 7]; per ego the kinematic branch at v <= v_ks, the dynamic
        one above; reference extraction, linearisation about the ctx's warm start (the reference's self.oa / self.odelta_v with its length
        rules), solve, output map -> dict(steer, speed, status, branch (1 dynamic, 0 kinematic)[, u [E, max(T, TK), 2] = the new
        (oa, odelta_v), NaN past the branch's horizon][, obj])"""
        return self._stmpc_qp_plan(x0, dcfg, kcfg, v_ks, dl, dlk, opts, want_u, want_obj)

    def stmpc_qp_plan_tracks(self, x0, track_ids, dcfg: _abi.StmpcCfg, kcfg: KmpcCfg, v_ks=2.0, dl=0.03, dlk=0.03, opts=None, want_u=True,
                             want_obj=True):
        """stmpc_qp_plan with ego e's references from track track_ids[e] of set_tracks; the same dict.  The warm start is the one of
        stmpc_qp_plan (it follows the ego, not the track).  A bad id: status F1P_ST_BAD_TRACK, branch -1, NaN outputs, its warm start
        untouched."""
        return self._stmpc_qp_plan(x0, dcfg, kcfg, v_ks, dl, dlk, opts, want_u, want_obj, _tid(track_ids))

    def _stmpc_qp_plan(self, x0, dcfg, kcfg, v_ks, dl, dlk, opts, want_u, want_obj, ids=None):
        x0 = _f64(x0, (-1, 7)); E = x0.shape[0]; ids = None if ids is None else self._ids(ids, E); W = max(dcfg.horizon, kcfg.horizon)
        out = dict(steer=np.empty(E), speed=np.empty(E), status=np.empty(E, np.int32), branch=np.empty(E, np.int32))
        if want_u:
            out["u"] = np.empty((E, W, 2))
        if want_obj:
            out["obj"] = np.empty(E)
        fn, tid = _pick(self.lib.f1p_stmpc_qp_plan_batch, self.lib.f1p_stmpc_qp_plan_tracks_batch, ids)
        self._check(fn(self.h, _ptr(x0), *tid, E, C.byref(dcfg), C.byref(kcfg), float(v_ks), float(dl), float(dlk), _ref(opts),
                       _ptr(out["steer"]), _ptr(out["speed"]), _ptr(out["status"]), _ptr(out["branch"]), _ptr(out.get("u")),
                       _ptr(out.get("obj"))))
        return out

    def kmpc_qp_warm_reset(self):
        self._check(self.lib.f1p_kmpc_qp_warm_reset(self.h))

    def kmpc_qp_warm_get(self, E, T):
        w = np.empty((int(E), int(T), 2))
        self._check(self.lib.f1p_kmpc_qp_warm_get(self.h, _ptr(w), int(E), int(T)))
        return w

    def kmpc_qp_warm_set(self, warm):
        w = _f64(warm)
        self._check(self.lib.f1p_kmpc_qp_warm_set(self.h, _ptr(w), w.shape[0], w.shape[1]))

    def kmpc_qp_set_pack(self, egos_per_wave=0):
        """egos per wave of the QP kernel at T <= 8 (0: default, 1 or 4)"""
        self._check(self.lib.f1p_kmpc_qp_set_pack(self.h, int(egos_per_wave)))

    def stmpc_qp_warm_reset(self):
        self._check(self.lib.f1p_stmpc_qp_warm_reset(self.h))

    def stmpc_qp_warm_get(self, E, W):
        """-> (warm [E, W, 2] = (oa, odelta_v), len [E]: the length of each ego's oa, 0 = None)"""
        w = np.empty((int(E), int(W), 2)); n = np.empty(int(E), np.int32)
        self._check(self.lib.f1p_stmpc_qp_warm_get(self.h, _ptr(w), _ptr(n), int(E), int(W)))
        return w, n

    def stmpc_qp_warm_set(self, warm, lengths):
        w = _f64(warm); n = np.ascontiguousarray(lengths, dtype=np.int32)
        self._check(self.lib.f1p_stmpc_qp_warm_set(self.h, _ptr(w), _ptr(n), w.shape[0], w.shape[1]))
