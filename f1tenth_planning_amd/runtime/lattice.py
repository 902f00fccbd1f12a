"""Context's lattice planner: plans, closed-loop steps, clothoids, schedule switches and test hooks (csrc/f1p_lattice.hip)."""
import ctypes as C

import numpy as np

from .._abi import LatticeCfg
from .core import _dev, _f64, _pick, _ptr, _tid


def lattice_set_obstacles(ctx, obs, pace=None):
    """moving discs for the lattice planner's candidates (f1p_lattice_set_obstacles) on Context `ctx`: obs [E, M, 5] fp64 rows
    (x, y, vx, vy, r), map frame, constant velocity, M <= 16, a row with r < 0 or NaN is empty; pace [E] in s/m (seconds per metre of path: station j
    of a candidate is reached at s_j * pace).  They stay until the next set; None clears.  (The public face of Context._lattice_set_obstacles:
    Context's public methods are a pinned record, tests/test_runtime_calls.py.)"""
    ctx._lattice_set_obstacles(obs, pace)


def lattice_set_obstacles_dev(ctx, d_obs, d_pace=None, E=None, M=None):
    """lattice_set_obstacles on device buffers [E][M][5] and [E] fp64 that the context BORROWS: keep them alive, rewrite them in place between
    plans.  None clears."""
    ctx._lattice_set_obstacles_dev(d_obs, d_pace, E, M)


class _Lattice:
    def _lattice_set_obstacles(self, obs, pace):
        if obs is None:
            self._check(self.lib.f1p_lattice_set_obstacles(self.h, None, None, 0, 0))
            return
        o = _f64(obs)
        if o.ndim != 3 or o.shape[2] != 5:
            raise ValueError("obstacles must be [E, M, 5] = (x, y, vx, vy, r)")
        if pace is None:
            raise ValueError("lattice obstacles need a pace [E] in s/m")
        p = _f64(pace).reshape(-1)
        if p.shape[0] != o.shape[0]:
            raise ValueError(f"pace must be [E={o.shape[0]}]")
        self._check(self.lib.f1p_lattice_set_obstacles(self.h, _ptr(o), _ptr(p), o.shape[0], o.shape[1]))

    def _lattice_set_obstacles_dev(self, d_obs, d_pace, E, M):
        if d_obs is None:
            self._check(self.lib.f1p_lattice_set_obstacles_dev(self.h, None, None, 0, 0))
            return
        if d_pace is None or E is None or M is None:
            raise ValueError("device arrays of obstacles need their paces, E and M")
        self._check(self.lib.f1p_lattice_set_obstacles_dev(self.h, _dev(d_obs), _dev(d_pace), int(E), int(M)))

    # ---- lattice -------------------------------------------------------------------------------------------
    def lattice_plan(self, poses, cfg: LatticeCfg, goals=None, prev_theta=None, want_traj=True, want_all=False,
                     reuse_outputs=False, traj_dtype=np.float64):
        """reuse_outputs: results land in page-locked arrays owned by the context (no bounce buffers, no fresh pages per
        call); they are overwritten by the next call with the same batch shape.
        traj_dtype=np.float32: best_traj comes back as f32 rows (f1p_lattice_plan_batch_f32: the fp64 rows rounded once on the
        device, half the PCIe bytes); everything else is unchanged."""
        return self._lattice_plan(poses, cfg, goals, prev_theta, want_traj, want_all, reuse_outputs, traj_dtype, None)

    def lattice_plan_tracks(self, poses, track_ids, cfg: LatticeCfg, goals=None, prev_theta=None, want_traj=True, want_all=False,
                            reuse_outputs=False, traj_dtype=np.float64):
        """lattice_plan on the track set (set_tracks): ego e plans along track track_ids[e], bit-identical to lattice_plan on a context
        whose raceline is that track.  An id outside [0, K): NaN steer / speed / best_cost, best_idx and near_idx -1, status
        F1P_ST_BAD_TRACK, zero rows."""
        E = int(np.shape(poses)[0])
        return self._lattice_plan(poses, cfg, goals, prev_theta, want_traj, want_all, reuse_outputs, traj_dtype, self._ids(track_ids, E))

    def _lattice_plan(self, poses, cfg, goals, prev_theta, want_traj, want_all, reuse_outputs, traj_dtype, ids):
        f32 = np.dtype(traj_dtype) == np.float32
        if f32 and want_all:
            raise ValueError("traj_dtype=float32 is a winner-only mode (no all_cost / all_traj)")
        poses = _f64(poses, (-1, 4)); E = poses.shape[0]; Cn = cfg.n_cand; S = cfg.n_stations
        g = None if goals is None else _f64(goals, (E, Cn, 3))
        pt = None if prev_theta is None else _f64(prev_theta, (E, S))
        ptrs = None
        if reuse_outputs:
            # the page-locked arrays of this batch shape and their addresses are looked up ONCE (eight pinned() look-ups and nine ctypes pointer objects were
            # ~15 us of a 0.22 ms call)
            key = ("plan", E, S, f32, bool(want_traj))
            b = self._bundles.get(key)
            if b is None:
                pin = self.pinned
                hp = pin("lat_poses", (E, 4), np.float64)
                o = dict(steer=pin("lat_steer", E, np.float64), speed=pin("lat_speed", E, np.float64),
                         best_idx=pin("lat_bidx", E, np.int32), best_cost=pin("lat_bcost", E, np.float64),
                         status=pin("lat_status", E, np.int32), near_idx=pin("lat_near", E, np.int32))
                if want_traj:
                    o["best_traj"] = pin("lat_traj32" if f32 else "lat_traj", (E, S, 4), np.float32 if f32 else np.float64)
                b = self._bundles[key] = (hp, o, {k: _ptr(v) for k, v in o.items()}, _ptr(hp))
            hp, o, ptrs, php = b
            hp[...] = poses; poses = hp
            out = dict(o)
            if ids is not None:                # (page-locked too: the kernels read them in place)
                hi = self.pinned("lat_tid", E, np.int32)
                hi[...] = ids; ids = hi
        else:
            # fresh arrays for the caller: the six result columns are views of ONE buffer, so that one address look-up (1.5 us each) serves all of them
            cols = np.empty(36 * E + 8, np.uint8)
            base = cols.__array_interface__["data"][0]
            o8, o4 = 8 * E, 4 * E
            out = dict(steer=cols[0:o8].view(np.float64), speed=cols[o8:2 * o8].view(np.float64), best_cost=cols[2 * o8:3 * o8].view(np.float64),
                       best_idx=cols[3 * o8:3 * o8 + o4].view(np.int32), status=cols[3 * o8 + o4:3 * o8 + 2 * o4].view(np.int32),
                       near_idx=cols[3 * o8 + 2 * o4:3 * o8 + 3 * o4].view(np.int32))
            ptrs = dict(steer=C.c_void_p(base), speed=C.c_void_p(base + o8), best_cost=C.c_void_p(base + 2 * o8), best_idx=C.c_void_p(base + 3 * o8),
                        status=C.c_void_p(base + 3 * o8 + o4), near_idx=C.c_void_p(base + 3 * o8 + 2 * o4))
            php = None
            if want_traj:
                out["best_traj"] = np.empty((E, S, 4), np.float32 if f32 else np.float64)
                ptrs["best_traj"] = _ptr(out["best_traj"])
        if want_all:
            out["all_cost"] = np.empty((E, Cn)); out["all_traj"] = np.empty((E, Cn, S, 4))
        if cfg.cand_count > 0:            # a candidate shard only evaluates: (best_idx, best_cost, near_idx)
            for k in ("steer", "speed", "status", "best_traj"):
                out.pop(k, None)
        if ptrs is not None and not want_all:
            P = lambda k: ptrs[k] if k in out else None   # noqa: E731
            pp = php if php is not None else _ptr(poses)
        else:
            P = lambda k: _ptr(out.get(k))                # noqa: E731
            pp = _ptr(poses)
        lib = self.lib
        if f32:                            # (winner-only: the f32 entry points take no all_cost / all_traj)
            fn, tid = _pick(lib.f1p_lattice_plan_batch_f32, lib.f1p_lattice_plan_tracks_batch_f32, ids)
            every = ()
        else:
            fn, tid = _pick(lib.f1p_lattice_plan_batch, lib.f1p_lattice_plan_tracks_batch, ids)
            every = (_ptr(out.get("all_cost")), _ptr(out.get("all_traj")))
        self._check(fn(self.h, pp, _ptr(g), _ptr(pt), *tid, E, C.byref(cfg),
                       P("steer"), P("speed"), P("best_idx"), P("best_cost"), P("status"), P("near_idx"), P("best_traj"), *every))
        return out

    def lattice_plan_dev(self, d_poses, E, cfg: LatticeCfg, d_steer, d_speed, d_best_idx, d_best_cost=None, d_status=None,
                         d_near_idx=None, d_best_traj=None, d_goals=None, d_prev_theta=None, d_all_cost=None,
                         d_all_traj=None):
        """Asynchronous launch on HBM-resident buffers (DeviceBuffer or None)."""
        self._lattice_plan_dev((), d_poses, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx, d_best_traj, d_goals,
                               d_prev_theta, d_all_cost, d_all_traj)

    def lattice_plan_tracks_dev(self, d_poses, d_track_ids, E, cfg: LatticeCfg, d_steer, d_speed, d_best_idx, d_best_cost=None, d_status=None,
                                d_near_idx=None, d_best_traj=None, d_goals=None, d_prev_theta=None, d_all_cost=None, d_all_traj=None):
        """lattice_plan_dev on the track set: ego e on track d_track_ids[e] ([E] int32 on the device); asynchronous."""
        self._lattice_plan_dev((_dev(d_track_ids),), d_poses, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx,
                               d_best_traj, d_goals, d_prev_theta, d_all_cost, d_all_traj)

    def _lattice_plan_dev(self, tid, d_poses, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx, d_best_traj, d_goals,
                          d_prev_theta, d_all_cost, d_all_traj):
        """tid: () or (the track ids' device pointer,)"""
        fn = self.lib.f1p_lattice_plan_tracks_dev if tid else self.lib.f1p_lattice_plan_dev
        self._check(fn(self.h, _dev(d_poses), _dev(d_goals), _dev(d_prev_theta), *tid, int(E), C.byref(cfg), _dev(d_steer), _dev(d_speed),
                       _dev(d_best_idx), _dev(d_best_cost), _dev(d_status), _dev(d_near_idx), _dev(d_best_traj), _dev(d_all_cost),
                       _dev(d_all_traj)))

    def lattice_step(self, poses, cfg: LatticeCfg, keep_traj=False):
        """One closed-loop control step (f1p_lattice_step_batch): poses [E, 4] -> dict(steer, speed, status), page-locked arrays owned by
        the context (overwritten by the next step of the same batch size).  The previous plan's headings (similarity term) stay on the
        device; keep_traj=True keeps the winners' rows there too (lattice_fetch_traj)."""
        return self._lattice_step(poses, cfg, keep_traj)

    def lattice_step_tracks(self, poses, track_ids, cfg: LatticeCfg, keep_traj=False):
        """lattice_step on the track set (f1p_lattice_step_tracks_batch): ego e on track track_ids[e]; the chain as lattice_step's."""
        return self._lattice_step(poses, cfg, keep_traj, _tid(track_ids))

    def _lattice_step(self, poses, cfg, keep_traj, ids=None):
        E = int(np.shape(poses)[0])
        if ids is not None:
            ids = self._ids(ids, E)
        b = self._bundles.get(("step", E))
        if b is None:
            hp = self.pinned("step_poses", (E, 4), np.float64)
            o = dict(steer=self.pinned("step_steer", E, np.float64), speed=self.pinned("step_speed", E, np.float64),
                     status=self.pinned("step_status", E, np.int32))
            b = self._bundles[("step", E)] = (hp, o, (_ptr(hp), _ptr(o["steer"]), _ptr(o["speed"]), _ptr(o["status"])))
        hp, o, (php, ps, pv, pt) = b
        hp[...] = poses
        fn, tid = self.lib.f1p_lattice_step_batch, ()
        if ids is not None:                # (page-locked like the poses: the kernels read them in place)
            hi = self.pinned("step_tid", E, np.int32)
            hi[...] = ids
            fn, tid = self.lib.f1p_lattice_step_tracks_batch, (_ptr(hi),)
        self._check(fn(self.h, php, *tid, E, C.byref(cfg), ps, pv, pt, 1 if keep_traj else 0))
        return dict(o)

    def lattice_fetch_traj(self, E, S):
        """the winners' rows [E, S, 4] of the last lattice_step(keep_traj=True)"""
        out = np.empty((int(E), int(S), 4))
        self._check(self.lib.f1p_lattice_fetch_traj(self.h, _ptr(out), int(E), int(S)))
        return out

    def clothoid_g1(self, goals):
        g = _f64(goals, (-1, 3)); n = g.shape[0]
        k0 = np.empty(n); dk = np.empty(n); L = np.empty(n); ok = np.empty(n, np.int32)
        self._check(self.lib.f1p_clothoid_g1_batch(self.h, _ptr(g), n, _ptr(k0), _ptr(dk), _ptr(L), _ptr(ok)))
        return k0, dk, L, ok.astype(bool)

    def clothoid_sample(self, params, npts):
        """params [n, 3] = (kappa0, dkappa, length) -> rows [n, npts, 4] (x, y, theta, |kappa|) in each clothoid's start frame"""
        p = _f64(params, (-1, 3)); n = p.shape[0]
        rows = np.empty((n, int(npts), 4))
        self._check(self.lib.f1p_clothoid_sample_batch(self.h, _ptr(p), n, int(npts), _ptr(rows)))
        return rows

    def lattice_set_closed_loop(self, on=True):
        """closed-loop mode: every plan's winning headings stay on the device and are the next plan's prev_theta (similarity cost,
        lattice_planner.py:287-296) whenever prev_theta is None; (re)arming forgets the previous path"""
        self._check(self.lib.f1p_lattice_set_closed_loop(self.h, 1 if on else 0))

    def lattice_closed_loop_prev(self):
        """the headings the NEXT closed-loop plan would use as prev_theta: numpy [E, S] (a copy), or None"""
        ptr = C.c_void_p(); E = C.c_int32(); S = C.c_int32()
        self._check(self.lib.f1p_lattice_closed_loop_state(self.h, C.byref(ptr), C.byref(E), C.byref(S)))
        if not ptr.value:
            return None
        out = np.empty((E.value, S.value))
        self._check(self.lib.f1p_d2h(self.h, C.c_void_p(out.ctypes.data), ptr, C.c_size_t(out.nbytes)))
        self.sync()
        return out

    def lattice_set_mode(self, mixed=1, d_cost32=None, d_state=None):
        """0: all fp64; 1 (default): f32 filter + fp64 decision, every plan shape from one ego (two-egos-per-wave prologue from 3072 egos); 2: always,
        two-ego prologue at any size; 3: as 2 with the one-ego-per-wave prologue (A/B, tests).  Optional device buffers [E][C] receive
        the filter's costs (f32) and states (i32)."""
        self._check(self.lib.f1p_lattice_set_mode(self.h, int(mixed), None if d_cost32 is None else d_cost32.ptr,
                                                  None if d_state is None else d_state.ptr))

    def lattice_set_split(self, groups=0):
        """workgroups per ego of the single-kernel lattice schedules (0 = automatic)"""
        self._check(self.lib.f1p_lattice_set_split(self.h, int(groups)))

    def lattice_set_clearance(self, stations_each_side=2):
        """f32 filter's occupancy test: one station in 2 r + 1 against the clearance map (r > 0) or every station against the bitmap (0)"""
        self._check(self.lib.f1p_lattice_set_clearance(self.h, int(stations_each_side)))

    def lattice_debug_queue(self, E):
        """entries per ego the last mixed-schedule plan of E egos handed to the fp64 refinement (numpy int32 [E])"""
        out = np.empty(int(E), np.int32)
        self._check(self.lib.f1p_lattice_debug_queue(self.h, _ptr(out), int(E)))
        return out

    def lattice_debug_bound(self, d_bound=None):
        """test hook: [E][C] f32 device buffer for the f32 filter's per-candidate a-priori cost error bounds (None = off)"""
        self._check(self.lib.f1p_lattice_debug_bound(self.h, None if d_bound is None else d_bound.ptr))

    def lattice_set_order(self, heavy_first=True):
        """dispatch order of the candidate kernel: egos whose previous plan took the long station pass first (default) or ego order; outputs identical"""
        self._check(self.lib.f1p_lattice_set_order(self.h, 1 if heavy_first else 0))

    def lattice_debug_pass(self, d_pass=None):
        """measurement hook: [E][4] i32 device buffer (zeroed by the caller) for the lazy station pass's per-ego statistics -- candidates
        looked at, of them lane-per-candidate, rounds, queue entries (None = off)"""
        self._check(self.lib.f1p_lattice_debug_pass(self.h, None if d_pass is None else d_pass.ptr))

    def lattice_set_audit(self, every_n=0, n_egos=64):
        """every every_n-th mixed plan is re-planned on a moving window of n_egos egos by the all-fp64 kernel and compared bit for bit"""
        self._check(self.lib.f1p_lattice_set_audit(self.h, int(every_n), int(n_egos)))

    def lattice_audit_read(self, reset=False):
        """dict(plans, egos, mismatching_egos) of the runtime audit since the last reset"""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.f1p_lattice_audit_read(self.h, out, 1 if reset else 0))
        return dict(plans=int(out[0]), egos=int(out[1]), mismatching_egos=int(out[2]))

    def lattice_set_pipeline(self, chunks=0):
        """chunks of egos a mixed plan is pipelined in over two internal streams (0 = automatic, 1 = off)"""
        self._check(self.lib.f1p_lattice_set_pipeline(self.h, int(chunks)))

    def lattice_profile(self, enable=True, read=False):
        """HIP-event timing around the kernels of the mixed schedule; read=True returns (prologue, filter, refine, select) ms of the
        last profiled plan (prologue = 0 when the one-kernel filter ran)"""
        ms = (C.c_float * 4)()
        self._check(self.lib.f1p_lattice_profile(self.h, 1 if enable else 0, ms if read else None))
        return tuple(ms) if read else None

    def lattice_emit_dev(self, d_poses, E, cfg: LatticeCfg, d_cand_idx, d_cand_cost, d_steer, d_speed, d_status=None,
                         d_near_idx=None, d_best_traj=None, d_goals=None):
        self._check(self.lib.f1p_lattice_emit_dev(self.h, _dev(d_poses), _dev(d_goals), int(E), C.byref(cfg), _dev(d_cand_idx),
                                                  _dev(d_cand_cost), _dev(d_steer), _dev(d_speed), _dev(d_status), _dev(d_near_idx),
                                                  _dev(d_best_traj)))
