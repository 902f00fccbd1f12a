"""MultiContext: one process, several GPUs, one Context per device."""
import copy
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .. import _abi
from ..dist import shard_range
from . import Context
from .core import F1PError, _cut, _f64, _tid


class MultiContext:
    """One process, several GPUs (SURVEY.md 8b "Threading"): one Context per device, each driven by its own host thread
    (ctypes releases the GIL for the duration of a C call, and distinct f1p_ctx are thread-safe).  Egos are independent, so a
    batch is cut into contiguous ego ranges -- GPU g gets egos [g E/G, (g+1) E/G) -- with NO collective; the scene (waypoints,
    grid) is replicated.  Results are concatenated in ego order, so the output is identical to one Context planning the whole
    batch.  `devices` may repeat an index (two contexts, two streams on one GPU): that is how a single-GPU box tests this path.
    """

    def __init__(self, devices=None):
        if devices is None:
            n = _abi.load_library().f1p_device_count()
            if n <= 0:
                raise F1PError(_abi.F1P_ENODEV, "no HIP device visible -- the HIP path is mandatory, there is no CPU fallback")
            devices = range(n)
        self.devices = [int(d) for d in devices]
        if not self.devices:
            raise ValueError("devices must name at least one GPU")
        self.ctxs = [Context(d) for d in self.devices]
        self._pool = ThreadPoolExecutor(max_workers=len(self.ctxs), thread_name_prefix="f1p-gpu")

    def close(self):
        if getattr(self, "_pool", None) is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        for c in getattr(self, "ctxs", []):
            c.close()
        self.ctxs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _each(self, fn):
        """run fn(ctx, g) on every context's thread; re-raises the first failure"""
        return [f.result() for f in [self._pool.submit(fn, c, g) for g, c in enumerate(self.ctxs)]]

    # ---- scene: replicated ---------------------------------------------------------------------------------------
    def set_waypoints(self, waypoints, cols=None):
        self._each(lambda c, g: c.set_waypoints(waypoints, cols))

    def set_waypoints_cached(self, waypoints, cols=None):
        self._each(lambda c, g: c.set_waypoints_cached(waypoints, cols))

    def set_tracks(self, tracks, cols=None):
        self._each(lambda c, g: c.set_tracks(tracks, cols))

    def set_tracks_cached(self, tracks, cols=None):
        self._each(lambda c, g: c.set_tracks_cached(tracks, cols))

    def set_grid(self, img, resolution, origin, occupied_below):
        self._each(lambda c, g: c.set_grid(img, resolution, origin, occupied_below))

    def inflate_grid(self, radius):
        self._each(lambda c, g: c.inflate_grid(radius))

    def set_footprint(self, offsets, radius):
        self._each(lambda c, g: c.set_footprint(offsets, radius))

    def sync(self):
        self._each(lambda c, g: c.sync())

    def lattice_set_closed_loop(self, on=True):
        """closed-loop mode on every replica: the ego ranges of a batch are stable, so each context keeps the headings of ITS
        egos' winners and the chain equals the single-context chain"""
        self._each(lambda c, g: c.lattice_set_closed_loop(on))

    def lattice_closed_loop_prev(self):
        """the headings the next closed-loop plan would use, concatenated in ego order (None when no replica holds any)"""
        parts = [p for p in self._each(lambda c, g: c.lattice_closed_loop_prev()) if p is not None]
        return np.concatenate(parts, axis=0) if parts else None

    # ---- batched planners: ego-sharded -----------------------------------------------------------------------------
    def _sharded(self, n_items, call):
        """call(ctx, lo, hi) -> dict of arrays with leading dimension hi - lo; concatenated over the ego ranges"""
        G = len(self.ctxs)
        ranges = [shard_range(n_items, g, G) for g in range(G)]

        def run(c, g):
            lo, hi = ranges[g]
            return call(c, lo, hi) if hi > lo else None
        parts = [p for p in self._each(run) if p is not None]
        if not parts:
            return call(self.ctxs[0], 0, 0)
        return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}

    # (a raceline / track-set pair shares one body, on top of the body the pair shares in Context: ids = None is the raceline)
    def lattice_plan(self, poses, cfg, goals=None, prev_theta=None, want_traj=True, traj_dtype=np.float64):
        return self._lattice_plan(poses, cfg, goals, prev_theta, want_traj, traj_dtype)

    def lattice_plan_tracks(self, poses, track_ids, cfg, goals=None, prev_theta=None, want_traj=True, traj_dtype=np.float64):
        """lattice_plan on the track set, sharded by ego ranges like lattice_plan (set_tracks replicates the set)"""
        return self._lattice_plan(poses, cfg, goals, prev_theta, want_traj, traj_dtype, _tid(track_ids))

    def _lattice_plan(self, poses, cfg, goals, prev_theta, want_traj, traj_dtype, ids=None):
        poses = _f64(poses, (-1, 4)); E = poses.shape[0]; ids = None if ids is None else Context._ids(ids, E)
        g = None if goals is None else _f64(goals, (E, cfg.n_cand, 3))
        pt = None if prev_theta is None else _f64(prev_theta, (E, cfg.n_stations))
        return self._sharded(E, lambda c, lo, hi: c._lattice_plan(poses[lo:hi], cfg, _cut(g, lo, hi), _cut(pt, lo, hi), want_traj, False, False,
                                                                    traj_dtype, _cut(ids, lo, hi)))

    def pure_pursuit(self, poses, lookahead, wheelbase=0.33, max_reacquire=20.0):
        return self._pure_pursuit(poses, lookahead, wheelbase, max_reacquire)

    def pure_pursuit_tracks(self, poses, track_ids, lookahead, wheelbase=0.33, max_reacquire=20.0):
        return self._pure_pursuit(poses, lookahead, wheelbase, max_reacquire, _tid(track_ids))

    def _pure_pursuit(self, poses, lookahead, wheelbase, max_reacquire, ids=None):
        poses = _f64(poses, (-1, 3)); ids = None if ids is None else Context._ids(ids, poses.shape[0])
        return self._sharded(poses.shape[0], lambda c, lo, hi: c._pure_pursuit(poses[lo:hi], lookahead, wheelbase, max_reacquire, _cut(ids, lo, hi)))

    def kmpc_ref(self, states, horizon, dt=0.1, dl=0.03):
        return self._mpc_ref(Context._kmpc_ref, states, horizon, dt, dl)

    def kmpc_ref_tracks(self, states, track_ids, horizon, dt=0.1, dl=0.03):
        return self._mpc_ref(Context._kmpc_ref, states, horizon, dt, dl, _tid(track_ids))

    def stmpc_ref_tracks(self, states, track_ids, horizon, dt=0.025, dl=0.03):
        return self._mpc_ref(Context._stmpc_ref, states, horizon, dt, dl, _tid(track_ids))

    def _mpc_ref(self, ref, states, horizon, dt, dl, ids=None):
        st = _f64(states, (-1, 4)); ids = None if ids is None else Context._ids(ids, st.shape[0])
        return self._sharded(st.shape[0], lambda c, lo, hi: dict(ref=ref(c, st[lo:hi], horizon, dt, dl, _cut(ids, lo, hi))))["ref"]

    def stmpc_qp_plan_tracks(self, x0, track_ids, dcfg, kcfg, v_ks=2.0, dl=0.03, dlk=0.03, opts=None, want_u=True, want_obj=True):
        """Context.stmpc_qp_plan_tracks sharded by ego ranges.  Each context holds the warm start of ITS range, so E and the device list
        must stay the same from call to call for the chain to equal the single-context chain (a new E restarts every warm start)."""
        x0 = _f64(x0, (-1, 7)); ids = Context._ids(track_ids, x0.shape[0])
        return self._sharded(x0.shape[0], lambda c, lo, hi: c.stmpc_qp_plan_tracks(x0[lo:hi], ids[lo:hi], dcfg, kcfg, v_ks, dl, dlk, opts,
                                                                                   want_u, want_obj))

    def stmpc_plan(self, x0, dcfg, kcfg, sampler, v_ks=2.0, dl=0.03, dlk=0.03, want_seq=True, want_cost=True):
        """Context.stmpc_plan sharded by ego ranges.  The generator's ego word is the GLOBAL ego index (each range's first index goes
        down as the sampler's ego offset), so the result equals the single-context call bit for bit.  Each context holds the warm start
        of its range: E and the device list must stay the same from call to call for the chain to equal the single-context chain."""
        x0 = _f64(x0, (-1, 7))

        def call(c, lo, hi):
            s = copy.copy(sampler)
            s.ego_offset = sampler.ego_offset + lo
            return c.stmpc_plan(x0[lo:hi], dcfg, kcfg, s, v_ks, dl, dlk, want_seq, want_cost)
        return self._sharded(x0.shape[0], call)

    def kmpc_shoot(self, x0, ref, controls, cfg, want_seq=True):
        x0 = _f64(x0, (-1, 4))
        return self._sharded(x0.shape[0], lambda c, lo, hi: c.kmpc_shoot(x0[lo:hi], ref[lo:hi], controls[lo:hi], cfg, want_seq))
