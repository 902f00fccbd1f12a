"""Context's path trackers and their leaf kernels: nearest point, circle intersection, pure pursuit, Stanley, LQR (csrc/f1p_trackers.hip)."""
import ctypes as C

import numpy as np

from .core import _dev, _f64, _pick, _ptr, _tid


class _Trackers:
    # ---- leaf kernels; every *_tracks form: ego e follows track track_ids[e] of set_tracks ----------------------------
    def nearest_point(self, pts):
        return self._nearest_point(pts)

    def nearest_point_tracks(self, pts, track_ids):
        return self._nearest_point(pts, _tid(track_ids))

    def _nearest_point(self, pts, ids=None):
        pts = _f64(pts, (-1, 2)); E = pts.shape[0]; ids = None if ids is None else self._ids(ids, E)
        proj = np.empty((E, 2)); dist = np.empty(E); t = np.empty(E); idx = np.empty(E, np.int32)
        fn, tid = _pick(self.lib.f1p_nearest_point_batch, self.lib.f1p_nearest_point_tracks_batch, ids)
        self._check(fn(self.h, _ptr(pts), *tid, E, _ptr(proj), _ptr(dist), _ptr(t), _ptr(idx)))
        return proj, dist, t, idx

    def intersect_point(self, pts, radius, start_t, wrap=False):
        pts = _f64(pts, (-1, 2)); E = pts.shape[0]
        st = _f64(np.broadcast_to(start_t, (E,)))
        p = np.empty((E, 2)); i = np.empty(E, np.int32); t = np.empty(E); found = np.empty(E, np.int32)
        self._check(self.lib.f1p_intersect_point_batch(self.h, _ptr(pts), _ptr(st), E, float(radius), 1 if wrap else 0,
                                                       _ptr(p), _ptr(i), _ptr(t), _ptr(found)))
        return p, i, t, found.astype(bool)

    # ---- pure pursuit ------------------------------------------------------------------------------------
    def pure_pursuit(self, poses, lookahead, wheelbase=0.33, max_reacquire=20.0):
        return self._pure_pursuit(poses, lookahead, wheelbase, max_reacquire)

    def pure_pursuit_tracks(self, poses, track_ids, lookahead, wheelbase=0.33, max_reacquire=20.0):
        return self._pure_pursuit(poses, lookahead, wheelbase, max_reacquire, _tid(track_ids))

    def _pure_pursuit(self, poses, lookahead, wheelbase, max_reacquire, ids=None):
        poses = _f64(poses, (-1, 3)); E = poses.shape[0]; ids = None if ids is None else self._ids(ids, E)
        cols = np.empty(28 * E + 8, np.uint8)                     # the five result columns as views of one buffer: one address look-up (lattice_plan does the same)
        base = cols.__array_interface__["data"][0]
        o8, o4 = 8 * E, 4 * E
        out = dict(steer=cols[0:o8].view(np.float64), speed=cols[o8:2 * o8].view(np.float64), near_idx=cols[2 * o8:2 * o8 + o4].view(np.int32),
                   la_idx=cols[2 * o8 + o4:2 * o8 + 2 * o4].view(np.int32), status=cols[2 * o8 + 2 * o4:2 * o8 + 3 * o4].view(np.int32))
        V = C.c_void_p
        fn, tid = _pick(self.lib.f1p_pure_pursuit_batch, self.lib.f1p_pure_pursuit_tracks_batch, ids)
        self._check(fn(self.h, _ptr(poses), *tid, E, float(lookahead), float(wheelbase), float(max_reacquire),
                       V(base), V(base + o8), V(base + 2 * o8), V(base + 2 * o8 + o4), V(base + 2 * o8 + 2 * o4)))
        return out

    def pure_pursuit_dev(self, d_poses, E, lookahead, d_steer, d_speed, d_near_idx=None, d_la_idx=None, d_status=None,
                         wheelbase=0.33, max_reacquire=20.0):
        """Asynchronous launch on HBM-resident buffers; poses [E][3]."""
        self._pure_pursuit_dev((), d_poses, E, lookahead, d_steer, d_speed, d_near_idx, d_la_idx, d_status, wheelbase, max_reacquire)

    def pure_pursuit_tracks_dev(self, d_poses, d_track_ids, E, lookahead, d_steer, d_speed, d_near_idx=None, d_la_idx=None, d_status=None,
                                wheelbase=0.33, max_reacquire=20.0):
        """Asynchronous launch on HBM-resident buffers; poses [E][3], track ids [E] int32."""
        self._pure_pursuit_dev((_dev(d_track_ids),), d_poses, E, lookahead, d_steer, d_speed, d_near_idx, d_la_idx, d_status, wheelbase,
                               max_reacquire)

    def _pure_pursuit_dev(self, tid, d_poses, E, lookahead, d_steer, d_speed, d_near_idx, d_la_idx, d_status, wheelbase, max_reacquire):
        """tid: () or (the track ids' device pointer,)"""
        fn = self.lib.f1p_pure_pursuit_tracks_dev if tid else self.lib.f1p_pure_pursuit_dev
        self._check(fn(self.h, _dev(d_poses), *tid, int(E), float(lookahead), float(wheelbase), float(max_reacquire),
                       _dev(d_steer), _dev(d_speed), _dev(d_near_idx), _dev(d_la_idx), _dev(d_status)))

    def pure_pursuit_set_form(self, egos_per_wave=0):
        """Egos per wave of the batched pure pursuit: 0 (default) by batch size, 1 = k_pure_pursuit, 4 | 8 | 16 = k_pure_pursuit16<G>.  Identical outputs (A/B, tests)."""
        self._check(self.lib.f1p_pure_pursuit_set_form(self.h, int(egos_per_wave)))

    # ---- Stanley / LQR --------------------------------------------------------------------
    def stanley(self, states, wheelbase=0.33, k_path=5.0):
        return self._stanley(states, wheelbase, k_path)

    def stanley_tracks(self, states, track_ids, wheelbase=0.33, k_path=5.0):
        return self._stanley(states, wheelbase, k_path, _tid(track_ids))

    def _stanley(self, states, wheelbase, k_path, ids=None):
        st = _f64(states, (-1, 4)); E = st.shape[0]; ids = None if ids is None else self._ids(ids, E)
        out = dict(steer=np.empty(E), speed=np.empty(E), near_idx=np.empty(E, np.int32))
        fn, tid = _pick(self.lib.f1p_stanley_batch, self.lib.f1p_stanley_tracks_batch, ids)
        self._check(fn(self.h, _ptr(st), *tid, E, float(wheelbase), float(k_path), _ptr(out["steer"]), _ptr(out["speed"]),
                       _ptr(out["near_idx"])))
        return out

    def lqr(self, states, err, wheelbase=0.33, timestep=0.01, q=(0.999, 0.0, 0.0066, 0.0), r=0.75, max_iter=50, eps=0.001):
        """err [E, 2] = (e_cog, theta_e) of the previous call; the updated errors come back in out['err']"""
        return self._lqr(states, err, wheelbase, timestep, q, r, max_iter, eps)

    def lqr_tracks(self, states, track_ids, err, wheelbase=0.33, timestep=0.01, q=(0.999, 0.0, 0.0066, 0.0), r=0.75, max_iter=50, eps=0.001):
        """as lqr(); an ego with a bad track id keeps its err"""
        return self._lqr(states, err, wheelbase, timestep, q, r, max_iter, eps, _tid(track_ids))

    def _lqr(self, states, err, wheelbase, timestep, q, r, max_iter, eps, ids=None):
        st = _f64(states, (-1, 4)); E = st.shape[0]; ids = None if ids is None else self._ids(ids, E)
        err = _f64(err, (E, 2)).copy(); qa = _f64(q, (4,))
        out = dict(steer=np.empty(E), speed=np.empty(E), near_idx=np.empty(E, np.int32), err=err)
        fn, tid = _pick(self.lib.f1p_lqr_batch, self.lib.f1p_lqr_tracks_batch, ids)
        self._check(fn(self.h, _ptr(st), *tid, _ptr(err), E, float(wheelbase), float(timestep), _ptr(qa), float(r), int(max_iter),
                       float(eps), _ptr(out["steer"]), _ptr(out["speed"]), _ptr(out["near_idx"])))
        return out
