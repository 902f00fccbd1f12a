"""Context's scene: raceline, track set, occupancy grid and footprint (csrc/f1p_scene.hip)."""
import ctypes as C

import numpy as np

from .. import _abi
from . import _content_signature
from .core import F1PError, _f64, _ptr


class _Scene:
    # ---- scene ---------------------------------------------------------------------------------------
    def set_waypoints(self, waypoints, cols=None):
        """waypoints [N, m>=3]; cols = (x, y, v, psi) column indices, psi = -1 for none.  Default: the
        pure-pursuit layout [x, y, v, psi, ...] (pure_pursuit.py:49)."""
        wp = np.asarray(waypoints)
        if wp.ndim != 2 or wp.shape[1] < 3:
            raise ValueError('Waypoints needs to be a (Nxm), m >= 3, numpy array!')   # pure_pursuit.py:101-102
        wp = _f64(wp)
        if cols is None:
            cols = (0, 1, 2, 3 if wp.shape[1] >= 4 else -1, 4 if wp.shape[1] >= 5 else -1)
        cols = tuple(int(c) for c in cols) + (-1,) * (5 - len(cols))      # (x, y, v, psi, kappa)
        self._check(self.lib.f1p_set_waypoints_ex(self.h, _ptr(wp), wp.shape[0], wp.shape[1], *cols))
        self.n_waypoints = wp.shape[0]

    def set_waypoints_cached(self, waypoints, cols=None):
        """Upload only when the caller's array changed (the reference keeps a live reference to the caller's
        array, pure_pursuit.py:103, so in-place edits must be seen)."""
        wp = np.asarray(waypoints)
        if wp.ndim != 2 or wp.shape[1] < 3:
            raise ValueError('Waypoints needs to be a (Nxm), m >= 3, numpy array!')
        key = (wp.shape, wp.dtype.str, cols, _content_signature(wp))
        if key != self._wp_key:
            self.set_waypoints(wp, cols)
            self._wp_key = key

    def set_tracks(self, tracks, cols=None):
        """Track set (f1p_set_track_set): `tracks` = K arrays [N_k, m], m >= 3, every N_k >= 2, all with the same columns; cols as
        set_waypoints.  The *_tracks calls then take track_ids [E] int32 (ego e follows tracks[track_ids[e]]).  Independent of the
        raceline of set_waypoints.  An empty list clears the set."""
        tracks = [np.asarray(t) for t in tracks]
        if not tracks:
            self._check(self.lib.f1p_set_track_set(self.h, None, None, 0, 0, 0, 0, 0, -1, -1))
            self.n_tracks = 0
            return
        m = tracks[0].shape[1] if tracks[0].ndim == 2 else -1
        if any(t.ndim != 2 or t.shape[1] != m for t in tracks) or m < 3:
            raise ValueError("tracks must be 2-D arrays [N_k, m], m >= 3, all with the same m")
        wp = _f64(np.concatenate(tracks, axis=0))
        offsets = np.zeros(len(tracks) + 1, np.int64)
        offsets[1:] = np.cumsum([t.shape[0] for t in tracks])
        if cols is None:
            cols = (0, 1, 2, 3 if m >= 4 else -1, 4 if m >= 5 else -1)
        cols = tuple(int(c) for c in cols) + (-1,) * (5 - len(cols))      # (x, y, v, psi, kappa)
        self._check(self.lib.f1p_set_track_set(self.h, _ptr(wp), _ptr(offsets), len(tracks), m, *cols))
        self.n_tracks = len(tracks)

    def set_tracks_cached(self, tracks, cols=None):
        """set_tracks, skipping the upload when neither the arrays' content nor the columns changed since the last upload"""
        tracks = [np.asarray(t) for t in tracks]
        key = (tuple((t.shape, t.dtype.str, _content_signature(t)) for t in tracks), None if cols is None else tuple(cols))
        if key != self._tracks_key:
            self._tracks_key = None
            self.set_tracks(tracks, cols)
            self._tracks_key = key

    def set_grid(self, img, resolution, origin, occupied_below):
        """img [h, w] u8, row 0 = top (ROS map_server); a cell is occupied iff value < occupied_below."""
        if img is None:
            self._check(self.lib.f1p_set_grid(self.h, None, 0, 0, 0.0, 0.0, 0.0, 0))
            self.has_grid = False
            return
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.ndim != 2:
            raise ValueError("occupancy image must be 2-D u8")
        self._check(self.lib.f1p_set_grid(self.h, _ptr(img), img.shape[1], img.shape[0], float(resolution),
                                          float(origin[0]), float(origin[1]), int(occupied_below)))
        self.has_grid = True
        self._grid_shape = (int(img.shape[0]), int(img.shape[1]))

    def grid_distance(self, cap_cells=64):
        """Euclidean distance transform of the installed grid -> f32 [h, w] metres in the image's row order, saturated at
        cap_cells * resolution (f1p_grid_distance_batch)."""
        if not self.has_grid:
            raise F1PError(_abi.F1P_ESTATE, "occupancy grid not set")
        dist = np.empty(self._grid_shape, dtype=np.float32)
        self._check(self.lib.f1p_grid_distance_batch(self.h, _ptr(dist), int(cap_cells)))
        return dist

    def inflate_grid(self, radius):
        """Dilate the collision bitmap by a disc of `radius` metres (0 restores the uploaded grid)."""
        self._check(self.lib.f1p_inflate_grid(self.h, float(radius)))

    def set_footprint(self, offsets, radius):
        """Oriented footprint: discs of `radius` at longitudinal `offsets` [m] along the heading (f1p_set_footprint); offsets = ()
        restores the point test."""
        off = _f64(list(offsets)).reshape(-1)
        self._check(self.lib.f1p_set_footprint(self.h, int(off.shape[0]), _ptr(off) if off.shape[0] else None, float(radius)))

    def grid_debug_read(self, which):
        """test hook (f1p_grid_debug_read): one of the packed maps cell by cell -- which = 0 the grid as uploaded, 1 the active bitmap,
        2 the clearance map -> (cells bool [h, w] in the image's row order, padding_all_set bool, clear_dist_cells float)"""
        cells = np.empty(self._grid_shape if self.has_grid else (1, 1), dtype=np.uint8)    # (without a grid the call is rejected)
        dist = C.c_double(); pad = C.c_int32()
        self._check(self.lib.f1p_grid_debug_read(self.h, int(which), _ptr(cells), C.byref(dist), C.byref(pad)))
        return cells.astype(bool), bool(pad.value), dist.value

    def grid_occupied(self, pts):
        """test hook (f1p_grid_occupied_batch): the collision tests' point rule on the active bitmap, pts [E, 2] metres -> bool [E]
        (occupied, outside the image or not finite)"""
        pts = _f64(pts, (-1, 2)); E = pts.shape[0]
        out = np.empty(E, dtype=np.uint8)
        self._check(self.lib.f1p_grid_occupied_batch(self.h, _ptr(pts), E, _ptr(out)))
        return out.astype(bool)
