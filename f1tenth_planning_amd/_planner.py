"""What the six drop-in planner classes share: the lazily created context, the reference's waypoint check, the track-set checks, the
occupancy map of set_map / load_map, and the configuration checks and cfg builders of the two MPC planners."""
import os

import numpy as np

from . import _abi
from ._rivals import check_rivals
from .runtime import Context

NO_WAYPOINTS = 'Please set waypoints to track during planner instantiation or when calling plan()'


class Planner:
    """Base of the planner classes.  A class keeps `waypoints`, `_device` and `_ctx` (None until the first GPU call)."""

    def _context(self):
        if self._ctx is None:
            self._ctx = Context(self._device if self._device is not None else int(os.environ.get("LOCAL_RANK", "0")))
            self._on_context(self._ctx)
        return self._ctx

    def _on_context(self, ctx):
        """called once, with the context just created"""

    def _take_waypoints(self, waypoints, min_cols, message, asarray=False):
        """The reference's validation (pure_pursuit.py:100-106 and its siblings): a given array is checked and kept, none needs one kept
        earlier.  asarray: read the shape of np.asarray(waypoints) (the MPC planners, whose courses are lists of columns) instead of
        waypoints.shape (the trackers)."""
        if waypoints is not None:
            shape = np.asarray(waypoints).shape if asarray else waypoints.shape
            if len(shape) != 2 or shape[1] < min_cols:
                raise ValueError(message)
            self.waypoints = waypoints
        elif self.waypoints is None:
            raise ValueError(NO_WAYPOINTS)

    def _bind_waypoints(self, waypoints, min_cols, message):
        """_take_waypoints, then the waypoints on the context (uploaded when they changed) -> the context"""
        self._take_waypoints(waypoints, min_cols, message)
        ctx = self._context()
        ctx.set_waypoints_cached(self.waypoints)
        return ctx

    def _bind_tracks(self, tracks, track_ids, min_cols):
        """_check_tracks, then the track set on the context (uploaded when it changed) -> the context"""
        _check_tracks(tracks, track_ids, min_cols)
        ctx = self._context()
        ctx.set_tracks_cached(tracks)
        return ctx


def _check_tracks(tracks, track_ids, min_cols):
    """the per-vehicle waypoint validation of the reference (pure_pursuit.py:100-102, stanley.py:131-132, lqr.py:195-196) for every track"""
    if track_ids is None:
        raise ValueError("tracks needs track_ids: one track index per ego")
    if len(tracks) == 0:
        raise ValueError("tracks must hold at least one waypoint array")
    for t in tracks:
        if len(np.shape(t)) != 2 or np.shape(t)[1] < min_cols:
            raise ValueError(f'Waypoints needs to be a (Nxm), m >= {min_cols}, numpy array!')


def _course_columns(path):
    """an MPC course [x, y, yaw, v] (four 1-D arrays or an array [4, N], kinematic_mpc.py:479-482) as (x, y, v, yaw) columns"""
    cx, cy, cyaw, sp = (np.asarray(path[k], dtype=np.float64) for k in range(4))
    return np.column_stack([cx, cy, sp, cyaw])


def _track_columns(tracks, track_ids):
    """ValueError before anything touches the GPU; -> the MPC courses as (x, y, v, yaw) columns"""
    if track_ids is None:
        raise ValueError("tracks needs track_ids: one track index per ego")
    if len(tracks) == 0:
        raise ValueError("tracks must hold at least one course")
    cols = []
    for path in tracks:
        if len(path) < 4:
            raise ValueError("every track must hold [x, y, yaw, v]")
        cols.append(_course_columns(path))
    return cols


class OccupancyMap:
    """set_map / load_map of LatticePlanner, KMPCPlanner and STMPCPlanner: the map is kept on the host and installed on the planner's
    context when there is one, or when it is created."""
    _map = None                            # (img u8, resolution, (ox, oy), occupied_below) of set_map
    _inflate = 0.0

    def set_map(self, image, resolution, origin, occupied_thresh=0.65, negate=0, inflate=0.0):
        """Occupancy image in the ROS map_server layout (examples/control/Spielberg_map.yaml:1-6): u8 [h, w], row 0 at
        the top, `origin` = world (x, y[, yaw]) of the lower-left pixel.  A cell is occupied when its occupancy
        probability (255 - v)/255 (v/255 if negate) exceeds occupied_thresh.  `inflate` (metres) dilates the occupied set by
        a disc on the device (distance-transform preprocessor), turning the point test -- the lattice's per station, mpc_config.COLLISION's
        per rollout point -- into a disc test: e.g. 0.155 for the half width of the reference's 0.58 m x 0.31 m vehicle
        (kinematic_mpc.py:60-61)."""
        image = np.asarray(image)
        if image.ndim != 2:
            raise ValueError("map image must be 2-D")
        if len(origin) > 2 and abs(origin[2]) > 1e-12:
            raise ValueError("map origin yaw must be 0")
        img = image.astype(np.uint8)
        if negate:
            img = 255 - img
        occupied_below = int(np.ceil(255.0 * (1.0 - occupied_thresh)))      # v < 255 (1 - thresh)  <=>  p > thresh
        self._map = (np.ascontiguousarray(img), float(resolution), (float(origin[0]), float(origin[1])), occupied_below)
        self._inflate = float(inflate)
        self._map_changed()
        if self._ctx is not None:
            self._install_map(self._ctx)

    def load_map(self, yaml_path, inflate=0.0):
        """Read a ROS map_server YAML + image (examples/control/Spielberg_map.yaml) and install it as the occupancy grid."""
        from .io import load_map
        m = load_map(yaml_path)
        self.set_map(m["image"], m["resolution"], m["origin"], occupied_thresh=m["occupied_thresh"], negate=0, inflate=inflate)   # negate already applied
        return m

    def _map_changed(self):
        """called by set_map once the new map is kept, before it goes to the context"""

    def _install_map(self, ctx):
        ctx.set_grid(*self._map)
        if self._inflate > 0.0:
            ctx.inflate_grid(self._inflate)

    def _on_context(self, ctx):
        if self._map is not None:
            self._install_map(ctx)


# ---- shared by KMPCPlanner and STMPCPlanner ---------------------------------------------------------------------------------------------
SOLVERS = ("shooting", "qp")


def _diag(m):
    m = np.asarray(m.todense()) if hasattr(m, "todense") else np.asarray(m)
    return np.diag(m) if m.ndim == 2 else m


def qp_walls_field(c):
    """the name of the config's wall switch that is on -- QP_WALLS (KMPCPlanner's mpc_config) or QP_WALLS_ST (STMPCPlanner's) -- or None"""
    for name in ("QP_WALLS", "QP_WALLS_ST"):
        if getattr(c, name, False):
            return name
    return None


def check_solver(c, weights, substeps, tk_within_t=False, avoid_max_t=None, walls=False, walls_st=False):
    """ValueError before anything touches the GPU: an unknown SOLVER, weights the QP path does not take (diagonal only), a COLLISION
    setting without meaning.  weights: ((mpc_config field, size), ...) of the QP's weight matrices; substeps: the fields that count tested
    points per step; tk_within_t: the QP also needs TK <= T (STMPCPlanner); avoid_max_t: QP_AVOID's cap on T (STMPCPlanner's dynamic QP);
    walls: the planner's QP has wall rows behind QP_WALLS (KMPCPlanner); walls_st: behind QP_WALLS_ST (STMPCPlanner, both branches)."""
    if c.SOLVER not in SOLVERS:
        raise ValueError(f"mpc_config.SOLVER must be one of {SOLVERS}, not {c.SOLVER!r}")
    if c.SOLVER == "qp":
        for name, n in weights:
            w = getattr(c, name)
            w = np.asarray(w.todense() if hasattr(w, "todense") else w, dtype=np.float64)
            if w.shape != (n, n) or np.any(w - np.diag(np.diag(w)) != 0):
                raise ValueError(f"SOLVER='qp' takes diagonal {n}x{n} weights only; mpc_config.{name} is not")
        if tk_within_t and c.TK > c.T:
            raise ValueError("SOLVER='qp' needs TK <= T (the reference's kinematic branch would linearise about a cut-short prediction)")
    if getattr(c, "QP_AVOID", False):
        if c.SOLVER != "qp":
            raise ValueError("mpc_config.QP_AVOID adds avoidance rows to the QP; the shooting solver tests its rollouts without it (SOLVER='qp')")
        rho, lin, margin = float(c.QP_AVOID_RHO), float(c.QP_AVOID_LIN), float(c.QP_AVOID_MARGIN)
        if not (rho > 0.0 and np.isfinite(rho)):
            raise ValueError(f"mpc_config.QP_AVOID_RHO must be finite and > 0, not {c.QP_AVOID_RHO!r}")
        if not (lin >= 0.0 and np.isfinite(lin)):
            raise ValueError(f"mpc_config.QP_AVOID_LIN must be finite and >= 0, not {c.QP_AVOID_LIN!r}")
        if not np.isfinite(margin):
            raise ValueError(f"mpc_config.QP_AVOID_MARGIN must be finite, not {c.QP_AVOID_MARGIN!r}")
        if int(c.TK) > 31:
            raise ValueError("mpc_config.QP_AVOID needs TK <= 31 (the slack takes the 64th lane's place)")
        if avoid_max_t is not None and int(c.T) > avoid_max_t:
            raise ValueError(f"mpc_config.QP_AVOID needs T <= {avoid_max_t} (F1P_STMPC_QP_AVOID_MAX_T: the avoidance rows share the CU's LDS with the Newton matrix)")
    if getattr(c, "QP_WALLS", False) and not walls:
        raise ValueError("QP_WALLS: KMPCPlanner only")
    if getattr(c, "QP_WALLS_ST", False) and not walls_st:
        raise ValueError("QP_WALLS_ST: STMPCPlanner only")
    wf = qp_walls_field(c)
    if wf:
        if c.SOLVER != "qp":
            raise ValueError(f"mpc_config.{wf} adds wall rows to the QP; the shooting solver tests its rollouts with COLLISION (SOLVER='qp')")
        reach, margin = float(c.QP_WALL_REACH), float(c.QP_WALL_MARGIN)
        if not (reach > 0.0 and np.isfinite(reach)):
            raise ValueError(f"mpc_config.QP_WALL_REACH must be finite and > 0, not {c.QP_WALL_REACH!r}")
        if not np.isfinite(margin):
            raise ValueError(f"mpc_config.QP_WALL_MARGIN must be finite, not {c.QP_WALL_MARGIN!r}")
        if int(c.TK) > 31:
            raise ValueError(f"mpc_config.{wf} needs TK <= 31 (the slack takes the 64th lane's place)")
        if wf == "QP_WALLS_ST" and avoid_max_t is not None and int(c.T) > avoid_max_t:
            raise ValueError(f"mpc_config.QP_WALLS_ST needs T <= {avoid_max_t} (F1P_STMPC_QP_AVOID_MAX_T: the wall rows share the CU's LDS with the Newton matrix)")
    if c.COLLISION:
        if c.SOLVER == "qp":
            raise ValueError("mpc_config.COLLISION tests the shooting solver's rollouts; SOLVER='qp' has none")
        for name in substeps:
            if not 1 <= int(getattr(c, name)) <= 16:
                raise ValueError(f"mpc_config.{name} must be in [1, 16], not {getattr(c, name)!r}")


def qp_opts(c):
    return _abi.kmpc_qp_opts(max_iter=c.QP_MAX_ITER, tol=c.QP_TOL)


def qp_avoid(c):
    """mpc_config.QP_AVOID* as the f1p_kmpc_qp_avoid struct, None while it is off"""
    if not getattr(c, "QP_AVOID", False):
        return None
    return _abi.kmpc_qp_avoid(True, c.QP_AVOID_MARGIN, c.QP_AVOID_RHO, c.QP_AVOID_LIN)


def qp_wall_samples(reach, resolution):
    """the march's steps per side: ceil(reach / (resolution / 2)); ValueError past the library's 256"""
    n = int(np.ceil(float(reach) / (0.5 * float(resolution))))
    if n > _abi.KMPC_QP_WALL_MAX_SAMPLES:
        raise ValueError(f"mpc_config.QP_WALL_REACH = {reach!r} m at a map resolution of {resolution!r} m needs {n} samples per side; "
                         f"at most {_abi.KMPC_QP_WALL_MAX_SAMPLES} (reach <= {_abi.KMPC_QP_WALL_MAX_SAMPLES * 0.5 * float(resolution):g} m)")
    return max(n, 1)


def qp_walls(c, resolution):
    """mpc_config.QP_WALL* as the f1p_kmpc_qp_walls struct for a map of this resolution, None while QP_WALLS / QP_WALLS_ST is off"""
    if not qp_walls_field(c):
        return None
    return _abi.kmpc_qp_walls(True, qp_wall_samples(c.QP_WALL_REACH, resolution), c.QP_WALL_MARGIN)


def kin_cfg_struct(c, n_rollouts=None):
    """the kinematic model's f1p_kmpc_cfg from either mpc_config (dense, sparse or vector weights)"""
    return _abi.kmpc_cfg(horizon=c.TK, n_rollouts=n_rollouts or c.N_ROLLOUTS, dt=c.DTK, wheelbase=c.WB, max_steer=c.MAX_STEER,
                         max_dsteer=c.MAX_DSTEER, max_speed=c.MAX_SPEED, min_speed=c.MIN_SPEED, max_accel=c.MAX_ACCEL,
                         q=_diag(c.Qk), qf=_diag(c.Qfk), r=_diag(c.Rk), rd=_diag(c.Rdk))


def take_obstacles(planner):
    """the attribute `obstacles` of a planner: the next plan / plan_batch call TAKES it -- None again afterwards, also when the call raises"""
    obstacles, planner.obstacles = planner.obstacles, None
    return obstacles


def check_obstacle_shape(obstacles, E, single=False):
    """obstacles as fp64 [E, M, 5] with 1 <= M <= 16; ValueError before anything touches the GPU.  single: plan()'s [M, 5] for its one ego"""
    o = np.ascontiguousarray(obstacles, dtype=np.float64)
    if single:
        if o.ndim != 2:
            raise ValueError("obstacles must be [M, 5] = (x, y, vx, vy, r)")
        o = o[None]
    if o.ndim != 3 or o.shape[0] != E or o.shape[2] != 5 or o.shape[1] < 1:
        raise ValueError(f"obstacles must be [E={E}, M, 5] = (x, y, vx, vy, r) with 1 <= M <= 16")
    if o.shape[1] > 16:
        raise ValueError("at most 16 obstacles per ego (M <= 16)")
    return o


class MPCPlanner(OccupancyMap, Planner):
    """Base of KMPCPlanner and STMPCPlanner.  A class names its mpc_config's QP weights and COLLISION substep fields."""
    _QP_WEIGHTS = ()                       # ((mpc_config field, size), ...)
    _SUBSTEPS = ()
    _TK_WITHIN_T = False
    _QP_AVOID_MAX_T = None                 # mpc_config.QP_AVOID's cap on T, where the planner's QP has one
    _QP_WALLS = False                      # the planner's QP takes mpc_config.QP_WALLS
    _QP_WALLS_ST = False                   # ... mpc_config.QP_WALLS_ST (STMPCPlanner: its config's QP_WALLS keeps raising)

    def _check_solver(self):
        check_solver(self.config, self._QP_WEIGHTS, self._SUBSTEPS, self._TK_WITHIN_T, self._QP_AVOID_MAX_T, self._QP_WALLS, self._QP_WALLS_ST)

    def _check_collision(self):
        """ValueError before anything touches the GPU: the checks of check_solver, and COLLISION / QP_WALLS without a map"""
        self._check_solver()
        if self.config.COLLISION and self._map is None:
            raise ValueError("mpc_config.COLLISION needs an occupancy grid: call set_map / load_map first")
        wf = qp_walls_field(self.config)
        if wf:
            if self._map is None:
                raise ValueError(f"mpc_config.{wf} needs an occupancy grid: call set_map / load_map first")
            qp_wall_samples(self.config.QP_WALL_REACH, self._map[1])

    # the attribute `obstacles` (moving discs): the next plan / plan_batch call TAKES it -- None again afterwards, also
    # when the call raises -- so obstacles are given per call, as a keyword argument would be
    def _take_obstacles(self):
        return take_obstacles(self)

    def _check_obstacles(self, obstacles, E, single=False):
        """-> None or obstacles as fp64 [E, M, 5]; ValueError before anything touches the GPU.  single: plan()'s [M, 5] for its one ego"""
        if obstacles is None:
            return None
        c = self.config
        if c.SOLVER == "qp":
            if not getattr(c, "QP_AVOID", False):
                raise ValueError("obstacles are tested on the shooting solver's rollouts; SOLVER='qp' takes none")
            return check_obstacle_shape(obstacles, E, single)      # (mpc_config.QP_AVOID: rows of the QP, no tested points)
        o = check_obstacle_shape(obstacles, E, single)
        for name in self._SUBSTEPS:
            if not 1 <= int(getattr(c, name)) <= 16:
                raise ValueError(f"{name} must be in [1, 16]")
        return o

    def _check_rivals(self, rivals, E, obstacles):
        """the attribute `rivals` of a plan_batch over E egos; ValueError before anything touches the GPU"""
        qp_rows = self.config.SOLVER == "qp" and getattr(self.config, "QP_AVOID", False)
        check_rivals(rivals, E, obstacles, None if qp_rows else self.config.SOLVER)
        if qp_rows:
            return
        for name in self._SUBSTEPS:
            if not 1 <= int(getattr(self.config, name)) <= 16:
                raise ValueError(f"{name} must be in [1, 16]")
