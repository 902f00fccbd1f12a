"""KMPCPlanner on the MI355X path: kinematic-bicycle MPC solved by random shooting.

Same class names (`mpc_config`, `State`, `KMPCPlanner`), constructor and `plan(states, waypoints=None)` signature
as the reference (f1tenth_planning/control/kinematic_mpc/kinematic_mpc.py:40-160), so
examples/control/kinematic_mpc.py drives it unchanged.  What differs is the solver: the reference linearises the
model and solves a QP with cvxpy/OSQP (:283-450, third-party, out of scope); here R candidate control sequences are
rolled out through the reference's own nonlinear step (update_state_kinematic :223-243) on the GPU
(csrc/k_kmpc.hip), scored with the reference's objective (:324-334) and bounds (:391-401), and the best one is
applied (:506-508).  The candidates are generated inside the kernel (counter-based Philox4x32-10, include/f1p.h
f1p_kmpc_sampler) around a warm start that stays on the device; a plan uploads 32 bytes per vehicle.  The reference trajectory extraction (calc_ref_trajectory_kinematic :162-206) also runs on the
GPU.

mpc_config.SOLVER = "qp" selects the reference's own solver instead: the linearised QP of :245-450, solved exactly (to QP_TOL) by
a batched fp64 interior-point kernel (csrc/k_kmpc_qp.hip), warm-started like the reference from the previous solution (unshifted).

mpc_config.COLLISION = True (shooting only) tests every rollout against the occupancy grid installed with set_map / load_map: a rollout
that touches an occupied cell cannot win (f1p_kmpc_set_collision).

planner.obstacles = [M, 5] before plan() / [E, M, 5] before plan_batch() (shooting only) tests every rollout of THAT call against moving
discs, rows (x, y, vx, vy, r) in the map frame at constant velocity, M <= 16, r < 0 or NaN = an empty slot: a rollout that is inside a
disc at the time it gets there cannot win (f1p_kmpc_set_obstacles).  The next plan / plan_batch call TAKES the attribute:
it is None again afterwards, so obstacles are given per call, as a keyword argument would be, and a call without them plans without any.
The caller folds the vehicle's own radius into r.  (An attribute, not a keyword: the signatures of plan and plan_batch are the
reference's and a pinned record, tests/test_runtime_calls.py.)

planner.rivals = Rivals(count=M, radius=r[, reach, groups, predict, horizon, knots, inflate, wrap]) (shooting only, plan_batch only) makes the vehicles of a batch each other's
obstacles: while it is set, every plan_batch finds each ego's M nearest other vehicles of its race among the call's own x0 ON THE DEVICE
(f1p_rivals_dev) and tests the rollouts against them as above.  Persistent until set to None; not together with `obstacles`.
predict="track" predicts each rival along the course it follows (the call's tracks / track_ids, else the raceline) over TK * DTK seconds
(f1p_rivals_predict_dev); with speed="profile" the rival moves with that course's speed column, scaled by its speed now
(DESIGN.md 5u).

mpc_config.QP_AVOID = True (SOLVER="qp" only) lets the QP take `obstacles` (plan and plan_batch) and `rivals` (plan_batch) as well: per step
the two discs nearest to the previous solution's path become half-plane rows of the QP, softened by one slack variable with the cost
QP_AVOID_RHO eps^2 + QP_AVOID_LIN eps (f1p_kmpc_qp_set_avoid).  The rows are linearised and soft -- an avoidance term, not a
guarantee; QP_AVOID_MARGIN [m] widens every disc.  TK <= 31.

mpc_config.QP_WALLS = True (SOLVER="qp" only, needs set_map / load_map) lets the QP see the map: per step the walls found within QP_WALL_REACH
metres to the left and to the right of the previous solution's path, on the occupancy grid as inflated by set_map(inflate=...), compete with
the discs for the step's two half-plane rows (f1p_kmpc_qp_set_walls).  Soft and linearised like the discs' rows and under the
same slack; QP_WALL_MARGIN [m] keeps the rows that far off the contact.  Works with plan, plan_batch, tracks and rivals, with or without
QP_AVOID.  TK <= 31.
"""
import warnings
from dataclasses import dataclass, field

import numpy as np

from ... import _abi
from ..._planner import MPCPlanner, _track_columns, qp_avoid, qp_opts, qp_walls
from ..._planner import kin_cfg_struct as _cfg_struct
from ..._rivals import SINGLE_EGO, RivalFeed
from ...runtime import Context, kmpc_qp_set_avoid, kmpc_qp_set_walls, kmpc_set_obstacles, kmpc_set_obstacles_dev


@dataclass
class mpc_config:
    NXK: int = 4  # length of kinematic state vector: z = [x, y, v, yaw]
    NU: int = 2  # length of input vector: u = [acceleration, steering angle]
    TK: int = 8  # finite time horizon length kinematic
    Rk: list = field(default_factory=lambda: np.diag([0.01, 100.0]))   # input cost matrix [accel, steer]
    Rdk: list = field(default_factory=lambda: np.diag([0.01, 100.0]))  # input difference cost matrix
    Qk: list = field(default_factory=lambda: np.diag([13.5, 13.5, 5.5, 13.0]))   # state error cost [x, y, v, yaw]
    Qfk: list = field(default_factory=lambda: np.diag([13.5, 13.5, 5.5, 13.0]))  # final state error cost
    N_IND_SEARCH: int = 20  # Search index number
    DTK: float = 0.1  # time step [s] kinematic
    dlk: float = 0.03  # dist step [m] kinematic
    LENGTH: float = 0.58  # Length of the vehicle [m]
    WIDTH: float = 0.31  # Width of the vehicle [m]
    WB: float = 0.33  # Wheelbase [m]
    MIN_STEER: float = -0.4189  # minimum steering angle [rad]
    MAX_STEER: float = 0.4189  # maximum steering angle [rad]
    MAX_DSTEER: float = np.deg2rad(180.0)  # maximum steering speed [rad/s]
    MAX_SPEED: float = 6.0  # maximum speed [m/s]
    MIN_SPEED: float = 0.0  # minimum backward speed [m/s]
    MAX_ACCEL: float = 3.0  # maximum acceleration [m/ss]
    # shooting parameters (not in the reference: its solver is a QP)
    N_ROLLOUTS: int = 512  # candidate control sequences per plan
    SIGMA_ACCEL: float = 1.5  # std of the acceleration samples [m/ss]
    SIGMA_STEER: float = 0.15  # std of the steering samples [rad]
    SEED: int = 0
    # solver: "shooting" (the default above) or "qp" -- the reference's own linearised QP (:283-450) solved exactly in fp64 on the GPU
    SOLVER: str = "shooting"
    QP_TOL: float = 1e-10  # interior point: scaled KKT residuals and duality gap below this
    QP_MAX_ITER: int = 50  # interior-point iterations at most (status 2 beyond: the last iterate, like cvxpy's OPTIMAL_INACCURATE)
    # occupancy test on the shooting solver's rollouts (set_map / load_map): a rollout through an occupied cell cannot win
    COLLISION: bool = False
    COLLISION_SUBSTEPS: int = 1  # tested points per time step, 1 .. 16 (a step covers up to MAX_SPEED * DTK metres)
    # SOLVER="qp" only: planner.obstacles / planner.rivals become soft, linearised half-plane rows of the QP
    # (repr=False: the config's repr is part of KMPCPlanner.__init__'s signature, a pinned record -- tests/test_runtime_calls.py)
    QP_AVOID: bool = field(default=False, repr=False)
    QP_AVOID_MARGIN: float = field(default=0.0, repr=False)  # added to every disc's radius [m]
    QP_AVOID_RHO: float = field(default=1e4, repr=False)  # the slack's quadratic penalty
    QP_AVOID_LIN: float = field(default=10.0, repr=False)  # the slack's linear penalty
    # SOLVER="qp" only: the occupancy grid of set_map / load_map as soft, linearised wall rows of the QP
    QP_WALLS: bool = field(default=False, repr=False)
    QP_WALL_REACH: float = field(default=1.5, repr=False)  # how far to each side a wall is looked for [m]: ceil(reach / (resolution / 2)) samples, <= 256
    QP_WALL_MARGIN: float = field(default=0.0, repr=False)  # kept between the path and the last free sample before the wall [m]


@dataclass
class State:
    x: float = 0.0
    y: float = 0.0
    delta: float = 0.0
    v: float = 0.0
    yaw: float = 0.0
    yawrate: float = 0.0
    beta: float = 0.0


def _fold_cyaw_inplace(cyaw, yaw):
    """The reference's heading fix-up (kinematic_mpc.py:198-203) with its exact semantics: IN PLACE on the caller's course-heading
    array, persistent across calls, the second mask evaluated after the first edit."""
    m = cyaw - yaw > 4.5
    cyaw[m] = np.abs(cyaw[m] - (2 * np.pi))
    m = cyaw - yaw < -4.5
    cyaw[m] = np.abs(cyaw[m] + (2 * np.pi))


class KMPCPlanner(MPCPlanner):
    """
    Kinematic MPC controller (random shooting on the GPU).  All poses are in the map frame.

    Args:
        waypoints: [x, y, yaw, v] as a list of four 1-D arrays or an array [4, N]
            (examples/control/kinematic_mpc.py:44-45)
        config (mpc_config)
    """
    _QP_WEIGHTS = (("Rk", 2), ("Rdk", 2), ("Qk", 4), ("Qfk", 4))
    _SUBSTEPS = ("COLLISION_SUBSTEPS",)
    _QP_WALLS = True

    def __init__(self, waypoints=None, config=mpc_config(),
                 params=np.array([3.74, 0.15875, 0.17145, 0.074, 4.718, 5.4562, 0.04712, 1.0489]), debug=False, device=None):
        self.waypoints = waypoints
        self.config = config
        self.vehicle_params = params
        self.odelta_v = None
        self.oa = None
        self.odelta = None
        self.init_flag = 0
        self.debug = debug
        self._device = device
        self._ctx = None
        self._calls = 0
        self._trk_qp_warm = None           # the QP warm start of the track-set path (plan_batch(tracks=...)): u [E, T, 2] fp64
        self._map = None                   # (img u8, resolution, (ox, oy), occupied_below) of set_map
        self._inflate = 0.0
        self.obstacles = None              # moving discs of the NEXT plan, which takes them: [M, 5] for plan(), [E, M, 5] for plan_batch()
        self._obstacles_set = False        # the context holds obstacles of an earlier plan
        self._qp_avoid_set = False         # the context's avoidance rows are switched on (mpc_config.QP_AVOID of an earlier plan)
        self._qp_walls_set = False         # ... and its wall rows (mpc_config.QP_WALLS of an earlier plan)
        self.rivals = None                 # Rivals(...): every plan_batch tests each ego against its nearest other vehicles; persistent
        self._rival_feed = RivalFeed("xyvyaw", lambda ctx: kmpc_set_obstacles_dev(ctx, None))
        self._check_solver()

    def _collision_switch(self, ctx, obstacles=None, rivals=None, x0=None, track_ids=None):
        """the occupancy switch and the obstacles of this plan (None clears them); COLLISION_SUBSTEPS serves both tests.  rivals: the slots
        are filled on the device from the call's x0 and the context borrows them"""
        c = self.config
        if c.SOLVER == "qp":
            av = qp_avoid(c)
            if av is not None or self._qp_avoid_set:             # (off after plans with it off: nothing to switch, no call -- as before QP_AVOID)
                kmpc_qp_set_avoid(ctx, av)                       # (None: off -- the QP then ignores whatever the context holds)
                self._qp_avoid_set = av is not None
            wl = qp_walls(c, self._map[1]) if c.QP_WALLS else None
            if wl is not None or self._qp_walls_set:
                kmpc_qp_set_walls(ctx, wl)
                self._qp_walls_set = wl is not None
        if c.SOLVER != "qp" or c.QP_AVOID:
            if c.SOLVER != "qp":
                tested = obstacles is not None or rivals is not None
                ctx.kmpc_set_collision(bool(c.COLLISION), int(c.COLLISION_SUBSTEPS) if (c.COLLISION or tested) else 1)
            if rivals is not None:
                d_obs, _, E, M = self._rival_feed.run(ctx, rivals, x0, horizon=(float(c.TK) * float(c.DTK), 0.0), track_ids=track_ids)
                kmpc_set_obstacles_dev(ctx, d_obs, E, M)
                self._obstacles_set = True
            elif obstacles is not None or self._obstacles_set:     # (a plan without any, after plans without any: nothing to clear)
                kmpc_set_obstacles(ctx, obstacles)
                self._obstacles_set = obstacles is not None

    def _bind(self, waypoints, fold_yaw=None):
        """fold_yaw: the vehicle heading of a single-vehicle call -- the course headings are then folded in place on the caller's
        array like the reference does (persistent state, :198-203) and the kernel's own stateless per-ego fold is switched off;
        None (batches): the kernel folds the gathered values per ego and the caller's array is left alone."""
        self._take_waypoints(waypoints, 3, "Waypoints needs to be a (Nxm), m >= 3, numpy array!", asarray=True)     # :131-132
        path = self.waypoints
        cx, cy, cyaw, sp = (np.asarray(path[k], dtype=np.float64) for k in range(4))             # :479-482
        ctx = self._context()
        if fold_yaw is not None:
            _fold_cyaw_inplace(cyaw, fold_yaw)                 # np.asarray of a float64 array is the caller's own array
        ctx.kmpc_set_yaw_fixup(fold_yaw is None)
        ctx.set_waypoints_cached(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
        return ctx

    def _sampler(self):
        c = self.config
        smp = _abi.kmpc_sampler(seed=c.SEED, call=self._calls, use_warm=True, sigma_accel=c.SIGMA_ACCEL, sigma_steer=c.SIGMA_STEER)
        self._calls += 1
        return smp

    def plan(self, states, waypoints=None):
        """
        states: [x, y, delta, v, yaw, yawrate, beta] (the 7-state of f110_gym, :139-147).
        self.obstacles: [M, 5] rows (x, y, vx, vy, r) of moving discs for this call (taken: None afterwards), or None.
        Returns (steering_angle, speed).
        """
        self._check_collision()
        obstacles = self._check_obstacles(self._take_obstacles(), 1, single=True)
        if self.rivals is not None:
            raise ValueError(SINGLE_EGO)
        ctx = self._bind(waypoints, fold_yaw=float(states[4]))
        self._collision_switch(ctx, obstacles)
        vehicle_state = State(x=states[0], y=states[1], delta=states[2], v=states[3], yaw=states[4], yawrate=states[5],
                              beta=states[6])
        x0 = np.array([[vehicle_state.x, vehicle_state.y, vehicle_state.v, vehicle_state.yaw]], dtype=np.float64)   # :487
        if self.config.SOLVER == "qp":
            out = self._qp(ctx, x0)
            st = int(out["status"][0])
            if st in (1, 3):        # the reference cannot go on either: its oa / odelta_v are None (:444-448, :500-505)
                raise RuntimeError("kinematic MPC QP: " + ("infeasible (speed outside [MIN_SPEED, MAX_SPEED])" if st == 1 else "non-finite input"))
            self.oa = out["u"][0, :, 0]                        # fp64; the next call linearises about them (device-resident copy)
            self.odelta_v = out["u"][0, :, 1]
            return float(out["steer"][0]), float(out["speed"][0])
        out = self._shoot(ctx, x0)
        if int(out["best_idx"][0]) < 0:        # every rollout runs into an occupied cell: a soft failure like pure pursuit's, (0, 0)
            warnings.warn("kinematic MPC: every rollout is blocked by the occupancy grid; returning (0.0, 0.0)", RuntimeWarning, stacklevel=2)
            self.oa = out["best_seq"][0, :, 0]
            self.odelta_v = out["best_seq"][0, :, 1]
            return 0.0, 0.0
        self.oa = out["best_seq"][0, :, 0]                 # the reference's attributes (:108-110); the warm start itself lives on the device
        self.odelta_v = out["best_seq"][0, :, 1]
        return float(out["steer"][0]), float(out["speed"][0])

    def _shoot(self, ctx, x0, want_seq=True):
        """One C call per plan (f1p_kmpc_plan_batch): reference extraction (:162-206), R candidate sequences generated IN THE
        KERNEL around the context's device-resident warm start (previous solution shifted by one step, :491-498; rollout 0 is the
        unperturbed warm start, rollout 1 all zero), rollouts, argmin, output map, new warm start.  Up: 32 B per ego.  Down: the
        winners.  The warm start belongs to (context, batch size): switching between plan() and plan_batch() sizes restarts it."""
        c = self.config
        return ctx.kmpc_plan(x0, _cfg_struct(c), self._sampler(), dl=c.dlk, want_seq=want_seq)

    def _qp(self, ctx, x0, want_u=True):
        """One C call per plan (f1p_kmpc_qp_plan_batch): reference extraction (:162-206), linearisation about the previous solution held
        on the device (unshifted, :462-468), the QP of :283-450 solved to tolerance, output map (:500-505), new warm start."""
        c = self.config
        return ctx.kmpc_qp_plan(x0, _cfg_struct(c), dl=c.dlk, opts=qp_opts(c), want_u=want_u)

    def reset(self):
        """forget the warm starts (shooting and QP) and restart the sampler's call counter (a new episode)"""
        self._calls = 0
        self.oa = self.odelta_v = None
        self._trk_qp_warm = None
        if self._ctx is not None:
            self._ctx.kmpc_warm_reset()
            self._ctx.kmpc_qp_warm_reset()

    def plan_batch(self, x0, waypoints=None, controls=None, want_seq=True, tracks=None, track_ids=None):
        """x0 [E, 4] = (x, y, v, yaw) -> dict(steer, speed, best_idx, best_cost[, best_seq]).  `controls`
        (f32 [E, T, 2, R]) overrides the in-kernel sampler with a caller-supplied candidate set (streamed from HBM).
        SOLVER == "qp": dict(steer, speed, status, obj[, u [E, T, 2]]) -- per-ego status (0 solved, 1 infeasible, 2 not converged,
        3 non-finite input), never raised.
        mpc_config.COLLISION: an ego whose rollouts are all blocked has best_idx -1, best_cost +inf, steer 0, speed 0 and a zero sequence.
        tracks: K courses in the `waypoints` format ([x, y, yaw, v]: four 1-D arrays or an array [4, N]) with track_ids [E]: ego e
        follows tracks[track_ids[e]]; `waypoints` is then not used.  The references come from one k_kmpc_ref_tracks launch (an id
        outside [0, K) gives NaN rows, hence NaN outputs and QP status 3 for that ego) and go to the same solvers.
        self.obstacles (taken by this call: None afterwards): [E, M, 5] rows (x, y, vx, vy, r) of moving discs per ego (M <= 16, r < 0 or NaN: empty), tested at COLLISION_SUBSTEPS
        points per step whether COLLISION is on or not; None: none.  All-blocked egos as with COLLISION.
        self.rivals (persistent): Rivals(count, radius[, reach, groups]): each ego's nearest other vehicles of x0 take the obstacle slots."""
        self._check_collision()
        if self.config.SOLVER == "qp" and controls is not None:
            raise ValueError("controls are candidates of the shooting solver; SOLVER='qp' takes none")
        obstacles = self._take_obstacles()
        if obstacles is not None:
            obstacles = self._check_obstacles(obstacles, np.asarray(x0).reshape(-1, 4).shape[0])
        rivals = self.rivals
        if rivals is not None:
            self._check_rivals(rivals, np.asarray(x0).reshape(-1, 4).shape[0], obstacles)
        if tracks is not None:
            return self._plan_tracks(x0, tracks, track_ids, controls, want_seq, obstacles, rivals)
        ctx = self._bind(waypoints)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, 4)
        self._collision_switch(ctx, obstacles, rivals, x0)
        if self.config.SOLVER == "qp":
            return self._qp(ctx, x0, want_u=want_seq)
        if controls is None:
            return self._shoot(ctx, x0, want_seq=want_seq)
        c = self.config
        cfg = _cfg_struct(c, n_rollouts=controls.shape[3])
        ref = ctx.kmpc_ref(x0, c.TK, c.DTK, c.dlk)
        return ctx.kmpc_shoot(x0, ref, controls, cfg)

    def _plan_tracks(self, x0, tracks, track_ids, controls, want_seq, obstacles=None, rivals=None):
        cols = _track_columns(tracks, track_ids)
        ctx = self._context()
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, 4)
        if rivals is not None and rivals.predict == "track":   # the rivals are predicted along the call's tracks: the set is on the context first
            ctx.set_tracks_cached(cols, cols=(0, 1, 2, 3))
        self._collision_switch(ctx, obstacles, rivals, x0, track_ids)
        ctx.kmpc_set_yaw_fixup(True)                           # a batch: per-ego fold of the gathered headings, the courses stay as given
        ctx.set_tracks_cached(cols, cols=(0, 1, 2, 3))
        c = self.config
        E, T = x0.shape[0], c.TK
        ids = Context._ids(track_ids, E)
        if controls is not None:
            cfg = _cfg_struct(c, n_rollouts=controls.shape[3])
            return ctx.kmpc_shoot(x0, ctx.kmpc_ref_tracks(x0, ids, T, c.DTK, c.dlk), controls, cfg)
        d = self._track_buffers(ctx, E, T)
        d["x0"].upload(x0)
        d["ids"].upload(ids)
        ctx.kmpc_ref_tracks_dev(d["x0"], d["ids"], E, T, d["ref"], c.DTK, c.dlk)            # calc_ref_trajectory_kinematic :162-206
        if c.SOLVER == "qp":
            # the warm start of the single-track path (f1p_kmpc_qp_plan_batch): the previous call's solution, unshifted, per (E, T); a failed
            # solve (status 1 / 3) leaves zeros, the reference's None
            warm = self._trk_qp_warm if self._trk_qp_warm is not None and self._trk_qp_warm.shape == (E, T, 2) else None
            if warm is not None:
                d["oa"].upload(np.ascontiguousarray(warm[:, :, 0]))
                d["od"].upload(np.ascontiguousarray(warm[:, :, 1]))
            ctx.kmpc_qp_dev(d["x0"], d["ref"], E, _cfg_struct(c), d["steer"], d["speed"], d["status"],
                            d["oa"] if warm is not None else None, d["od"] if warm is not None else None, opts=qp_opts(c), d_u=d["u"],
                            d_obj=d["obj"])
            out = dict(steer=d["steer"].download(np.float64, E), speed=d["speed"].download(np.float64, E),
                       status=d["status"].download(np.int32, E), obj=d["obj"].download(np.float64, E))
            u = d["u"].download(np.float64, (E, T, 2))
            nw = u.copy()
            nw[(out["status"] == 1) | (out["status"] == 3)] = 0.0
            self._trk_qp_warm = nw
            if want_seq:
                out["u"] = u
            return out
        ctx.kmpc_plan_dev(d["x0"], d["ref"], E, _cfg_struct(c), self._sampler(), d["steer"], d["speed"], d["best_idx"], d["best_cost"],
                          d["best_seq"] if want_seq else None)
        out = dict(steer=d["steer"].download(np.float64, E), speed=d["speed"].download(np.float64, E),
                   best_idx=d["best_idx"].download(np.int32, E), best_cost=d["best_cost"].download(np.float64, E))
        if want_seq:
            out["best_seq"] = d["best_seq"].download(np.float64, (E, T, 2))
        return out

    def _track_buffers(self, ctx, E, T):
        """device buffers of the track-set path, kept per (context, E, T)"""
        key = (id(ctx), E, T)
        if getattr(self, "_trk_key", None) != key:
            for b in getattr(self, "_trk_bufs", {}).values():
                b.free()
            n = max(E, 1)
            sizes = dict(x0=32 * n, ids=4 * n, ref=32 * n * (T + 1), oa=8 * n * T, od=8 * n * T, steer=8 * n, speed=8 * n, status=4 * n,
                         u=16 * n * T, obj=8 * n, best_idx=4 * n, best_cost=8 * n, best_seq=16 * n * T)
            self._trk_bufs = {k: ctx.alloc(v) for k, v in sizes.items()}
            self._trk_key = key
        return self._trk_bufs

    # the reference's helper methods, on the GPU ---------------------------------------------------------------------
    def predict_motion_kinematic(self, x0, oa, od, xref=None):
        """Open-loop rollout [4, T+1] of update_state_kinematic for the controls (oa, od) (:208-221)."""
        c = self.config
        cfg = _cfg_struct(c)
        cfg.horizon = len(oa)
        return self._context().kmpc_predict(np.asarray(x0, dtype=np.float64)[None, :], np.asarray(oa, dtype=np.float64)[None, :],
                                            np.asarray(od, dtype=np.float64)[None, :], cfg)[0]

    def calc_ref_trajectory_kinematic(self, state, cx, cy, cyaw, sp):
        """Reference trajectory [4, T+1] (rows x, y, v, yaw) along the course from the nearest point (:162-206).  Like the
        reference, a writable `cyaw` array is folded IN PLACE (:198-203) -- repeated calls with one array see the earlier
        calls' edits (golden G15: a sequence whose heading representation jumps by +-2 pi)."""
        ctx = self._context()
        if isinstance(cyaw, np.ndarray) and cyaw.dtype == np.float64 and cyaw.flags.writeable:
            _fold_cyaw_inplace(cyaw, state.yaw)
            ctx.kmpc_set_yaw_fixup(False)
        else:                                                  # a list / read-only view: stateless fold on the device
            ctx.kmpc_set_yaw_fixup(True)
        ctx.set_waypoints_cached(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
        c = self.config
        return ctx.kmpc_ref(np.array([[state.x, state.y, state.v, state.yaw]], dtype=np.float64), c.TK, c.DTK, c.dlk)[0]

    def update_state_kinematic(self, state, a, delta):
        """One explicit-Euler step of the kinematic bicycle (:223-243) on the GPU (k_kmpc_predict with a one-step horizon):
        steering clamped to +-MAX_STEER, x / y / yaw advanced with the OLD speed and heading, then the speed, clamped to
        [MIN_SPEED, MAX_SPEED]; `a` is not clamped.  Mutates and returns `state` like the reference."""
        cfg = _cfg_struct(self.config)
        cfg.horizon = 1
        path = self._context().kmpc_predict(np.array([[state.x, state.y, state.v, state.yaw]], dtype=np.float64),
                                            np.array([[a]], dtype=np.float64), np.array([[delta]], dtype=np.float64), cfg)[0]
        state.x, state.y, state.v, state.yaw = (float(path[k, 1]) for k in range(4))
        return state
