"""STMPCPlanner on the MI355X path: single-track MPC solved by random shooting.

Same class names (`mpc_config`, `State`, `STMPCPlanner`), constructor and `plan(states, waypoints=None)` signature as the
reference (f1tenth_planning/control/dynamic_mpc/dynamic_mpc.py:40-191).  Like the reference it switches on the speed:
at or below V_KS the kinematic model is used (:168-180), above it the dynamic single-track model (:181-191).  Both are
solved by rolling R sampled control sequences through the reference's own nonlinear step on the GPU (csrc/k_kmpc.hip,
csrc/k_stmpc.hip) instead of the reference's cvxpy/OSQP QP (third-party, out of scope).

mpc_config.SOLVER = "qp" selects the reference's own solver instead: the linearised QPs of :575-833, solved exactly (to QP_TOL) by
batched fp64 interior-point kernels -- csrc/k_stmpc_qp.hip for the dynamic branch, csrc/k_kmpc_qp.hip for the kinematic one --
warm-started like the reference from the previous solution (unshifted, with its reset rules :1005, :1052).

mpc_config.COLLISION = True (shooting only) tests every rollout of both branches against the occupancy grid installed with set_map /
load_map: a rollout that touches an occupied cell cannot win (f1p_stmpc_set_collision).

planner.obstacles = [M, 5] before plan() / [E, M, 5] before plan_batch() (shooting only) tests every rollout of THAT call, whichever branch
an ego takes, against moving discs: rows (x, y, vx, vy, r) in the map frame at constant velocity, M <= 16, r < 0 or NaN = an empty slot,
row e of a batch for ego e of `states`.  A rollout that is inside a disc at the time it gets there cannot win (f1p_stmpc_set_obstacles,
DESIGN.md 5k).  The next plan / plan_batch call TAKES the attribute: it is None again afterwards -- KMPCPlanner's contract.

planner.rivals = Rivals(count=M, radius=r[, reach, groups]) (shooting only, plan_batch only): while it is set, every plan_batch finds each
ego's M nearest other vehicles of its race among the call's own states on the device (heading yaw + beta; f1p_rivals_dev) and
tests the rollouts of both branches against them.  Persistent until set to None; not together with `obstacles`.
predict="track" predicts each rival along the planner's raceline over max(T * DT, TK * DTK) seconds, one value for both branches
(f1p_rivals_predict_dev); with speed="profile" the rival moves with the raceline's speed column, scaled by its speed now
(DESIGN.md 5u).

mpc_config.QP_AVOID = True (SOLVER="qp" only) lets the QP take `obstacles` (plan and plan_batch) and `rivals` (plan_batch, with and without
`tracks`) as well: in both branches the two discs nearest to the previous solution's path become, per step, half-plane rows of the QP,
softened by one slack variable with the cost QP_AVOID_RHO eps^2 + QP_AVOID_LIN eps (f1p_stmpc_qp_set_avoid).  The rows are
linearised and soft -- an avoidance term, not a guarantee; QP_AVOID_MARGIN [m] widens every disc.  T <= 40, TK <= 31.

mpc_config.QP_WALLS_ST = True (SOLVER="qp" only, needs set_map / load_map) lets both branches' QPs see the map: per step the walls found within
QP_WALL_REACH metres to the left and to the right of the previous solution's path -- of its direction of travel yaw + beta in the dynamic
branch -- on the occupancy grid as inflated by set_map(inflate=...) compete with the discs for the step's two half-plane rows
(f1p_stmpc_qp_set_walls).  Soft and linearised like the discs' rows and under the same slack; QP_WALL_MARGIN [m] keeps the rows
that far off the contact.  Works with plan, plan_batch, tracks, obstacles and rivals, with or without QP_AVOID.  T <= 40, TK <= 31.  (The
field is not called QP_WALLS: that name was KMPCPlanner's first and raises here, a pinned behaviour.)
"""
import warnings
from dataclasses import dataclass, field

import numpy as np

from ... import _abi
from ..._planner import MPCPlanner, _course_columns, _diag, _track_columns, kin_cfg_struct, qp_avoid, qp_opts, qp_walls
from ..._rivals import SINGLE_EGO, RivalFeed
from ...runtime import Context, kmpc_set_obstacles, stmpc_qp_set_avoid, stmpc_qp_set_walls, stmpc_set_obstacles, stmpc_set_obstacles_dev
from ..kinematic_mpc.kinematic_mpc import State  # noqa: F401  (same 7-field dataclass, :89-98)


@dataclass
class mpc_config:
    NX: int = 7  # length of state vector: z = [x, y, delta, v, yaw, yaw rate, beta]
    NXK: int = 4  # length of kinematic state vector: z = [x, y, v, yaw]
    NU: int = 2  # length of input vector: u = [steering speed, acceleration]
    T: int = 40  # finite time horizon length
    TK: int = 8  # finite time horizon length kinematic
    R: list = field(default_factory=lambda: np.diag([0.5, 0.01]))     # input cost [steering_speed, accel]
    Rd: list = field(default_factory=lambda: np.diag([0.3, 0.01]))    # input difference cost
    Q: list = field(default_factory=lambda: np.diag([32.0, 32.0, 0.0, 1.0, 0.5, 0.0, 0.0]))    # state error cost
    Qf: list = field(default_factory=lambda: np.diag([32.0, 32.0, 0.0, 1.0, 0.5, 0.0, 0.0]))   # final state error cost
    Rk: list = field(default_factory=lambda: np.diag([0.01, 100.0]))  # kinematic input cost [accel, steer]
    Rdk: list = field(default_factory=lambda: np.diag([0.01, 100.0]))
    Qk: list = field(default_factory=lambda: np.diag([13.5, 13.5, 5.5, 13.0]))
    Qfk: list = field(default_factory=lambda: np.diag([13.5, 13.5, 5.5, 13.0]))
    N_IND_SEARCH: int = 20
    DT: float = 0.025  # time step [s]
    DTK: float = 0.1  # time step [s] kinematic
    dl: float = 0.03  # dist step [m]
    dlk: float = 0.03  # dist step [m] kinematic
    LENGTH: float = 0.58
    WIDTH: float = 0.31
    WB: float = 0.33
    MIN_STEER: float = -0.4189
    MAX_STEER: float = 0.4189
    MAX_DSTEER: float = np.deg2rad(180.0)
    MAX_STEER_V: float = 3.2  # maximum steering speed [rad/s]
    MAX_SPEED: float = 6.0
    MIN_SPEED: float = 0.0
    MAX_ACCEL: float = 3.0
    V_KS: float = 2.0  # switching velocity from kinematic to dynamic [m/s]
    # shooting parameters (not in the reference: its solver is a QP)
    N_ROLLOUTS: int = 512
    SIGMA_STEER_V: float = 1.0   # std of the steering-speed samples [rad/s]
    SIGMA_ACCEL: float = 1.5     # std of the acceleration samples [m/ss]
    SIGMA_STEER: float = 0.15    # std of the steering samples of the kinematic branch [rad]
    SEED: int = 0
    # solver: "shooting" (the default above) or "qp" -- the reference's own linearised QPs (:575-833) solved exactly in fp64 on the GPU
    SOLVER: str = "shooting"
    QP_TOL: float = 1e-10  # interior point: scaled KKT residuals and duality gap below this
    QP_MAX_ITER: int = 50  # interior-point iterations at most (status 2 beyond: the last iterate, like cvxpy's OPTIMAL_INACCURATE)
    # occupancy test on the shooting solver's rollouts (set_map / load_map): a rollout through an occupied cell cannot win
    COLLISION: bool = False
    COLLISION_SUBSTEPS: int = 1    # tested points per step of the dynamic model, 1 .. 16 (a step covers up to MAX_SPEED * DT = 0.15 m)
    COLLISION_SUBSTEPS_K: int = 2  # ... per step of the kinematic branch, 1 .. 16 (up to V_KS * DTK + acceleration)
    # SOLVER="qp" only: planner.obstacles / planner.rivals become soft, linearised half-plane rows of both branches' QPs
    # (repr=False: the config's repr is part of STMPCPlanner.__init__'s signature, a pinned record -- tests/test_runtime_calls.py)
    QP_AVOID: bool = field(default=False, repr=False)
    QP_AVOID_MARGIN: float = field(default=0.0, repr=False)  # added to every disc's radius [m]
    QP_AVOID_RHO: float = field(default=1e4, repr=False)  # the slack's quadratic penalty
    QP_AVOID_LIN: float = field(default=10.0, repr=False)  # the slack's linear penalty
    QP_WALLS: bool = field(default=False, repr=False)  # the kinematic QP's wall rows: KMPCPlanner only, True raises here
    # SOLVER="qp" only: the occupancy grid of set_map / load_map as soft, linearised wall rows of both branches' QPs.  Not
    # QP_WALLS: that field raises "KMPCPlanner only" here, which tests/test_kmpc_qp_walls_host.py pins, so this planner's switch has a name of its own
    QP_WALLS_ST: bool = field(default=False, repr=False)
    QP_WALL_REACH: float = field(default=1.5, repr=False)  # how far to each side a wall is looked for [m]: ceil(reach / (resolution / 2)) samples, <= 256
    QP_WALL_MARGIN: float = field(default=0.0, repr=False)  # kept between the path and the last free sample before the wall [m]


class STMPCPlanner(MPCPlanner):
    """
    Single-track MPC controller (random shooting on the GPU).  All poses are in the map frame.

    Args:
        waypoints: [x, y, yaw, v] as a list of four 1-D arrays or an array [4, N] (examples/control/dynamic_mpc.py)
        config (mpc_config)
        params: mass, l_f, l_r, h_CoG, c_f, c_r, Iz, mu
    """
    _QP_WEIGHTS = (("R", 2), ("Rd", 2), ("Q", 7), ("Qf", 7), ("Rk", 2), ("Rdk", 2), ("Qk", 4), ("Qfk", 4))
    _SUBSTEPS = ("COLLISION_SUBSTEPS", "COLLISION_SUBSTEPS_K")
    _TK_WITHIN_T = True
    _QP_AVOID_MAX_T = _abi.STMPC_QP_AVOID_MAX_T
    _QP_WALLS_ST = True

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
        self._batch_calls = 0
        self._map = None                   # (img u8, resolution, (ox, oy), occupied_below) of set_map
        self._inflate = 0.0
        self.obstacles = None              # moving discs of the NEXT plan, which takes them: [M, 5] for plan(), [E, M, 5] for plan_batch()
        self._obstacles_set = [False, False]   # the context holds obstacles of an earlier plan: the kmpc state, the stmpc state
        self._qp_avoid_set = False         # the context's avoidance rows are switched on (mpc_config.QP_AVOID of an earlier plan)
        self._qp_walls_set = False         # ... and its wall rows (mpc_config.QP_WALLS_ST of an earlier plan)
        self.rivals = None                 # Rivals(...): every plan_batch tests each ego against its nearest other vehicles; persistent
        self._rival_feed = RivalFeed("st7", lambda ctx: stmpc_set_obstacles_dev(ctx, None))
        self._check_solver()

    def _collision_switch(self, ctx, obstacles=None, kinematic=False, rivals=None, states=None, track_ids=None):
        """the planner's context follows mpc_config: the stmpc switch (plan_batch, plan()'s dynamic branch) and, for plan()'s kinematic
        branch through ctx.kmpc_shoot, the kmpc switch with COLLISION_SUBSTEPS_K.  The obstacles of this plan (None clears them) go to
        the stmpc state, or (kinematic: plan()'s kinematic branch) to the kmpc state; the substep counts serve both tests"""
        c = self.config
        if c.SOLVER == "qp":
            av = qp_avoid(c)
            if av is not None or self._qp_avoid_set:             # (off after plans with it off: nothing to switch, no call -- as before QP_AVOID)
                stmpc_qp_set_avoid(ctx, av)                      # (None: off -- the QP then ignores whatever the context holds)
                self._qp_avoid_set = av is not None
            wl = qp_walls(c, self._map[1]) if c.QP_WALLS_ST else None
            if wl is not None or self._qp_walls_set:
                stmpc_qp_set_walls(ctx, wl)
                self._qp_walls_set = wl is not None
            if av is not None:                                   # both branches of the QP plan read the stmpc state, in the caller's order
                if rivals is not None:
                    d_obs, _, E, M = self._rival_feed.run(ctx, rivals, states, horizon=(max(float(c.T) * float(c.DT), float(c.TK) * float(c.DTK)), 0.0),
                                                          track_ids=track_ids)
                    stmpc_set_obstacles_dev(ctx, d_obs, E, M)
                    self._obstacles_set[1] = True
                elif obstacles is not None or self._obstacles_set[1]:
                    stmpc_set_obstacles(ctx, obstacles)
                    self._obstacles_set[1] = obstacles is not None
        if c.SOLVER != "qp":
            on = bool(c.COLLISION)
            sub = on or obstacles is not None or rivals is not None
            ctx.stmpc_set_collision(on, int(c.COLLISION_SUBSTEPS) if sub else 1, int(c.COLLISION_SUBSTEPS_K) if sub else 2)
            ctx.kmpc_set_collision(on, int(c.COLLISION_SUBSTEPS_K) if sub else 1)
            for k, setter in ((0, kmpc_set_obstacles), (1, stmpc_set_obstacles)):
                if k == 1 and rivals is not None:                 # (plan_batch: the stmpc state; the slots are filled on the device from the call's states)
                    d_obs, _, E, M = self._rival_feed.run(ctx, rivals, states, horizon=(max(float(c.T) * float(c.DT), float(c.TK) * float(c.DTK)), 0.0))
                    stmpc_set_obstacles_dev(ctx, d_obs, E, M)
                    self._obstacles_set[k] = True
                    continue
                o = obstacles if k == (0 if kinematic else 1) else None
                if o is not None or self._obstacles_set[k]:       # (a plan without any, after plans without any: nothing to clear)
                    setter(ctx, o)
                    self._obstacles_set[k] = o is not None

    def _bind(self, waypoints):
        self._take_waypoints(waypoints, 3, "Waypoints needs to be a (Nxm), m >= 3, numpy array!", asarray=True)
        cols = _course_columns(self.waypoints)
        ctx = self._context()
        ctx.set_waypoints_cached(cols, cols=(0, 1, 2, 3))
        return ctx

    def _dyn_cfg(self):
        c = self.config
        return _abi.stmpc_cfg(horizon=c.T, n_rollouts=c.N_ROLLOUTS, dt=c.DT, wheelbase=c.WB, max_steer=c.MAX_STEER,
                              max_steer_v=c.MAX_STEER_V, max_speed=c.MAX_SPEED, min_speed=c.MIN_SPEED, max_accel=c.MAX_ACCEL,
                              q=_diag(c.Q), qf=_diag(c.Qf), r=_diag(c.R), rd=_diag(c.Rd), params=self.vehicle_params)

    def _kin_cfg(self):
        return kin_cfg_struct(self.config)

    def _sample(self, T, R, s0, s1, lim0, lim1):
        rng = np.random.default_rng([self.config.SEED, self._calls])
        self._calls += 1
        ctrl = np.empty((1, T, 2, R), dtype=np.float32)
        ctrl[0, :, 0, :] = np.clip(rng.normal(0.0, s0, (T, R)), -lim0, lim0)
        ctrl[0, :, 1, :] = np.clip(rng.normal(0.0, s1, (T, R)), -lim1, lim1)
        ctrl[0, :, :, 0] = 0.0                                    # rollout 0: coast
        return ctrl

    def _qp(self, ctx, x0, want_u=True):
        """One C call per plan (f1p_stmpc_qp_plan_batch): per ego the branch (:168), reference extraction (:195-276), linearisation about
        the previous solution held on the device (unshifted, reset by the rules of :1005 / :1052), the branch's QP solved to tolerance,
        output map (:1112-1117, :1205-1207), new warm start."""
        c = self.config
        return ctx.stmpc_qp_plan(x0, self._dyn_cfg(), self._kin_cfg(), v_ks=c.V_KS, dl=c.dl, dlk=c.dlk,
                                 opts=qp_opts(c), want_u=want_u)

    def _shoot(self, ctx, x0, want_u=True):
        """One C call per plan (f1p_stmpc_plan_batch): per ego the branch (:168), reference extraction (:195-276), R control sequences
        generated in the kernels around the ego's warm start on the device (call counter = plans since reset()), rollouts through the
        branch's model, argmin, output map (:1112-1117, :1205-1207), new warm start."""
        c = self.config
        smp = _abi.stmpc_sampler(seed=c.SEED, call=self._batch_calls, use_warm=True, sigma_steer_v=c.SIGMA_STEER_V, sigma_accel=c.SIGMA_ACCEL,
                                 sigma_steer=c.SIGMA_STEER)
        out = ctx.stmpc_plan(x0, self._dyn_cfg(), self._kin_cfg(), smp, v_ks=c.V_KS, dl=c.dl, dlk=c.dlk, want_seq=want_u)
        self._batch_calls += 1
        if want_u:
            out["u"] = out.pop("best_seq")
        return out

    def plan_batch(self, states, waypoints=None, want_u=True, tracks=None, track_ids=None):
        """SOLVER == "shooting" (the default): states [E, 7] -> dict(steer, speed, best_idx, best_cost, branch (1 dynamic, 0 kinematic)[, u
        [E, max(T, TK), 2] = the winner's applied sequence, (steering speed, accel) in the dynamic branch and (accel, steer) in the
        kinematic one, NaN past the branch's horizon]).  One C call: the controls are generated in the kernels (Philox, seeded by
        mpc_config.SEED and the number of plans since reset()) around each ego's own warm start, which lives on the device -- the previous
        winner shifted by one step; an ego that crosses V_KS starts its new branch from zeros.  An ego's result depends on that ego's state
        and history alone, not on the batch around it.  plan() keeps its host-side sampler and has no warm start; a one-ego plan_batch is
        the warm-started single-vehicle call.  `tracks` needs SOLVER='qp' (below).
        mpc_config.COLLISION: every rollout of both branches is tested against the map; an ego whose rollouts are all blocked has best_idx
        -1, best_cost +inf, steer 0, speed 0, a zero sequence (up to its branch's horizon) and starts its next plan from a zero warm start.
        self.obstacles (taken by this call: None afterwards): [E, M, 5] rows (x, y, vx, vy, r) of moving discs, row e for ego e of `states`
        whichever branch it takes (M <= 16, r < 0 or NaN: empty), tested at COLLISION_SUBSTEPS / COLLISION_SUBSTEPS_K points per step
        whether COLLISION is on or not; None: none.  All-blocked egos as with COLLISION.
        SOLVER == "qp": states [E, 7] -> dict(steer, speed, status, branch (1 dynamic, 0 kinematic), obj[, u [E, max(T, TK), 2] =
        (oa, odelta_v), NaN past the branch's horizon]) -- per-ego status (0 solved, 1 infeasible, 2 not converged, 3 non-finite input
        or model data), never raised.
        tracks: K courses in the `waypoints` format ([x, y, yaw, v]: four 1-D arrays or an array [4, N]) with track_ids [E]: ego e
        follows tracks[track_ids[e]] (f1p_stmpc_qp_plan_tracks_batch); `waypoints` is then not used and the raceline stays as it is.
        The warm start is the one plan() and the raceline batch use: it follows the ego, not the track.  An id outside [0, K) gives
        that ego status 4 (F1P_ST_BAD_TRACK), branch -1 and NaN outputs, and leaves its warm start as it was.  The shooting solver on
        tracks is a Context-level chain: ctx.stmpc_ref_tracks -> ctx.stmpc_shoot, or its rows [0, 1, 3, 4] with (TK, DTK, dlk) ->
        ctx.kmpc_shoot for the kinematic branch."""
        self._check_collision()
        obstacles = self._take_obstacles()
        if obstacles is not None:
            obstacles = self._check_obstacles(obstacles, np.asarray(states).reshape(-1, 7).shape[0])
        rivals = self.rivals
        if rivals is not None:
            self._check_rivals(rivals, np.asarray(states).reshape(-1, 7).shape[0], obstacles)
        if self.config.SOLVER != "qp":
            if tracks is not None:
                raise ValueError("plan_batch with tracks needs SOLVER='qp'")
            ctx = self._bind(waypoints)
            x0 = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 7)
            self._collision_switch(ctx, obstacles, rivals=rivals, states=x0)
            return self._shoot(ctx, x0, want_u=want_u)
        if tracks is not None:
            cols = _track_columns(tracks, track_ids)
            ctx = self._context()
            ctx.set_tracks_cached(cols, cols=(0, 1, 2, 3))
            x0 = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 7)
            c = self.config
            self._collision_switch(ctx, obstacles, rivals=rivals, states=x0, track_ids=track_ids)
            return ctx.stmpc_qp_plan_tracks(x0, Context._ids(track_ids, x0.shape[0]), self._dyn_cfg(), self._kin_cfg(), v_ks=c.V_KS,
                                            dl=c.dl, dlk=c.dlk, opts=qp_opts(c), want_u=want_u)
        ctx = self._bind(waypoints)
        x0 = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 7)
        self._collision_switch(ctx, obstacles, rivals=rivals, states=x0)
        return self._qp(ctx, x0, want_u=want_u)

    def reset(self):
        """forget the warm start (a new episode)"""
        self._calls = 0
        self._batch_calls = 0
        self.oa = self.odelta_v = None
        if self._ctx is not None:
            self._ctx.stmpc_qp_warm_reset()
            self._ctx.stmpc_warm_reset()

    def plan(self, states, waypoints=None):
        """states: [x, y, delta, v, yaw, yawrate, beta].  Returns (steering_angle, speed).  mpc_config.COLLISION: the rollouts of the
        branch taken are tested against the map; when every one of them is blocked the call warns and returns (0.0, 0.0) -- a soft failure
        like KMPCPlanner's -- and oa / odelta_v are the zero sequence.
        self.obstacles: [M, 5] rows (x, y, vx, vy, r) of moving discs for this call (taken: None afterwards), or None; tested in the branch
        taken, an all-blocked plan warns and returns (0.0, 0.0) likewise."""
        self._check_collision()
        obstacles = self._check_obstacles(self._take_obstacles(), 1, single=True)
        if self.rivals is not None:
            raise ValueError(SINGLE_EGO)
        ctx = self._bind(waypoints)
        c = self.config
        st = np.asarray(states, dtype=np.float64)
        self._collision_switch(ctx, obstacles, kinematic=bool(st[3] <= c.V_KS))
        if c.SOLVER == "qp":
            out = self._qp(ctx, st[None, :7])
            s = int(out["status"][0])
            if s in (1, 3):         # the reference cannot go on either: its oa / odelta_v are None (:1112, :1205)
                raise RuntimeError("dynamic MPC QP: " + ("infeasible (steering or speed outside its bounds)" if s == 1 else
                                                         "non-finite input or model data"))
            n = c.T if out["branch"][0] else c.TK
            self.oa, self.odelta_v = out["u"][0, :n, 0].copy(), out["u"][0, :n, 1].copy()
            return float(out["steer"][0]), float(out["speed"][0])
        if st[3] <= c.V_KS:                                      # kinematic branch (:168-180)
            cfg = self._kin_cfg()
            x0 = np.array([[st[0], st[1], st[3], st[4]]])
            # STMPCPlanner's own calc_ref_trajectory_kinematic (dynamic_mpc.py:236-276): same gathers as the dynamic one with
            # (TK, DTK, dlk) and ITS yaw fix-up threshold of 5 (:273-274) -- not KMPCPlanner's 4.5 (kinematic_mpc.py:198-203)
            ref = np.ascontiguousarray(ctx.stmpc_ref(x0, c.TK, c.DTK, c.dlk)[:, [0, 1, 3, 4]])
            out = ctx.kmpc_shoot(x0, ref, self._sample(c.TK, c.N_ROLLOUTS, c.SIGMA_ACCEL, c.SIGMA_STEER, c.MAX_ACCEL, c.MAX_STEER), cfg)
            self.oa, self.odelta_v = out["best_seq"][0, :, 0], out["best_seq"][0, :, 1]
        else:                                                    # dynamic branch (:181-191)
            cfg = self._dyn_cfg()
            ref = ctx.stmpc_ref(np.array([[st[0], st[1], st[3], st[4]]]), c.T, c.DT, c.dl)
            out = ctx.stmpc_shoot(st[None, :7], ref, self._sample(c.T, c.N_ROLLOUTS, c.SIGMA_STEER_V, c.SIGMA_ACCEL, c.MAX_STEER_V, c.MAX_ACCEL), cfg)
            self.odelta_v, self.oa = out["best_seq"][0, :, 0], out["best_seq"][0, :, 1]
        if int(out["best_idx"][0]) < 0:        # every rollout runs into an occupied cell or a disc
            warnings.warn("dynamic MPC: every rollout is blocked by the " + ("occupancy grid" if obstacles is None else "obstacles or the occupancy grid") +
                          "; returning (0.0, 0.0)", RuntimeWarning, stacklevel=2)
            return 0.0, 0.0
        return float(out["steer"][0]), float(out["speed"][0])

    # the reference's helper methods, on the GPU ---------------------------------------------------------------------
    def predict_motion(self, x0, oa, od_v, xref=None, vehicle_params=None):
        """Open-loop rollout [7, T+1] of update_state (:280-300)."""
        cfg = self._dyn_cfg()
        if vehicle_params is not None:
            for i in range(8):
                cfg.params[i] = float(vehicle_params[i])
        cfg.horizon = len(oa)
        return self._context().stmpc_predict(np.asarray(x0, dtype=np.float64)[None, :], np.asarray(oa, dtype=np.float64)[None, :],
                                             np.asarray(od_v, dtype=np.float64)[None, :], cfg)[0]

    def calc_ref_trajectory(self, state, cx, cy, cyaw, sp):
        """Reference trajectory [7, T+1] (:195-233); the caller's cyaw array is not modified."""
        ctx = self._context()
        ctx.set_waypoints_cached(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
        c = self.config
        return ctx.stmpc_ref(np.array([[state.x, state.y, state.v, state.yaw]], dtype=np.float64), c.T, c.DT, c.dl)[0]
