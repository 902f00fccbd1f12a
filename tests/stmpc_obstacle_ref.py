"""Expected results of the dynamic MPC's moving-obstacle test (f1p_stmpc_set_obstacles), composed from what exists:
tests/stmpc_collision_ref.py's skeleton (the generator, every rollout's fp64 cost, the applied controls, orc.predict_motion_dynamic, the
tested points, the visit order) with tests/kmpc_obstacle_ref.py's disc rule, point times and scenes -- the latter called on the egos'
(x, y, v, yaw) with the branch's own (T, dt).  The "fragile" rule is theirs; the cell rule joins when a grid is given.  The kinematic half
of a batch is kmpc_obstacle_ref.expected on STMPC's kinematic reference.  Shared by tests/test_stmpc_obstacles_host.py (CPU) and
tests/test_gpu_stmpc_obstacles.py."""
import numpy as np

import kmpc_obstacle_ref as KO
import stmpc_collision_ref as S
from kmpc_obstacle_ref import EMPTY, MAX_OBS, disc_blocked, point_times  # noqa: F401
from stmpc_collision_ref import EDGE_EPS, SIG, TIE_EPS, _edge_dist, all_costs, applied, oracle_kref, oracle_ref, tested_points, warm_start  # noqa: F401
from f1tenth_planning_amd import _abi

DT, DTK = 0.025, 0.1


def xy4(x0):
    """[E, 7] -> (x, y, v, yaw) rows, what the scenes of kmpc_obstacle_ref are built around"""
    return np.ascontiguousarray(np.asarray(x0)[:, [0, 1, 3, 4]])


def traffic(x0, T, dt=DT, M=4, seed=0):
    return KO.traffic(xy4(x0), T, dt, M=M, seed=seed)


def crowd16(x0, T, dt=DT, seed=0):
    return KO.crowd16(xy4(x0), T, dt, seed=seed)


def expected(orc, x0, ref, cfg, obs, n_sub, seed, call, warm=None, grid=None, ego_ids=None, n_batch=None, nthreads=8):
    """x0 [E, 7], ref [E, 7, T+1], obs [E, M, 5] (row e: ego e of x0); grid = None or (img u8, res, ox, oy, occupied_below): both rules.
    ego_ids / n_batch: as stmpc_collision_ref.expected.  -> its dict"""
    x0 = np.ascontiguousarray(x0, np.float64); E = x0.shape[0]; T, R = cfg.horizon, cfg.n_rollouts
    obs = np.ascontiguousarray(obs, np.float64)
    assert obs.shape[0] == E and obs.shape[2] == 5 and 1 <= obs.shape[1] <= MAX_OBS
    ids = np.arange(E) if ego_ids is None else np.asarray(ego_ids)
    nb = E if n_batch is None else n_batch
    g = keep = None
    if grid is not None:
        img, res, ox, oy, occ = grid
        g, keep = orc.make_grid(img, res, ox, oy, occ)
    kc = _abi.kmpc_cfg(horizon=T, n_rollouts=R)                          # (the generator reads T and R only)
    ctrl = orc.kmpc_gen_controls(seed, call, nb, kc, SIG["sigma_steer_v"], SIG["sigma_accel"], warm)[ids]
    cost = all_costs(orc, x0, ref, ctrl, cfg, nthreads)
    assert not np.isnan(cost).any()
    tau = point_times(T, n_sub, cfg.dt)
    out = dict(steer=np.zeros(E), speed=np.zeros(E), best_idx=np.full(E, -1, np.int32), best_cost=np.full(E, np.inf),
               best_seq=np.zeros((E, T, 2)), warm=np.zeros((E, T, 2), np.float32), fragile=np.zeros(E, bool),
               all_blocked=np.zeros(E, bool), free_idx=np.argmin(cost, axis=1).astype(np.int32), n_tested=np.zeros(E, np.int32))
    for e in range(E):
        dv, a = applied(ctrl[e], cfg)
        order = np.argsort(cost[e], kind="stable")                      # first minimum by rollout index among equal costs
        win, near_edge = -1, False

        def blocked(r):
            pts = tested_points(orc.predict_motion_dynamic(x0[e], a[r], dv[r], cfg), n_sub)
            hit, near, firm = disc_blocked(pts, tau, obs[e])
            if g is not None:
                cell = False
                for x, y in pts:
                    cell = orc.cell_occupied(g, float(x), float(y)) or cell
                edge = _edge_dist(pts, res, ox, oy) < EDGE_EPS
                hit, near, firm = hit or cell, near or edge, firm or (cell and not edge)
            return hit, near and not firm                               # a rollout's verdict is unsure only where nothing blocks it firmly

        for n, r in enumerate(order):
            hit, edge = blocked(r)
            near_edge = near_edge or edge
            out["n_tested"][e] = n + 1
            if not hit:
                win = int(r)
                break
        out["fragile"][e] = near_edge
        if win < 0:
            out["all_blocked"][e] = True
            continue
        for r in order[out["n_tested"][e]:]:                                # the next ELIGIBLE cost: a tie with the winner's?
            if abs(cost[e, r] - cost[e, win]) > TIE_EPS * abs(cost[e, win]):
                break
            hit, edge = blocked(r)
            if not hit or edge:
                out["fragile"][e] = True
                break
        out["best_idx"][e] = win; out["best_cost"][e] = cost[e, win]
        out["steer"][e] = x0[e, 2] + dv[win, 0] * cfg.dt; out["speed"][e] = x0[e, 3] + a[win, 0] * cfg.dt
        seq = np.stack([dv[win], a[win]], 1)
        out["best_seq"][e] = seq
        w = seq.astype(np.float32)
        out["warm"][e, :-1] = w[1:]; out["warm"][e, -1] = w[-1]
    del keep
    return out


def expected_batch(orc, x0, wp, dcfg, kcfg, obs, n_sub, n_sub_k, seed, call, warm=None, grid=None, v_ks=2.0):
    """f1p_stmpc_plan_batch with obs [E, M, 5] in the batch's ego order: the dynamic egos (v > v_ks) by `expected`, the kinematic ones by
    kmpc_obstacle_ref.expected on STMPC's kinematic reference, each with the batch's ego words.  warm [E, max(T, TK), 2] or None.
    -> (branch [E], dict of the dynamic egos, dict of the kinematic ones -- each with its `ids`)"""
    E = x0.shape[0]; T, TK = dcfg.horizon, kcfg.horizon
    dyn = ~(x0[:, 3] <= v_ks)
    di, ki = np.nonzero(dyn)[0], np.nonzero(~dyn)[0]
    wd = None if warm is None else np.ascontiguousarray(warm[:, :T])
    wk = None if warm is None else np.ascontiguousarray(warm[:, :TK])
    d = expected(orc, x0[di], oracle_ref(orc, x0[di], wp, T, dcfg.dt), dcfg, obs[di], n_sub, seed, call, warm=wd, grid=grid, ego_ids=di, n_batch=E)
    k = KO.expected(orc, xy4(x0), oracle_kref(orc, x0, wp, TK, kcfg.dt), kcfg, obs, n_sub_k, seed, call, SIG["sigma_accel"], SIG["sigma_steer"],
                    warm=wk, grid=grid)
    k = {key: v[ki] for key, v in k.items()}
    d["ids"], k["ids"] = di, ki
    return dyn.astype(np.int32), d, k


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def scene_traffic(E, T, M=4, seed=0, grid="b"):
    """scene B's egos (scene D's, on an all-free image; grid "d": on scene D's map) with traffic() built for the dynamic branch's (T, DT);
    M 16: crowd16 -> dict(wp, x0 [E, 7], grid, obs [E, M, 5])"""
    s = (S.scene_b if grid == "b" else S.scene_d)(E, seed)
    s["obs"] = crowd16(s["x0"], T, seed=seed) if M == 16 else traffic(s["x0"], T, M=M, seed=seed)
    return s


def scene_mixed(E=48, seed=2, T=40, TK=8):
    """the mixed batch: scene D's egos at mixed speeds on its map, traffic(seed) per ego built with the ego's own branch's horizon and time
    step -- (T, DT) for the dynamic rows, (TK, DTK) for the kinematic ones.  (Seed 2: seeds 0 and 3 have one fragile kinematic ego of 21.)"""
    s = S.scene_d(E, seed=seed, mixed_speeds=True)
    dyn = ~(s["x0"][:, 3] <= 2.0)
    s["obs"] = np.ascontiguousarray(np.where(dyn[:, None, None], traffic(s["x0"], T, DT, seed=seed), traffic(s["x0"], TK, DTK, seed=seed)))
    return s


# ---- the disc rule's hand cases (the numpy restatement on the CPU, the kernels on the device) ------------------------------------------------
HAND_DT = 2.0 ** -5


def hand_cases():
    """[(name, x0 [7], T, n_sub, obs [M, 5], blocked)]: a vehicle at the origin heading along +x at v = 4, every other state 0, zero
    controls, DT = 2^-5: p_t = (0.125 t, 0) exactly (orc.predict_motion_dynamic; tests/test_stmpc_obstacles_host.py checks it); the last
    ones with a non-finite state instead -- or with v = 0, where the model's own yr / v makes the NaN"""
    x0 = (0.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0)
    nan = float("nan")
    far = [(500.0, 500.0, 0.0, 0.0, 0.1)]

    def st(**kw):
        s = dict(x=0.0, y=0.0, delta=0.0, v=4.0, yaw=0.0, yr=0.0, beta=0.0); s.update(kw)
        return tuple(s[k] for k in ("x", "y", "delta", "v", "yaw", "yr", "beta"))

    return [
        ("touching: d2 == r r from exactly representable numbers", x0, 1, 1, [(0.625, 0.0, 0.0, 0.0, 0.5)], True),
        ("one ulp less of radius", x0, 1, 1, [(0.625, 0.0, 0.0, 0.0, float(np.nextafter(0.5, 0.0)))], False),
        ("on the line at t = 0, gone before the vehicle arrives", x0, 4, 1, [(0.375, 0.0, 0.0, 100.0, 0.1)], False),
        ("the same disc parked", x0, 4, 1, [(0.375, 0.0, 0.0, 0.0, 0.1)], True),
        ("a small fast disc met at a sub-step time only, n_sub 4", x0, 1, 4, [(0.0625, -0.5, 0.0, 32.0, 0.01)], True),
        ("... which n_sub 1 does not see", x0, 1, 1, [(0.0625, -0.5, 0.0, 32.0, 0.01)], False),
        ("r = -1: empty", x0, 2, 2, [(0.125, 0.0, 0.0, 0.0, -1.0)], False),
        ("r = NaN: empty", x0, 2, 2, [(0.125, 0.0, 0.0, 0.0, nan)], False),
        ("an empty slot between live ones", x0, 2, 1, [(5.0, 5.0, 0.0, 0.0, 0.1), (0.0, 0.0, 0.0, 0.0, -1.0), (0.25, 0.0, 0.0, 0.0, 0.1)], True),
        ("a NaN centre in a live slot blocks everything", x0, 1, 1, [(nan, 0.0, 0.0, 0.0, 0.1)], True),
        ("a NaN velocity in a live slot blocks everything", x0, 1, 1, [(50.0, 50.0, 0.0, nan, 0.1)], True),
        ("r = 0: a point obstacle met exactly", x0, 1, 1, [(0.125, 0.0, 0.0, 0.0, 0.0)], True),
        ("a NaN ego speed is blocked by a live slot however far", st(v=nan), 2, 1, far, True),
        ("a NaN ego heading likewise", st(yaw=nan), 2, 2, far, True),
        ("a NaN ego position likewise", st(x=nan), 1, 1, [(0.0, 0.0, 0.0, 0.0, -1.0)] + far, True),
        ("a NaN slip angle likewise", st(beta=nan), 1, 1, far, True),
        ("a NaN yaw rate reaches the position at the second step", st(yr=nan), 3, 1, far, True),
        ("... not at the first", st(yr=nan), 1, 1, far, False),
        ("a NaN steering angle likewise", st(delta=nan), 3, 2, far, True),
        ("v = 0: the model's own 0 / 0 makes NaN positions, blocked by a live slot however far", st(v=0.0), 3, 1, far, True),
        ("... and by no empty one", st(v=nan), 2, 1, [(0.0, 0.0, 0.0, 0.0, -1.0)], False),
    ]
