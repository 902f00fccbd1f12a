"""Expected results of the shooting MPC's moving-obstacle test (f1p_kmpc_set_obstacles), composed as tests/kmpc_collision_ref.py
composes the occupancy test's: the oracle's generator, every rollout's fp64 cost, the rollout itself (predict_motion_kinematic), rollouts
visited in ascending (cost, index) order until the first unblocked one.  The disc rule is restated here in numpy, literally and in the order
of include/f1p.h; the cell rule (orc.cell_occupied) joins it when a grid is given.  Shared by tests/test_kmpc_obstacles_host.py (the scene
meets its conditions, the rule's hand cases; CPU) and tests/test_gpu_kmpc_obstacles.py.

An ego is "fragile" -- not compared -- when the verdict on a rollout no costlier than the winner could fall either way: a tested point
within DISC_EPS of a disc's rim (or EDGE_EPS of a cell edge) and no point of that rollout blocked by more than that; or when the next
eligible cost is within TIE_EPS of the winner's.  (The parked disc of slot 3 has a sub-step point exactly on its rim at even n_sub and its
centre on p_1: blocked firmly, so not fragile.)"""
import numpy as np

from kmpc_collision_ref import EDGE_EPS, TIE_EPS, _edge_dist, applied, oracle_ref, scene_a, scene_b, tested_points, warm_start  # noqa: F401

DISC_EPS = 1e-9          # [m] a tested point this close to a disc's rim may fall either way (device sincos vs glibc, last ulp)
MAX_OBS = 16


def point_times(T, n_sub, dt):
    """tau of tested_points' rows: ((double)t + (double)j / (double)n_sub) * dt, j = 1 .. n_sub within t = 0 .. T-1"""
    return np.array([(float(t) + float(j) / float(n_sub)) * dt for t in range(T) for j in range(1, n_sub + 1)])


def live_slots(obs_e):
    """rows with r >= 0 (a negative or NaN radius: an empty slot)"""
    return obs_e[obs_e[:, 4] >= 0.0]


def disc_blocked(pts, tau, obs_e):
    """pts [N, 2], tau [N], obs_e [M, 5] -> (blocked, a point within DISC_EPS of a rim, a point inside a disc by more than that or
    non-finite: blocked whatever the last ulp does).  The rule, per point and live slot:
    cx = x + vx * tau; cy = y + vy * tau; dx = Px - cx; dy = Py - cy; d2 = dx*dx + dy*dy; blocked when not (d2 > r*r)"""
    hit, near, firm = False, False, False
    with np.errstate(invalid="ignore", over="ignore"):
        for x, y, vx, vy, r in live_slots(obs_e):
            cx = x + vx * tau; cy = y + vy * tau
            dx = pts[:, 0] - cx; dy = pts[:, 1] - cy
            d2 = dx * dx + dy * dy
            hit = hit or bool((~(d2 > r * r)).any())
            near = near or bool((np.abs(np.sqrt(d2) - r) < DISC_EPS).any())
            firm = firm or bool((~(np.sqrt(d2) > r - DISC_EPS)).any())
    return hit, near, firm


def expected(orc, x0, ref, cfg, obs, n_sub, seed, call, sigma_a=1.5, sigma_d=0.15, warm=None, grid=None, nthreads=8):
    """obs [E, M, 5]; grid = None or (img u8, res, ox, oy, occupied_below): both rules.  -> kmpc_collision_ref.expected's dict"""
    x0 = np.ascontiguousarray(x0, np.float64); E = x0.shape[0]; T, R = cfg.horizon, cfg.n_rollouts
    obs = np.ascontiguousarray(obs, np.float64)
    assert obs.shape[0] == E and obs.shape[2] == 5 and 1 <= obs.shape[1] <= MAX_OBS
    g = keep = None
    if grid is not None:
        img, res, ox, oy, occ = grid
        g, keep = orc.make_grid(img, res, ox, oy, occ)
    ctrl = orc.kmpc_gen_controls(seed, call, E, cfg, sigma_a, sigma_d, warm)
    sh = orc.kmpc_shoot_batch(x0, ref, ctrl, cfg, want_all=True, nthreads=nthreads)
    cost = sh["all_cost"]
    assert not np.isnan(cost).any()
    tau = point_times(T, n_sub, cfg.dt)
    out = dict(steer=np.zeros(E), speed=np.zeros(E), best_idx=np.full(E, -1, np.int32), best_cost=np.full(E, np.inf),
               best_seq=np.zeros((E, T, 2)), warm=np.zeros((E, T, 2), np.float32), fragile=np.zeros(E, bool),
               all_blocked=np.zeros(E, bool), free_idx=sh["best_idx"].copy(), n_tested=np.zeros(E, np.int32))
    for e in range(E):
        a, d = applied(ctrl[e], cfg)
        order = np.argsort(cost[e], kind="stable")                      # first minimum by rollout index among equal costs
        win, near_edge = -1, False

        def blocked(r):
            pts = tested_points(orc.predict_motion_kinematic(x0[e], a[r], d[r], cfg), n_sub)
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
        out["steer"][e] = d[win, 0]; out["speed"][e] = x0[e, 2] + a[win, 0] * cfg.dt
        seq = np.stack([a[win], d[win]], 1)
        out["best_seq"][e] = seq
        w = seq.astype(np.float32)
        out["warm"][e, :-1] = w[1:]; out["warm"][e, -1] = w[-1]
    del keep
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
EMPTY = (0.0, 0.0, 0.0, 0.0, -1.0)


def traffic(x0, T, dt=0.1, M=4, seed=0):
    """the obstacles of scene "traffic" for the egos x0 [E, 4] = (x, y, v, yaw) -> obs [E, M, 5], M >= 4 (slots past 3 are empty, every
    third of them with a NaN radius).
    slot 0: a slower car ahead of every ego -- 0.7 m to 0.5 + 0.6 v T dt ahead, lateral N(0, 0.15), 0 .. 0.8 x the ego's speed along its
            heading, r 0.30;
    slot 1: empty;
    slot 2: every other ego: a disc of r 0.25 that starts 1.5 m to one side and crosses the ego's line within the horizon, where the ego
            would be at that time;
    slot 3: egos 3::8: a parked disc centred on the ego's first station p_0 + v dt (cos, sin), which no control moves, r = min(0.2, 0.5 v dt):
            every rollout is blocked;
    egos 4::5: every slot empty."""
    E = x0.shape[0]
    rng = np.random.default_rng(seed + 2)
    obs = np.empty((E, M, 5)); obs[:] = EMPTY
    obs[:, 5::3, 4] = np.nan
    x, y, v, yaw = x0.T
    c, s = np.cos(yaw), np.sin(yaw)
    ahead = rng.uniform(0.7, 0.5 + 0.6 * v * T * dt); lat = rng.normal(0, 0.15, E); sp = rng.uniform(0.0, 0.8, E) * v
    obs[:, 0] = np.column_stack([x + ahead * c - lat * s, y + ahead * s + lat * c, sp * c, sp * s, np.full(E, 0.30)])
    tc = rng.uniform(0.3, 0.9, E) * T * dt; side = np.where(rng.random(E) < 0.5, -1.0, 1.0)
    cross = np.column_stack([x + v * tc * c - 1.5 * side * s, y + v * tc * s + 1.5 * side * c, 1.5 * side * s / tc, -1.5 * side * c / tc,
                             np.full(E, 0.25)])
    obs[0::2, 2] = cross[0::2]
    r3 = np.minimum(0.2, 0.5 * v * dt)
    park = np.column_stack([x + v * dt * c, y + v * dt * s, np.zeros(E), np.zeros(E), r3])
    obs[3::8, 3] = park[3::8]
    obs[4::5] = EMPTY
    return np.ascontiguousarray(obs)


def crowd16(x0, T, dt=0.1, seed=0):
    """16 LIVE discs for every ego: traffic(M = 16) with each of its empty slots (those of egos 4::5 included) taken by a bystander -- a disc
    of r 0.15 placed 0 .. v T dt ahead of the ego and 0.6 .. 2.5 m to either side, drifting at up to 0.5 m/s: within the horizon's reach, so
    no slot is dropped before the tests, and mostly beside the road the ego takes.  -> obs [E, 16, 5]"""
    E = x0.shape[0]
    obs = traffic(x0, T, dt, M=16, seed=seed)
    rng = np.random.default_rng(seed + 3)
    x, y, v, yaw = (q[:, None] for q in x0.T)
    c, s = np.cos(yaw), np.sin(yaw)
    ahead = rng.uniform(0.0, 1.0, (E, 16)) * v * T * dt
    lat = rng.uniform(0.6, 2.5, (E, 16)) * np.where(rng.random((E, 16)) < 0.5, -1.0, 1.0)
    by = np.stack([x + ahead * c - lat * s, y + ahead * s + lat * c, rng.uniform(-0.5, 0.5, (E, 16)), rng.uniform(-0.5, 0.5, (E, 16)),
                   np.full((E, 16), 0.15)], 2)
    empty = ~(obs[:, :, 4] >= 0.0)
    obs[empty] = by[empty]
    return np.ascontiguousarray(obs)


def scene_traffic(E, T, M=4, seed=0):
    """scene_b's course and egos in open space with traffic() -> dict(wp, x0, grid (no occupied cell), obs [E, M, 5])"""
    s = scene_b(E, T, seed)
    s["obs"] = traffic(s["x0"], T, M=M, seed=seed)
    return s


# ---- the disc rule's hand cases (the numpy restatement on the CPU, the kernels on the device) ------------------------------------------------
def hand_cases():
    """[(name, x0 (x, y, v, yaw), T, n_sub, obs [M, 5], blocked)]: a vehicle at the origin heading along +x at 2.5 m/s with zero controls,
    dt 0.1: p_t = (0.25 t, 0) exactly; the last four with a non-finite state instead"""
    x0 = (0.0, 0.0, 2.5, 0.0)
    nan = float("nan")
    return [
        ("touching: d2 == r r from exactly representable numbers", x0, 1, 1, [(0.75, 0.0, 0.0, 0.0, 0.5)], True),
        ("one ulp less of radius", x0, 1, 1, [(0.75, 0.0, 0.0, 0.0, float(np.nextafter(0.5, 0.0)))], False),
        ("on the line at t = 0, gone before the vehicle arrives", x0, 4, 1, [(0.75, 0.0, 0.0, 10.0, 0.2)], False),
        ("the same disc parked", x0, 4, 1, [(0.75, 0.0, 0.0, 0.0, 0.2)], True),
        ("a small fast disc met at a sub-step time only, n_sub 4", x0, 1, 4, [(0.125, -0.5, 0.0, 10.0, 0.01)], True),
        ("... which n_sub 1 does not see", x0, 1, 1, [(0.125, -0.5, 0.0, 10.0, 0.01)], False),
        ("r = -1: empty", x0, 2, 2, [(0.25, 0.0, 0.0, 0.0, -1.0)], False),
        ("r = NaN: empty", x0, 2, 2, [(0.25, 0.0, 0.0, 0.0, nan)], False),
        ("an empty slot between live ones", x0, 2, 1, [(5.0, 5.0, 0.0, 0.0, 0.1), (0.0, 0.0, 0.0, 0.0, -1.0), (0.5, 0.0, 0.0, 0.0, 0.1)], True),
        ("a NaN centre in a live slot blocks everything", x0, 1, 1, [(nan, 0.0, 0.0, 0.0, 0.1)], True),
        ("a NaN velocity in a live slot blocks everything", x0, 1, 1, [(50.0, 50.0, 0.0, nan, 0.1)], True),
        ("r = 0: a point obstacle met exactly", x0, 1, 1, [(0.25, 0.0, 0.0, 0.0, 0.0)], True),
        ("a NaN ego speed is blocked by a live slot however far", (0.0, 0.0, nan, 0.0), 2, 1, [(500.0, 500.0, 0.0, 0.0, 0.1)], True),
        ("a NaN ego heading likewise", (0.0, 0.0, 2.5, nan), 2, 2, [(500.0, 500.0, 0.0, 0.0, 0.1)], True),
        ("a NaN ego position likewise", (nan, 0.0, 2.5, 0.0), 1, 1, [(0.0, 0.0, 0.0, 0.0, -1.0), (500.0, 500.0, 0.0, 0.0, 0.1)], True),
        ("... and by no empty one", (0.0, 0.0, nan, 0.0), 2, 1, [(0.0, 0.0, 0.0, 0.0, -1.0)], False),
    ]
