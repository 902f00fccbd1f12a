"""Grazing scenes for the FREE verdict of the kinematic shooting solver's f32 filter (csrc/k_kmpc.hip, the `n_eff == 1 && !best_cost`
branch: a single survivor is emitted on the filter's word, no fp64 test follows).  Shared by tests/test_shoot_graze_host.py
(the scenes meet their conditions; CPU) and tests/test_gpu_shoot_graze.py.

A batch = a configuration of one of the filter's three instantiations, a horizon and n_sub:
    egos, course and reference: kmpc_collision_ref.scene_b (open space), the speeds mapped from 1 .. 5 to 2.5 .. 5 m/s (see "geometry");
    warm start: the winner of four oracle plans with shrinking sigmas, each around the last; the tested call then samples with SIGMA =
        (3.0, 0.3) around it, so that rollout 0 -- the warm start -- has the lowest long-double cost by at least 10x the filter's margin
        |fmin| min(3.4e-6 T, 0.5) + 0.02: the filter keeps ONE survivor (n_refined == 1);
    the designated point (t*, j*) of rollout 0's long-double rollout (shoot_ref.kin_rollout on the applied sequence), t* cycled over the
        second half of the horizon, j* over 1 .. n_sub;
    one disc per ego whose centre, at the point's own time, lies at r - delta (INSIDE: rollout 0 is blocked) or r + delta (OUTSIDE: it is
        free) from the point; the velocity cycled over 0, +-1.5 m/s along the path, +-1.5 m/s across it;
    delta: eight rungs, geometric from max(1e-8 m, 64 x the point's |float64 - long double| deviation) to twice the filter's allowance
        (allowance(): obs_compact's F1P_K4_POS_ERR_REL x reach + 1e-6 S restated); ego e has rung (e % 16) // 2 and sign e % 2;
    the direction from point to centre: the first of 16 for which no other tested point of rollout 0, and no tested point of any rollout
        at or below the expected winner's long-double cost, lies within 10 allowances of the rim.
The expected winner is the first long-double minimum over the rollouts unblocked under the rule of include/f1p.h (blocked when
!(|P - c(tau)|^2 > r r) at any tested point), evaluated on the fp64 disc rows the device gets.  An ego is DECISIVE when all of the above
succeeded and the expected winner's cost lies more than the cost tolerance of tests/test_gpu_shoot_offdefault.py (16 max(|fp64 - long
double| cost deviation, 4 eps |cost|)) below the next unblocked rollout's.

Geometry.  A neighbour of the designated point on a locally straight path is s = v dt / n_sub away; with the centre abeam it clears the
rim by s^2 / 2r.  10 allowances = 18 mm at T = 30 (4.8 mm at T = 8), so T = 30 goes with n_sub = 4 and the radii 0.05 / 0.15 / 0.3 m,
T = 8 with n_sub = 16 and the radii 0.005 / 0.01 / 0.02 m (at 0.05 m and above no direction clears the neighbours at n_sub = 16), and
the egos run at 2.5 m/s and above.  Where none of the 16 directions will do at the ego's radius the smaller radii of its set are tried; an
ego for which none does is not decisive, and the host test holds the share."""
import numpy as np

import kmpc_collision_ref as KC
import shoot_ref as S
from f1tenth_planning_amd import _abi

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
E, R = 48, 256
SEED, CALL = 23, 5
SIGMA = (3.0, 0.3)
MARGIN_REL, MARGIN_ABS = 3.4e-6, 0.02                                  # F1P_K4_MARGIN_REL / _ABS
POS_ERR_REL, OBS_ERR_REL = 1.0e-4, 1.0e-6                              # F1P_K4_POS_ERR_REL / F1P_K4_OBS_ERR_REL (shoot_col.h)
N_RUNGS, N_DIR, K_LOW = 8, 16, 24
VELS = ((0.0, 0.0), (1.5, 0.0), (0.0, 1.5), (-1.5, 0.0), (0.0, -1.5))  # (along, across) the path at the designated point [m/s]
RADII = {4: (0.05, 0.15, 0.3), 16: (0.005, 0.01, 0.02)}               # by n_sub

CONFIGS = {                                                            # name -> (kmpc_cfg keywords, the filter's instantiation)
    "iso": (dict(), "<POLY, ISO>"),
    "qxy": (dict(q=(13.5, 27.0, 5.5, 13.0), qf=(13.5, 27.0, 5.5, 13.0)), "<POLY, !ISO>"),
    "tanf": (dict(max_steer=0.9), "<!POLY, !ISO>"),
}
BATCHES = [(c, T, n_sub) for c in CONFIGS for T, n_sub in ((30, 4), (8, 16))]
STMPC_BATCHES = [("iso", 8, 16), ("qxy", 30, 4)]                       # through f1p_stmpc_plan_batch's kinematic branch (build(stmpc=True))
STMPC_V_KS = 10.0                                                      # every ego at or below it: the kinematic model


def make_cfg(name, T):
    return _abi.kmpc_cfg(horizon=T, n_rollouts=R, **CONFIGS[name][0])


def is_iso(cfg):
    """k_kmpc_plan_gen_t: poly && q[0] == q[1] && qf[0] == qf[1] (the weights' f32 square roots compare as the weights do)"""
    return cfg.max_steer <= 0.45 and cfg.q[0] == cfg.q[1] and cfg.qf[0] == cfg.qf[1]


def margin(fmin, T):
    return abs(float(fmin)) * min(MARGIN_REL * T, 0.5) + MARGIN_ABS


def applied(ctrl_e, cfg, dtype=LD):
    """kmpc_collision_ref.applied in `dtype`: controls f32 [T, 2, R] -> (a, d) [R, T]"""
    a = S.clamp(ctrl_e[:, 0, :].astype(dtype), -dtype(cfg.max_accel), dtype(cfg.max_accel))
    d = S.clamp(ctrl_e[:, 1, :].astype(dtype), -dtype(cfg.max_steer), dtype(cfg.max_steer))
    dmax = dtype(cfg.max_dsteer) * dtype(cfg.dt)
    for t in range(1, d.shape[0]):
        d[t] = S.clamp(d[t], d[t - 1] - dmax, d[t - 1] + dmax)
    return np.ascontiguousarray(a.T), np.ascontiguousarray(d.T)


def points(paths, n_sub):
    """paths [K, 4, T+1] -> the tested points [K, T, n_sub, 2]: p_t + (p_{t+1} - p_t) * ((double)j / (double)n_sub), j == n_sub: p_{t+1} itself"""
    p, q = paths[:, :2, :-1], paths[:, :2, 1:]
    cols = [q if j == n_sub else p + (q - p) * paths.dtype.type(float(j) / float(n_sub)) for j in range(1, n_sub + 1)]
    return np.stack(cols, 3).transpose(0, 2, 3, 1)


def times(T, n_sub, dt, dtype=LD):
    """tau [T, n_sub] = ((double)t + (double)j / (double)n_sub) * dt"""
    return np.array([[dtype(float(t) + float(j) / float(n_sub)) * dtype(dt) for j in range(1, n_sub + 1)] for t in range(T)], dtype)


def rim_distance(pts, tau, disc):
    """pts [K, T, n_sub, 2], disc (x, y, vx, vy, r) fp64 -> (|P - c(tau)| - r [K, T, n_sub], blocked [K, T, n_sub]: !(d2 > r r), the rule)"""
    t = pts.dtype.type
    x, y, vx, vy, r = (t(v) for v in disc)
    dx = pts[..., 0] - (x + vx * tau); dy = pts[..., 1] - (y + vy * tau)
    d2 = dx * dx + dy * dy
    return np.sqrt(d2) - r, ~(d2 > r * r)


def allowance(x0_e, disc, cfg):
    """obs_compact's eps for one live slot: POS_ERR_REL x reach + OBS_ERR_REL x S, S = |o_rel|_1 + |v|_1 T dt + r + reach in the filter's
    frame (ISO: rotated by -yaw0), reach = max(|v0|, |max_speed|, |min_speed|) T dt"""
    sx, sy, sv, syaw = (float(v) for v in x0_e)
    x, y, vx, vy, r = (float(v) for v in disc)
    Tdt = cfg.horizon * cfg.dt
    reach = max(abs(sv), abs(cfg.max_speed), abs(cfg.min_speed)) * Tdt
    dx, dy = x - sx, y - sy
    if is_iso(cfg):
        c0, s0 = np.cos(syaw), np.sin(syaw)
        dx, dy, vx, vy = c0 * dx + s0 * dy, c0 * dy - s0 * dx, c0 * vx + s0 * vy, c0 * vy - s0 * vx
    return POS_ERR_REL * reach + OBS_ERR_REL * ((abs(dx) + abs(dy)) + (abs(vx) + abs(vy)) * Tdt + r + reach)


def _verdicts(order, cost, pts, tau, disc):
    """rollouts in ascending (cost, index) order: -> (winner or -1, its position in `order`, gap to the next unblocked rollout's cost)"""
    _, blk = rim_distance(pts, tau, disc)
    hit = blk.reshape(len(order), -1).any(1)
    free = np.nonzero(~hit)[0]
    if len(free) == 0:
        return -1, -1, 0.0
    gap = float(cost[order[free[1]]] - cost[order[free[0]]]) if len(free) > 1 else 0.0     # (no second one among the K_LOW: not decisive)
    return int(order[free[0]]), int(free[0]), gap


_cache = {}


def build(orc, name, T, n_sub, stmpc=False):
    """stmpc: the batch for the kinematic branch of f1p_stmpc_plan_batch -- x7 [E, 7] = (x, y, 0, v, yaw, 0, 0) and STMPC's kinematic reference
    (stmpc_collision_ref.oracle_kref), which the device extracts itself; the generator, the model and the rule are the same.
    -> dict(cfg, wp, x0, ref, warm f32 [E, T, 2], ctrl, obs [E, 1, 5], inside [E], rung [E], delta [E], allow [E], tstar, jstar, win [E]
    (the expected winner, long double), win64 [E] (the float64 restatement's), decisive [E], gap0 [E] (runner-up - rollout 0 without
    obstacles, in margins), free_win [E] (the long-double winner without obstacles: 0 on every decisive ego), dev [E] (the designated
    point's |float64 - long double|), grid (the scene's image, no occupied cell), decisive_grid [E])"""
    key = (name, T, n_sub, stmpc)
    if key in _cache:
        return _cache[key]
    cfg = make_cfg(name, T)
    s = KC.scene_b(E, T)
    x0 = s["x0"].copy()
    x0[:, 2] = 2.5 + 0.625 * (x0[:, 2] - 1.0)
    x7 = np.zeros((E, 7)); x7[:, [0, 1, 3, 4]] = x0
    if stmpc:
        import stmpc_collision_ref as SC
        ref = SC.oracle_kref(orc, x7, s["wp"], T, cfg.dt)
    else:
        ref = KC.oracle_ref(orc, x0, s["wp"], T)
    warm = KC.warm_start(E, T)
    for i, k in enumerate((1.0, 0.5, 0.25, 0.125)):                     # a warm start near a local minimum: the winner of a short descent
        warm = orc.kmpc_plan_batch(x0, ref, cfg, 900 + i, i, 1.5 * k, 0.15 * k, warm=warm, nthreads=8)["best_seq"].astype(np.float32)
    ctrl = orc.kmpc_gen_controls(SEED, CALL, E, cfg, SIGMA[0], SIGMA[1], warm)
    ld = S.kin_shoot(x0, ref, ctrl, cfg)
    f64 = S.kin_shoot(x0, ref, ctrl, cfg, np.float64)
    cost, cost64 = ld["costs"], f64["costs"]
    out = dict(cfg=cfg, wp=s["wp"], x0=x0, ref=ref, warm=warm, ctrl=ctrl, obs=np.zeros((E, 1, 5)), inside=np.arange(E) % 2 == 0,
               rung=(np.arange(E) % 16) // 2, delta=np.zeros(E), allow=np.zeros(E), tstar=np.zeros(E, int), jstar=np.zeros(E, int),
               win=np.full(E, -2), win64=np.full(E, -3), decisive=np.zeros(E, bool), gap0=np.zeros(E), dev=np.zeros(E), n_sub=n_sub, free_win=np.zeros(E, int), x7=x7)
    out["obs"][:] = (0.0, 0.0, 0.0, 0.0, -1.0)
    # the scene's image without an occupied cell: with the occupancy test on as well nothing changes for an ego whose compared rollouts stay
    # inside it (decisive_grid), and the filter runs the discs' proof beside the clearance look-ups
    out["grid"] = s["grid"]; out["decisive_grid"] = np.zeros(E, bool)
    gimg, gres, gox, goy, _ = s["grid"]
    tau, tau64 = times(T, n_sub, cfg.dt), times(T, n_sub, cfg.dt, np.float64)
    radii = RADII[n_sub]
    nT = T - T // 2
    for e in range(E):
        order = np.argsort(cost[e], kind="stable")[:K_LOW]
        order64 = np.argsort(cost64[e], kind="stable")[:K_LOW]
        out["gap0"][e] = float(cost[e, order[1]] - cost[e, order[0]]) / margin(cost[e, order[0]], T)
        out["free_win"][e] = order[0]
        dev_c = float(np.abs(cost64[e, order[:8]] - cost[e, order[:8]]).max())
        tol = 16.0 * max(dev_c, 4 * EPS * abs(float(cost[e, order[0]])))
        a, d = applied(ctrl[e], cfg)
        a64, d64 = applied(ctrl[e], cfg, np.float64)
        pts = points(S.kin_rollout(np.repeat(x0[e][None], K_LOW, 0), a[order], d[order], cfg), n_sub)
        pts64 = points(S.kin_rollout(np.repeat(x0[e][None], K_LOW, 0), a64[order64], d64[order64], cfg, np.float64), n_sub)
        rep = e // 16
        ts, js = T // 2 + (7 * e + rep) % nT, (3 * e + rep) % n_sub       # js + 1 = j*: 1 .. n_sub
        va, vc = VELS[(2 * e + rep) % 5]
        out["tstar"][e], out["jstar"][e] = ts, js + 1
        if order[0] != 0 or order64[0] != 0 or out["gap0"][e] < 10.0:
            continue                                                   # the warm start does not win by 10 margins: not this ego
        P = pts[0, ts, js]
        out["dev"][e] = float(np.hypot(*(pts64[0, ts, js].astype(LD) - P)))
        step = pts[0, ts, n_sub - 1] - (pts[0, ts - 1, n_sub - 1])
        h = step / np.sqrt((step * step).sum())                        # the path's direction at the point
        vel = (va * h + vc * np.array([-h[1], h[0]])).astype(np.float64).astype(LD)     # the fp64 row's velocity
        inside = bool(out["inside"][e])
        lo = max(1e-8, 64.0 * out["dev"][e])
        mask0 = np.ones((T, n_sub), bool); mask0[ts, js] = False
        first = (e + rep) % 3                                          # the ego's radius; the smaller ones where no direction does for it
        for r, k in [(radii[i], k) for i in [first] + [i for i in (2, 1, 0) if i < first] for k in range(N_DIR)]:
            ang = LD(2 * np.pi * ((k + e) % N_DIR) / N_DIR + np.pi / N_DIR)
            u = np.array([np.cos(ang) * h[0] - np.sin(ang) * h[1], np.sin(ang) * h[0] + np.cos(ang) * h[1]])
            # the allowance depends (weakly: 1e-6 S) on where the disc stands: one fixed-point step from the disc at delta = 0
            disc = None
            allow = 0.0
            for _ in range(2):
                delta = lo * (2.0 * allow / lo) ** (out["rung"][e] / (N_RUNGS - 1.0)) if allow > 0 else 0.0
                c = P + (LD(r) + (-delta if inside else delta)) * u
                o = c - vel * tau[ts, js]
                disc = np.array([float(o[0]), float(o[1]), float(vel[0]), float(vel[1]), r])
                allow = allowance(x0[e], disc, cfg)
            if 2.0 * allow <= lo:
                break
            sd, _ = rim_distance(pts, tau, disc)
            if abs(float(sd[0, ts, js]) - (-delta if inside else delta)) > 1e-3 * delta:
                continue                                               # the rounding of the disc's row to fp64 moved the rim: not this direction
            win, pos, gap = _verdicts(order, cost[e], pts, tau, disc)
            if win < 0 or (win == 0) == inside:
                continue
            near = np.abs(sd[:pos + 1]).astype(np.float64)
            near[0][~mask0] = np.inf
            if near.min() < 10.0 * allow:
                continue
            out["obs"][e, 0] = disc; out["delta"][e] = delta; out["allow"][e] = allow; out["win"][e] = win
            out["win64"][e] = _verdicts(order64, cost64[e], pts64, tau64, disc)[0]
            out["decisive"][e] = gap > tol
            _, border = grid_blocked(pts[:pos + 1], [], gox, goy, gres, gimg.shape[0])
            out["decisive_grid"][e] = out["decisive"][e] and gimg.shape[0] == gimg.shape[1] and border.min() >= 10.0 * allow
            break
    _cache[key] = out
    return out


# ---- the grid twin: one occupied cell per ego under an interior sub-point of rollout 0 ----------------------------------------------------
GRID_RES, GRID_SIZE, GRID_NSUB = 0.02, 2000, 4                          # the scenes' 40 m x 40 m at 2 cm: v dt / n_sub > 4 cells from 3.2 m/s
GRID_BATCHES = [(c, T) for c in CONFIGS for T in (30, 8)]


def _cells(pts, ox, oy, inv_res):
    t = pts.dtype.type
    return (pts[..., 0] - t(ox)) * t(inv_res), (pts[..., 1] - t(oy)) * t(inv_res)


def grid_blocked(pts, cells, ox, oy, res, size):
    """the cell rule on pts [..., 2] against the occupied `cells` [(gx, gy)] of an otherwise free size x size image: -> (blocked [...],
    distance [m] to the nearest boundary between free and occupied: an occupied cell's edge or the image's border [...])"""
    inv_res = 1.0 / res
    u, v = _cells(pts, ox, oy, inv_res)
    fu, fv = np.floor(u), np.floor(v)
    blocked = ~((fu >= 0) & (fv >= 0) & (fu < size) & (fv < size))
    near = np.minimum(np.minimum(np.abs(u), np.abs(u - size)), np.minimum(np.abs(v), np.abs(v - size)))
    for gx, gy in cells:
        blocked |= (fu == gx) & (fv == gy)
        du = np.maximum(np.maximum(gx - u, u - (gx + 1)), 0); dv = np.maximum(np.maximum(gy - v, v - (gy + 1)), 0)
        out = np.sqrt(du * du + dv * dv)
        ins = np.minimum(np.minimum(u - gx, gx + 1 - u), np.minimum(v - gy, gy + 1 - v))
        near = np.minimum(near, np.where(out > 0, out, np.abs(ins)))
    return blocked, (near * res).astype(np.float64)


def _grid_verdict(order, cost, pts, cells, ox, oy, skip=None):
    """-> (winner, gap to the next unblocked rollout, the smallest boundary distance over the rollouts up to the winner -- `skip` = (t, j):
    rollout 0's designated point left out)"""
    blk, near = grid_blocked(pts, cells, ox, oy, GRID_RES, GRID_SIZE)
    hit = blk.reshape(len(order), -1).any(1)
    free = np.nonzero(~hit)[0]
    if len(free) < 2:
        return -1, 0.0, 0.0
    if skip is not None:
        near[0, skip[0], skip[1]] = np.inf
    return int(order[free[0]]), float(cost[order[free[1]]] - cost[order[free[0]]]), float(near[:free[0] + 1].min())


def build_grid(orc, name, T):
    """build()'s batch on an all-free 2 cm image with one occupied cell per ego: the ego is moved by less than a cell so that rollout 0's
    designated INTERIOR sub-point (1 <= j* < n_sub) lies delta inside the cell (inside egos) or delta outside it (outside egos), across
    one of the cell's four edges and level with its centre.  The sub-step spacing at the point exceeds four cells, so its neighbours lie
    outside the filter's 2-cell clearance zone.  The egos run at 3.8 .. 5.5 m/s for that.  An ego whose placement fails once every cell
    stands (another ego's cell within 10 allowances of a compared rollout) loses its cell and is not decisive.
    -> build()'s dict with grid = (img, res, ox, oy, occupied_below), cells [E, 2], obs / decisive_both: a bystander disc per ego"""
    key = ("grid", name, T)
    if key in _cache:
        return _cache[key]
    n_sub = GRID_NSUB
    cfg = make_cfg(name, T)
    s = KC.scene_b(E, T)
    _, _, ox, oy, occ = s["grid"]
    inv_res = 1.0 / GRID_RES
    x0 = s["x0"].copy()
    x0[:, 2] = 3.8 + 0.425 * (x0[:, 2] - 1.0)
    ref = KC.oracle_ref(orc, x0, s["wp"], T)
    warm = KC.warm_start(E, T)
    for i, k in enumerate((1.0, 0.5, 0.25, 0.125)):
        warm = orc.kmpc_plan_batch(x0, ref, cfg, 900 + i, i, 1.5 * k, 0.15 * k, warm=warm, nthreads=8)["best_seq"].astype(np.float32)
    ctrl = orc.kmpc_gen_controls(SEED, CALL, E, cfg, SIGMA[0], SIGMA[1], warm)
    out = dict(cfg=cfg, wp=s["wp"], x0=x0, ref=ref, warm=warm, ctrl=ctrl, inside=np.arange(E) % 2 == 0, rung=(np.arange(E) % 16) // 2,
               delta=np.zeros(E), allow=np.zeros(E), tstar=np.zeros(E, int), jstar=np.zeros(E, int), win=np.full(E, -2),
               win64=np.full(E, -3), decisive=np.zeros(E, bool), gap0=np.zeros(E), dev=np.zeros(E), n_sub=n_sub,
               cells=np.full((E, 2), -1), spacing=np.zeros(E))
    reach = max(abs(cfg.max_speed), abs(cfg.min_speed)) * T * cfg.dt
    nT = T - T // 2
    built = np.zeros(E, bool)
    cost0 = S.kin_shoot(x0, ref, ctrl, cfg)["costs"]
    kin1 = lambda xe, a_, d_, dt_=LD: points(S.kin_rollout(np.repeat(np.asarray(xe)[None], len(a_), 0), a_, d_, cfg, dt_), n_sub)
    for e in range(E):
        a, d = applied(ctrl[e], cfg)
        rep = e // 16
        js = (3 * e + rep) % (n_sub - 1)                               # j* = js + 1: 1 .. n_sub - 1
        inside = bool(out["inside"][e])
        allow = POS_ERR_REL * max(reach, abs(x0[e, 2]) * T * cfg.dt)
        p0 = kin1(x0[e], a[:1], d[:1])[0]
        p64 = kin1(x0[e], *(v[:1] for v in applied(ctrl[e], cfg, np.float64)), np.float64)[0]
        order0 = np.argsort(cost0[e], kind="stable")[:K_LOW]
        pK = kin1(x0[e], a[order0], d[order0]).astype(np.float64)      # the screening's rollouts: the unmoved ego's, translated with it (fp64 will do: 12 allowances)
        for ts, edge in [(T // 2 + (7 * e + rep + i) % nT, edge) for i in range(nT) for edge in range(4)]:
            sp = float(np.hypot(*(p0[ts, js + 1] - p0[ts, js])))
            if sp <= 4.0 * GRID_RES * 1.05:
                continue
            dev = float(np.hypot(*(p64[ts, js].astype(LD) - p0[ts, js])))
            lo = max(1e-8, 64.0 * dev)
            delta = lo * (2.0 * allow / lo) ** (out["rung"][e] / (N_RUNGS - 1.0))
            axis, side = (edge + e) % 2, ((edge + e) // 2) % 2          # the edge crossed: x or y, the cell's low or high one
            xe = x0[e].copy()
            u, v = _cells(p0[ts, js], ox, oy, inv_res)
            g = [int(np.floor(u)), int(np.floor(v))]
            for _ in range(3):                                         # move the ego so that the point sits where it should (the model is translation-invariant up to rounding)
                P = kin1(xe, a[:1], d[:1])[0][ts, js]
                uv = list(_cells(P, ox, oy, inv_res))
                want = [LD(g[0]) + LD(0.5), LD(g[1]) + LD(0.5)]
                depth = LD(delta if inside else -delta) * LD(inv_res)  # in cells, into the cell
                want[axis] = (LD(g[axis]) + depth) if side == 0 else (LD(g[axis] + 1) - depth)
                xe[0] += float((want[0] - uv[0]) * LD(GRID_RES)); xe[1] += float((want[1] - uv[1]) * LD(GRID_RES))
            pe = kin1(xe, a[:1], d[:1])
            blk, near = grid_blocked(pe, [g], ox, oy, GRID_RES, GRID_SIZE)
            if bool(blk[0, ts, js]) != inside or abs(near[0, ts, js] - delta) > 1e-3 * delta:
                continue
            shift = np.array([xe[0] - x0[e, 0], xe[1] - x0[e, 1]])
            win, _, near = _grid_verdict(order0, cost0[e], pK + shift, [tuple(c) for c in out["cells"][built]] + [g], ox, oy, (ts, js))
            if win < 0 or (win == 0) == inside or near < 12.0 * allow:
                continue
            out["tstar"][e], out["jstar"][e], out["dev"][e], out["delta"][e], out["allow"][e], out["spacing"][e] = ts, js + 1, dev, delta, allow, sp
            out["x0"][e] = xe; out["cells"][e] = g; built[e] = True
            break
    ld = S.kin_shoot(out["x0"], ref, ctrl, cfg)
    f64 = S.kin_shoot(out["x0"], ref, ctrl, cfg, np.float64)
    rolled = {}
    while True:                                                        # the verdicts with every ego's cell in the image; an ego that fails loses its cell
        cells = [tuple(c) for c in out["cells"][built]]
        failed = []
        for e in np.nonzero(built)[0]:
            cost, cost64 = ld["costs"][e], f64["costs"][e]
            order, order64 = np.argsort(cost, kind="stable")[:K_LOW], np.argsort(cost64, kind="stable")[:K_LOW]
            out["gap0"][e] = float(cost[order[1]] - cost[order[0]]) / margin(cost[order[0]], T)
            tol = 16.0 * max(float(np.abs(cost64[order[:8]] - cost[order[:8]]).max()), 4 * EPS * abs(float(cost[order[0]])))
            if e not in rolled:                                        # (a surviving ego keeps its place: its rollouts are computed once)
                a, d = applied(ctrl[e], cfg)
                a64, d64 = applied(ctrl[e], cfg, np.float64)
                rolled[e] = (kin1(out["x0"][e], a[order], d[order]), kin1(out["x0"][e], a64[order64], d64[order64], np.float64))
            win, gap, near = _grid_verdict(order, cost, rolled[e][0], cells, ox, oy, (out["tstar"][e], out["jstar"][e] - 1))
            if order[0] != 0 or order64[0] != 0 or out["gap0"][e] < 10.0 or win < 0 or (win == 0) == bool(out["inside"][e]) or near < 10.0 * out["allow"][e]:
                failed.append(e)
                continue
            out["win"][e] = win
            out["win64"][e] = _grid_verdict(order64, cost64, rolled[e][1], cells, ox, oy)[0]
            out["decisive"][e] = gap > tol
        if not failed:
            break
        built[failed] = False
        out["cells"][failed] = -1; out["x0"][failed] = x0[failed]; out["decisive"][:] = False
    img = np.full((GRID_SIZE, GRID_SIZE), 255, np.uint8)
    for gx, gy in cells:
        img[GRID_SIZE - 1 - gy, gx] = 0                                 # row 0 = top
    og, keep = orc.make_grid(img, GRID_RES, ox, oy, occ)
    for gx, gy in cells:
        assert orc.cell_occupied(og, ox + (gx + 0.5) * GRID_RES, oy + (gy + 0.5) * GRID_RES)
    assert not orc.cell_occupied(og, ox + 0.5 * GRID_RES, oy + 0.5 * GRID_RES)
    out["grid"] = (img, GRID_RES, ox, oy, occ)
    del keep
    # a bystander per ego for the grid + disc run: live, within reach, 1 m (or more) abeam of the designated point and at least 10 of the
    # discs' allowances from every tested point of the rollouts up to the expected winner -- the expected results stay the grid's
    out["obs"] = np.zeros((E, 1, 5)); out["obs"][:] = (0.0, 0.0, 0.0, 0.0, -1.0)
    out["decisive_both"] = np.zeros(E, bool)
    tau = times(T, n_sub, cfg.dt)
    for e in np.nonzero(out["decisive"])[0]:
        pts, order = rolled[e][0], np.argsort(ld["costs"][e], kind="stable")[:K_LOW]
        pos = int(np.nonzero(order == out["win"][e])[0][0])
        ts, js = out["tstar"][e], out["jstar"][e] - 1
        step = (pts[0, ts, js + 1] - pts[0, ts, js]).astype(np.float64)
        nrm = np.array([-step[1], step[0]]) / np.hypot(*step)
        for off in (1.0, -1.0, 1.6, -1.6, 2.4, -2.4):
            c = pts[0, ts, js].astype(np.float64) + off * nrm
            disc = np.array([c[0], c[1], 0.0, 0.0, 0.15])
            sd, _ = rim_distance(pts[:pos + 1], tau, disc)
            if float(sd.min()) >= 10.0 * allowance(out["x0"][e], disc, cfg):
                out["obs"][e, 0] = disc; out["decisive_both"][e] = True
                break
    _cache[key] = out
    return out
