"""f1p_stmpc_qp_avoid_* and STMPCPlanner(SOLVER="qp", QP_AVOID=True): the moving-disc avoidance rows of the dynamic QP against
the exact optima of tests/stmpc_qp_avoid_ref.py -- every family of rows, the half-planes themselves, KKT certificates from the returned
multipliers; an ego without discs against the plain QP; neighbour independence; errors; the plan path's per-branch gather of the discs;
the class in closed loop on the two levine scenes; rivals against the same slots given as obstacles."""
import math

import numpy as np
import pytest

import kmpc_qp_avoid_ref as KA
import stmpc_qp_avoid_ref as A
import stmpc_qp_avoid_scenes as SC
import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._rivals import Rivals
from f1tenth_planning_amd.runtime import (Context, F1PError, kmpc_qp_avoid, rivals, stmpc_qp_avoid, stmpc_qp_set_avoid, stmpc_set_obstacles)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _cfg(T):
    return _abi.stmpc_cfg(horizon=T)


KW = dict(want_x=True, want_duals=True, want_planes=True, want_avoid_duals=True)
OUT_KEYS = ("steer", "speed", "status", "u", "x", "obj", "duals", "iters", "eps", "planes", "avoid_duals")


def _solve(ctx, T, M, sel=slice(None), margin=0.0):
    x0, ref, oa, odv, obs, _ = SC.exact_scene(T, M)
    return stmpc_qp_avoid(ctx, x0[sel], ref[sel], obs[sel], _cfg(T), avoid=_abi.kmpc_qp_avoid(margin=margin), oa_prev=oa[sel], od_v_prev=odv[sel], **KW)


# ---- 1. the exact optimum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M,margin", SC.SHAPES)
def test_exact_optimum_planes_and_certificates(ctx, T, M, margin):
    x0, ref, oa, odv, obs, fam = SC.exact_scene(T, M)
    sols = SC.exact_solutions(T, M, margin)
    SC.assert_families(T, M, margin, obs, sols, fam)
    out = _solve(ctx, T, M, margin=margin)
    worst = dict(u=0.0, n=0.0, rhs=0.0, obj=0.0, primal=0.0, dual=0.0, comp=0.0, stat=0.0)
    print(f"T={T} M={M} margin={margin}: status {out['status'].tolist()} iters max {int(out['iters'].max())}")
    assert np.array_equal(out["status"], SC.expected_status(T, M)), out["status"]
    assert out["iters"].max() <= 50                            # QP_MAX_ITER, the default opts
    skipped = 0
    for e, s in enumerate(sols):
        if s is None:                                          # status 1 / 3: NaN in every output
            for k in OUT_KEYS:
                if k not in ("status", "iters"):
                    assert np.isnan(out[k][e]).all(), (e, k)
            continue
        pl, ref_pl = out["planes"][e], s["planes"]
        assert np.array_equal(pl[:, :, 3], ref_pl[:, :, 3]), (e, pl[:, :, 3], ref_pl[:, :, 3])
        worst["n"] = max(worst["n"], float(np.abs(pl[:, :, :2] - ref_pl[:, :, :2]).max()) / 1e-12)
        worst["rhs"] = max(worst["rhs"], float((np.abs(pl[:, :, 2] - ref_pl[:, :, 2]) / (1.0 + np.abs(ref_pl[:, :, 2]))).max()) / 1e-12)
        assert (np.abs(pl[:, :, :3] - ref_pl[:, :, :3]) <= 1e-12 * (1.0 + np.abs(ref_pl[:, :, :3]))).all(), (e, np.abs(pl - ref_pl).max())
        assert (pl[pl[:, :, 3] < 0][:, :3] == 0.0).all()
        b = s["build"]
        w = np.concatenate([out["u"][e].ravel(), [out["eps"][e]]])
        lam = A.lam_full(b, out["duals"][e], out["avoid_duals"][e])
        cert = A.cert(b, w, lam)
        rel = dict(cert); rel["comp"] /= 1.0 + lam.max()
        for k, bar in (("primal", 1e-9), ("dual", -1e-10), ("comp", 1e-9), ("stat", 1e-8)):
            worst[k] = max(worst[k], (min(rel[k], 0.0) if k == "dual" else rel[k]) / bar)
        assert A.cert_ok(cert, lam), (e, SC.family(e), cert)
        absent = np.setdiff1d(np.arange(2 * T), b["rows"])
        assert (out["avoid_duals"][e][absent] == 0.0).all()
        # obj: the value of the problem's objective at the GPU's point (the plain QP's constant and the slack's cost included)
        obj = 0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"]
        worst["obj"] = max(worst["obj"], abs(out["obj"][e] - obj) / (1.0 + abs(obj)) / 1e-10)
        assert abs(out["obj"][e] - obj) <= 1e-10 * (1.0 + abs(obj)), (e, out["obj"][e], obj)
        # x: the linear model's states at the GPU's u
        z = b["cond"]["Z"] @ out["u"][e].ravel() + b["cond"]["z0"]
        assert np.abs(out["x"][e] - z[:7 * (T + 1)].reshape(T + 1, 7).T).max() <= 1e-9
        if not s["certified"]:
            skipped += 1                                       # the yardstick does not certify itself here: the certificate above decided
            continue
        bar = A.u_bar(b, w, lam, s["w"], s["lam"], s["degenerate"])
        d = float(np.abs(w - s["w"]).max())
        worst["u"] = max(worst["u"], d / bar)
        assert d <= bar, (e, SC.family(e), d, bar)
        assert abs(obj - s["obj"]) <= 1e-10 * (1.0 + abs(s["obj"])), (e, obj - s["obj"])               # the optimal value, tightly
    print("  skipped", skipped, "worst fractions of the bars:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert 16 * skipped <= len(sols), skipped


# ---- 2. no live slot: the plain QP's optimum -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(2, 1), (10, 4), (SC.CAP, 16)])
def test_no_live_slot_agrees_with_the_plain_qp(ctx, T, M):
    x0, ref, oa, odv, obs, fam = SC.exact_scene(T, M)
    sel = fam["no_live"]
    got = _solve(ctx, T, M, sel)
    plain = ctx.stmpc_qp(x0[sel], ref[sel], _cfg(T), oa_prev=oa[sel], od_v_prev=odv[sel], want_duals=True)
    assert (got["status"] == 0).all() and (plain["status"] == 0).all()
    assert np.abs(got["eps"]).max() <= 1e-9 and (got["planes"][:, :, :, 3] == -1).all() and (got["planes"][:, :, :, :3] == 0).all()
    p = SQ.default_params(T)
    for i, e in enumerate(sel):
        c = SQ.condense(SQ.qp_data(x0[e], ref[e], oa[e], odv[e], p), T)
        for o in (got, plain):
            cert = SQ.cond_cert(c, o["u"][i].ravel(), o["duals"][i])
            cert["comp"] /= 1.0 + o["duals"][i].max()
            assert SQ.cert_ok(cert), (e, cert)
        us, lam_s, deg = SQ.exact(c, plain["duals"][i])
        if SQ.exact_ok(c, us, lam_s):
            b = dict(H=c["H"], g=c["g"], G=c["G"], h=c["h"])
            for o in (got, plain):
                assert np.abs(o["u"][i].ravel() - us).max() <= A.u_bar(b, o["u"][i].ravel(), o["duals"][i], us, lam_s, deg), e
        assert abs(got["obj"][i] - plain["obj"][i]) <= 1e-10 * (1.0 + abs(plain["obj"][i]))


# ---- 3. neighbour independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(2, 4), (10, 4), (SC.CAP, 4)])
def test_neighbour_independence(ctx, T, M):
    """an ego alone, among 31 and among 130 others: bit-identical"""
    x0, ref, oa, odv, obs, _ = SC.exact_scene(T, M)
    E = len(x0)
    cfg = _cfg(T)
    rep = np.resize(np.arange(E), 131)
    rep[1:] = np.random.default_rng(5).permutation(rep[1:])    # the ego of every family somewhere else each time
    big = stmpc_qp_avoid(ctx, x0[rep], ref[rep], obs[rep], cfg, oa_prev=oa[rep], od_v_prev=odv[rep], **KW)
    mid = stmpc_qp_avoid(ctx, x0[rep[:32]], ref[rep[:32]], obs[rep[:32]], cfg, oa_prev=oa[rep[:32]], od_v_prev=odv[rep[:32]], **KW)
    for k in OUT_KEYS:
        assert np.array_equal(mid[k], big[k][:32], equal_nan=True), k
    first = {int(e): int(np.flatnonzero(rep == e)[0]) for e in range(min(E, 10))}       # one ego of every family, alone
    for e, i in first.items():
        one = stmpc_qp_avoid(ctx, x0[e:e + 1], ref[e:e + 1], obs[e:e + 1], cfg, oa_prev=oa[e:e + 1], od_v_prev=odv[e:e + 1], **KW)
        for k in OUT_KEYS:
            assert np.array_equal(one[k][0], big[k][i], equal_nan=True), (e, k)
            for i2 in np.flatnonzero(rep == e)[1:]:
                assert np.array_equal(big[k][i2], big[k][i], equal_nan=True), (e, k, i2)


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------------
def _levine_ctx(ctx):
    cx, cy, cyaw, sp = SC.levine()
    ctx.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
    return cx, cy, cyaw, sp


def test_errors(ctx):
    x0, ref, oa, odv, obs, _ = SC.exact_scene(10, 4)
    T1 = SC.CAP + 1
    with pytest.raises(ValueError, match="F1P_STMPC_QP_AVOID_MAX_T"):       # F1P_EINVAL past the cap; the plain QP still takes it
        stmpc_qp_avoid(ctx, x0[:1], np.zeros((1, 7, T1 + 1)), obs[:1], _cfg(T1))
    for M in (0, 17):
        with pytest.raises(ValueError):
            stmpc_qp_avoid(ctx, x0[:2], ref[:2], np.zeros((2, M, 5)), _cfg(10))
    for bad in (dict(rho=0.0), dict(rho=np.nan), dict(lin=-1.0), dict(margin=np.inf)):
        with pytest.raises(ValueError):
            stmpc_qp_avoid(ctx, x0[:2], ref[:2], obs[:2], _cfg(10), avoid=_abi.kmpc_qp_avoid(**bad))
        with pytest.raises(ValueError):
            stmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid(**bad))
    # the plan path: the discs of stmpc_set_obstacles, and its E-mismatch error; off: ignored as before
    _levine_ctx(ctx)
    dcfg, kcfg = _cfg(10), _abi.kmpc_cfg(horizon=8)
    ctx.stmpc_qp_warm_reset()
    stmpc_set_obstacles(ctx, obs[:4])
    try:
        plain = ctx.stmpc_qp_plan(x0[:8], dcfg, kcfg)             # off: E = 8 against obstacles for 4 is no error
        stmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid())
        with pytest.raises(F1PError, match="obstacles were set for 4 egos, this plan has 8"):
            ctx.stmpc_qp_plan(x0[:8], dcfg, kcfg)
        with pytest.raises(ValueError, match="F1P_STMPC_QP_AVOID_MAX_T"):
            ctx.stmpc_qp_plan(x0[:4], _cfg(T1), kcfg)
        with pytest.raises(ValueError, match="kinematic branch"):
            ctx.stmpc_qp_plan(x0[:4], _cfg(SC.CAP), _abi.kmpc_cfg(horizon=32))
        stmpc_set_obstacles(ctx, None)
        ctx.stmpc_qp_warm_reset()
        none = ctx.stmpc_qp_plan(x0[:8], dcfg, kcfg)              # on, nothing held: no avoidance rows
        assert np.array_equal(none["status"], plain["status"])
        ok = plain["status"] == 0
        assert np.abs(none["u"][ok] - plain["u"][ok]).max() <= 2e-7
        stmpc_qp_set_avoid(ctx, None)
        ctx.stmpc_qp_warm_reset()
        again = ctx.stmpc_qp_plan(x0[:8], dcfg, kcfg)
        for k in ("steer", "speed", "status", "u", "obj"):
            assert np.array_equal(again[k], plain[k], equal_nan=True), k
        ctx.stmpc_qp_plan(x0[:4], _cfg(T1), kcfg)                 # off: the plain kernel's own cap (44) holds, not this one
    finally:
        stmpc_set_obstacles(ctx, None)
        stmpc_qp_set_avoid(ctx, None)
        ctx.stmpc_qp_warm_reset()


# ---- 5. the plan path: each branch gets its own egos' discs ------------------------------------------------------------------------------
def _plan_batch_case():
    """12 egos along levine, speeds on both sides of V_KS in no order, and per ego two discs of its own beside its first steps"""
    cx, cy, cyaw, sp = SC.levine()
    rng = np.random.default_rng(11)
    E = 12
    k = 40 + 120 * np.arange(E)
    v = np.array([3.0, 1.0, 2.6, 1.9, 2.0, 4.5, 0.8, 2.2, 1.5, 3.5, 2.01, 1.2])
    x0 = np.column_stack([cx[k], cy[k], rng.normal(0, 0.02, E), v, cyaw[k] + rng.normal(0, 0.03, E), rng.normal(0, 0.05, E), rng.normal(0, 0.01, E)])
    obs = np.zeros((E, 2, 5))
    for e in range(E):
        hd = x0[e, 4]
        ahead = 0.1 + 0.2 * v[e]
        for m, side in enumerate((1.0, -1.0)):
            lat = side * (0.40 + 0.02 * e)                      # a different row of discs for every ego, 0 .. 5 cm inside on one side
            obs[e, m] = [x0[e, 0] + ahead * math.cos(hd) - lat * math.sin(hd), x0[e, 1] + ahead * math.sin(hd) + lat * math.cos(hd), 0.0, 0.0,
                         0.42 if m == 0 else 0.30]
    return x0, obs


def _stateless(ctx, x0, obs, branch, ids, T, TK, av):
    """every ego through the stateless call of its own branch, on its own row of discs, from a zero previous solution"""
    out = dict(steer=np.full(len(x0), np.nan), speed=np.full(len(x0), np.nan), status=np.full(len(x0), -1, np.int32), obj=np.full(len(x0), np.nan),
               eps=np.full(len(x0), np.nan))
    d, k = np.flatnonzero(branch == 1), np.flatnonzero(branch == 0)
    s4 = np.ascontiguousarray(x0[:, [0, 1, 3, 4]])
    ref_of = (lambda sel, T_, dt: ctx.stmpc_ref(s4[sel], T_, dt, 0.03)) if ids is None else \
             (lambda sel, T_, dt: ctx.stmpc_ref_tracks(s4[sel], ids[sel], T_, dt, 0.03))
    if len(d):
        o = stmpc_qp_avoid(ctx, x0[d], ref_of(d, T, 0.025), obs[d], _cfg(T), avoid=av)
        for key in out:
            out[key][d] = o[key]
    if len(k):
        ref4 = np.ascontiguousarray(ref_of(k, TK, 0.1)[:, [0, 1, 3, 4]])
        o = kmpc_qp_avoid(ctx, s4[k], ref4, obs[k], _abi.kmpc_cfg(horizon=TK), avoid=av)
        for key in out:
            out[key][k] = o[key]
    return out


@pytest.mark.parametrize("tracks", [False, True])
def test_plan_path_gathers_each_branchs_discs(ctx, tracks):
    """f1p_stmpc_qp_plan_batch / _plan_tracks_batch with the switch on: the discs are held in the caller's ego order, each branch solves a
    compacted subset -- every ego must equal the stateless call of its own branch on ITS OWN row of discs (a missing gather hands ego k of a
    branch the discs of ego k of the batch)"""
    x0, obs = _plan_batch_case()
    cx, cy, cyaw, sp = _levine_ctx(ctx)
    T, TK = 10, 8
    av = _abi.kmpc_qp_avoid(margin=0.01)
    ids = None
    if tracks:
        wp = np.column_stack([cx, cy, sp, cyaw])
        slow = wp.copy(); slow[:, 2] *= 0.7
        ctx.set_tracks([wp, slow], cols=(0, 1, 2, 3))
        ids = (np.arange(len(x0)) % 2).astype(np.int32)
    ctx.stmpc_qp_warm_reset()
    stmpc_qp_set_avoid(ctx, av)
    stmpc_set_obstacles(ctx, obs)
    try:
        got = ctx.stmpc_qp_plan_tracks(x0, ids, _cfg(T), _abi.kmpc_cfg(horizon=TK)) if tracks else ctx.stmpc_qp_plan(x0, _cfg(T), _abi.kmpc_cfg(horizon=TK))
        assert np.array_equal(got["branch"], (x0[:, 3] > 2.0).astype(np.int32)) and 3 <= got["branch"].sum() <= len(x0) - 3
        want = _stateless(ctx, x0, obs, got["branch"], ids, T, TK, av)
        assert (want["status"] == 0).all(), want["status"]
        for key in ("steer", "speed", "status", "obj"):
            assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
        assert (want["eps"] > 1e-4).sum() >= 4                   # the discs matter: with another ego's row the result differs
        other = _stateless(ctx, x0, obs[::-1].copy(), got["branch"], ids, T, TK, av)
        assert (other["steer"] != want["steer"]).any()
    finally:
        stmpc_set_obstacles(ctx, None)
        stmpc_qp_set_avoid(ctx, None)
        ctx.stmpc_qp_warm_reset()
        if tracks:
            ctx.set_tracks([])


# ---- 6. the class in closed loop ------------------------------------------------------------------------------------------------------
def _closed_loop(kind, steps, avoid, T=10, TK=8):
    """levine from waypoint 0 at 3 m/s (above V_KS), the plant of tests/stmpc_qp_ref.py, a plan at every step of DT.  parked: a disc of radius
    0.35, 0.30 m left of waypoint 120 (the line runs 5 cm inside it); moving: the kinematic tests' disc on waypoint 60, 1.5 m/s along the
    heading there.  The planner drives; every step it is compared with the exact solution of the same step, which carries its own
    previous solution by the reference's rules (stmpc_qp_ref.plan_step)."""
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    cx, cy, cyaw, sp = SC.levine()
    planner = STMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp", QP_AVOID=avoid, T=T, TK=TK))
    p, pk = SQ.default_params(T), SQ.kin_params(TK)
    disc0 = KA.parked_disc(cx, cy, cyaw, off=0.30, r=0.35) if kind == "parked" else KA.moving_disc(cx, cy, cyaw)
    s = np.array([cx[0], cy[0], 0.0, 3.0, cyaw[0], 0.0, 0.0])
    warm = None
    out = dict(dmin=math.inf, eps_max=0.0, active=0, checked=0, worst=0.0, branches=[0, 0], diffs=[])
    with Context(0) as rc:
        rc.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
        for step in range(steps):
            disc = KA.disc_at(disc0, p["DT"] * step)
            if avoid:
                planner.obstacles = disc[None]
            steer, speed = planner.plan(s)
            assert planner.obstacles is None
            out["dmin"] = min(out["dmin"], math.hypot(s[0] - disc[0], s[1] - disc[1]))
            if avoid:
                s4 = s[None, [0, 1, 3, 4]]
                if s[3] <= 2.0:                                  # kinematic branch; reset when len(oa) > TK
                    oa, od = (None, None) if warm is None or len(warm[0]) > TK else warm
                    ref = rc.stmpc_ref(s4, TK, 0.1, 0.03)[0][[0, 1, 3, 4]]
                    sol = KA.solve(s4[0], ref, oa, od, disc[None], pk)
                    ok = KA.cert_ok(sol["cert"])
                    warm = (sol["u"][:, 0].copy(), sol["u"][:, 1].copy())
                    out["branches"][0] += 1
                else:                                            # dynamic branch; reset when len(oa) < T
                    oa, odv = (None, None) if warm is None or len(warm[0]) < T else (warm[0][:T], warm[1][:T])
                    ref = rc.stmpc_ref(s4, T, 0.025, 0.03)[0]
                    sol = A.solve(s, ref, oa, odv, disc[None], p)
                    ok = sol["certified"]
                    warm = (sol["u"][:, 1].copy(), sol["u"][:, 0].copy())
                    out["branches"][1] += 1
                out["eps_max"] = max(out["eps_max"], sol["eps"])
                out["active"] += bool((sol["avoid_lam"][:-1] > 1e-9).any())
                if ok:
                    bar = 1e-5 if sol["degenerate"] else 1e-7
                    out["checked"] += 1
                    out["diffs"].append((step, abs(steer - sol["steer"]), abs(speed - sol["speed"]), bar))
                    out["worst"] = max(out["worst"], max(abs(steer - sol["steer"]), abs(speed - sol["speed"])) / bar)
            s = SQ.plant(s, steer, speed, p)
    return out


@pytest.mark.parametrize("kind", ["parked", "moving"])
def test_class_closed_loop(kind):
    steps = 100
    r = _closed_loop(kind, steps, True)
    free = _closed_loop(kind, steps, False)
    print(f"{kind}: checked {r['checked']} of {steps}, worst diff / bar {r['worst']:.3g}, active steps {r['active']}, eps max {r['eps_max']:.4f}, "
          f"branches (kin, dyn) {r['branches']}, closest approach {r['dmin']:.3f} m with QP_AVOID, {free['dmin']:.3f} m without")
    for step, ds, dv, bar in r["diffs"]:
        assert ds <= bar and dv <= bar, (step, ds, dv, bar)
    assert r["checked"] >= 0.9 * steps and r["active"] >= 1 and r["branches"][1] >= 1


# ---- 7. rivals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predict", ["velocity", "track"])
@pytest.mark.parametrize("tracks", [False, True])
def test_rivals_equal_the_same_slots_as_obstacles(ctx, predict, tracks):
    """E = 8 on two staggered lines of vehicles along levine, speeds on both sides of V_KS: planner.rivals against planner.obstacles = the
    slots runtime.rivals returns, with and without tracks"""
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    from f1tenth_planning_amd.runtime import rivals_predict, rivals_set_course
    cx, cy, cyaw, sp = SC.levine()
    k = 300 + 22 * np.arange(8)                                  # 0.76 m apart along the line, alternately 0.2 m left and right of it
    lat = np.where(np.arange(8) % 2 == 0, 0.2, -0.2)
    x0 = np.column_stack([cx[k] - lat * np.sin(cyaw[k]), cy[k] + lat * np.cos(cyaw[k]), np.zeros(8), np.linspace(3.5, 1.0, 8), cyaw[k], np.zeros(8),
                          np.zeros(8)])
    T, TK = 10, 8
    course = [cx, cy, cyaw, sp]
    ids = np.zeros(8, np.int32)
    kw = dict(tracks=[course], track_ids=ids) if tracks else {}

    def make():
        return STMPCPlanner(waypoints=[a.copy() for a in course], config=mpc_config(SOLVER="qp", QP_AVOID=True, T=T, TK=TK))
    a, b, free = make(), make(), make()
    a.rivals = Rivals(count=2, radius=0.45, predict=predict)
    if predict == "track":
        wp = np.column_stack([cx, cy, sp, cyaw])
        if tracks:
            ctx.set_tracks([wp], cols=(0, 1, 2, 3))
            rivals_set_course(ctx, ids)
        else:
            ctx.set_waypoints(wp, cols=(0, 1, 2, 3))
            rivals_set_course(ctx, None)
        slots = rivals_predict(ctx, x0, "st7", 2, 0.45, max(T * 0.025, TK * 0.1))
    else:
        slots = rivals(ctx, x0, "st7", 2, 0.45)
    assert (slots["idx"] >= 0).all()
    got = a.plan_batch(x0, **kw)
    b.obstacles = slots["obs"]
    want = b.plan_batch(x0, **kw)
    for key in ("steer", "speed", "status", "branch"):
        assert np.array_equal(got[key], want[key]), key
    assert set(got["branch"].tolist()) == {0, 1}
    assert (got["steer"] != free.plan_batch(x0, **kw)["steer"]).any()   # the rows matter in this scene
    if tracks:
        ctx.set_tracks([])
