"""f1p_kmpc_qp_avoid_* and KMPCPlanner(SOLVER="qp", QP_AVOID=True): the moving-disc avoidance rows of the kinematic QP against
the exact optima of tests/kmpc_qp_avoid_ref.py -- every family of rows, the half-planes themselves, KKT certificates from the returned
multipliers; an ego without discs against the plain QP; neighbour independence; errors; the class in closed loop on the two levine scenes;
rivals against the same slots given as obstacles."""
import numpy as np
import pytest

import kmpc_qp_avoid_ref as A
import kmpc_qp_avoid_scenes as SC
import kmpc_qp_ref as Q
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._rivals import Rivals
from f1tenth_planning_amd.runtime import Context, F1PError, kmpc_qp_avoid, kmpc_qp_set_avoid, kmpc_set_obstacles, rivals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _cfg(T):
    return _abi.kmpc_cfg(horizon=T)


def _solve(ctx, T, M, sel=slice(None), **want):
    x0, ref, oa, od, obs, _ = SC.exact_scene(T, M)
    return kmpc_qp_avoid(ctx, x0[sel], ref[sel], obs[sel], _cfg(T), oa_prev=oa[sel], od_prev=od[sel], want_xk=True, want_duals=True,
                         want_planes=True, want_avoid_duals=True, **want)


OUT_KEYS = ("steer", "speed", "status", "u", "xk", "obj", "duals", "iters", "eps", "planes", "avoid_duals")


# ---- 1. the exact optimum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", SC.SHAPES)
def test_exact_optimum_planes_and_certificates(ctx, T, M):
    x0, ref, oa, od, obs, fam = SC.exact_scene(T, M)
    sols = SC.exact_solutions(T, M)
    SC.assert_families(T, M, obs, sols, fam)
    out = _solve(ctx, T, M)
    assert np.array_equal(out["status"], SC.expected_status(T, M)), out["status"]
    skipped = 0
    worst = dict(u=0.0, eps=0.0, n=0.0, rhs=0.0)
    for e, s in enumerate(sols):
        if s is None:                                          # status 1 / 3: NaN in every output
            for k in OUT_KEYS:
                if k not in ("status", "iters"):
                    assert np.isnan(out[k][e]).all(), (e, k)
            continue
        pl, ref_pl = out["planes"][e], s["planes"]
        assert np.array_equal(pl[:, :, 3], ref_pl[:, :, 3]), (e, pl[:, :, 3], ref_pl[:, :, 3])
        assert (np.abs(pl[:, :, :3] - ref_pl[:, :, :3]) <= 1e-12 * (1.0 + np.abs(ref_pl[:, :, :3]))).all(), (e, np.abs(pl - ref_pl).max())
        assert (pl[pl[:, :, 3] < 0][:, :3] == 0.0).all()
        worst["n"] = max(worst["n"], float(np.abs(pl[:, :, :2] - ref_pl[:, :, :2]).max()))
        worst["rhs"] = max(worst["rhs"], float((np.abs(pl[:, :, 2] - ref_pl[:, :, 2]) / (1.0 + np.abs(ref_pl[:, :, 2]))).max()))
        b = s["build"]
        w = np.concatenate([out["u"][e].ravel(), [out["eps"][e]]])
        cert = A.cert(b, w, A.lam_full(b, out["duals"][e], out["avoid_duals"][e]))
        assert A.cert_ok(cert), (e, cert)
        absent = np.setdiff1d(np.arange(2 * T), b["rows"])
        assert (out["avoid_duals"][e][absent] == 0.0).all()
        # obj: the value of the problem's objective at the GPU's point (the plain QP's constant included)
        obj = 0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"]
        assert abs(out["obj"][e] - obj) <= 1e-9 * (1.0 + abs(obj)), (e, out["obj"][e], obj)
        if not A.cert_ok(s["cert"]):
            skipped += 1                                       # the reference does not certify itself here: the certificate above decided
            continue
        bar = 1e-5 if s["degenerate"] else 1e-7
        du, de = float(np.abs(out["u"][e] - s["u"]).max()), abs(float(out["eps"][e]) - s["eps"])
        worst["u"], worst["eps"] = max(worst["u"], du / bar), max(worst["eps"], de / bar)
        assert du <= bar and de <= bar, (e, du, de, bar)
    print(f"T={T} M={M}: skipped {skipped}, worst |du| / bar {worst['u']:.3g}, |deps| / bar {worst['eps']:.3g}, |dn| {worst['n']:.3g}, "
          f"rel |drhs| {worst['rhs']:.3g}, iters max {int(out['iters'].max())}")
    assert skipped <= 0.05 * SC.E, skipped


# ---- 2. no live slot: the plain QP's optimum -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(2, 1), (8, 4), (31, 16)])
def test_no_live_slot_agrees_with_the_plain_qp(ctx, T, M):
    x0, ref, oa, od, obs, fam = SC.exact_scene(T, M)
    sel = fam["no_live"]
    got = _solve(ctx, T, M, sel)
    plain = ctx.kmpc_qp(x0[sel], ref[sel], _cfg(T), oa_prev=oa[sel], od_prev=od[sel])
    assert (got["status"] == 0).all() and (plain["status"] == 0).all()
    assert np.abs(got["u"] - plain["u"]).max() <= 2e-7
    assert np.abs(got["eps"]).max() <= 1e-7 and (got["planes"][:, :, :, 3] == -1).all()
    p = Q.default_params(T)
    for i, e in enumerate(sel):
        s = Q.solve_case(x0[e], ref[e], oa[e], od[e], p)
        bar = 1e-5 if s["degenerate"] else 1e-7
        assert np.abs(got["u"][i] - s["u"]).max() <= bar and np.abs(plain["u"][i] - s["u"]).max() <= bar, (e, bar)


# ---- 3. neighbour independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(2, 1), (8, 4), (15, 4), (16, 4), (31, 16)])
def test_neighbour_independence(ctx, T, M):
    """T = 15 is the last horizon with two egos per wave, 16 the first with one"""
    if (T, M) in SC.SHAPES:
        x0, ref, oa, od, obs, _ = SC.exact_scene(T, M)
    else:
        x0, ref, oa, od, obs, _ = SC.exact_scene(8, M)
        rng = np.random.default_rng(T)
        cx, cy, cyaw, sp = SC.levine()
        p = Q.default_params(T)
        ref = np.array([Q.ref_trajectory(x0[e], cx, cy, cyaw.copy(), sp, p, dlk=0.03) for e in range(SC.E)])
        oa, od = rng.normal(0.0, 0.5, (SC.E, T)), rng.normal(0.0, 0.05, (SC.E, T))
    cfg = _cfg(T)
    kw = dict(want_xk=True, want_duals=True, want_planes=True, want_avoid_duals=True)
    full = kmpc_qp_avoid(ctx, x0, ref, obs, cfg, oa_prev=oa, od_prev=od, **kw)
    perm = np.random.default_rng(5).permutation(SC.E)
    shuf = kmpc_qp_avoid(ctx, x0[perm], ref[perm], obs[perm], cfg, oa_prev=oa[perm], od_prev=od[perm], **kw)
    for k in OUT_KEYS:
        assert np.array_equal(shuf[k], full[k][perm], equal_nan=True), k
    for e in (0, 15, 22, 30, 36, 44, 50, 63):                  # one of (nearly) every family, alone
        one = kmpc_qp_avoid(ctx, x0[e:e + 1], ref[e:e + 1], obs[e:e + 1], cfg, oa_prev=oa[e:e + 1], od_prev=od[e:e + 1], **kw)
        for k in OUT_KEYS:
            assert np.array_equal(one[k][0], full[k][e], equal_nan=True), (e, k)


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    x0, ref, oa, od, obs, _ = SC.exact_scene(8, 4)
    with pytest.raises(ValueError):                            # F1P_EINVAL: 2T + 1 inputs need T <= 31
        kmpc_qp_avoid(ctx, x0[:1], np.zeros((1, 4, 33)), obs[:1], _cfg(32))
    for M in (0, 17):
        with pytest.raises(ValueError):
            kmpc_qp_avoid(ctx, x0[:2], ref[:2], np.zeros((2, M, 5)), _cfg(8))
    for bad in (dict(rho=0.0), dict(rho=np.nan), dict(lin=-1.0), dict(margin=np.inf)):
        with pytest.raises(ValueError):
            kmpc_qp_avoid(ctx, x0[:2], ref[:2], obs[:2], _cfg(8), avoid=_abi.kmpc_qp_avoid(**bad))
        with pytest.raises(ValueError):
            kmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid(**bad))
    # the plan path: the discs of kmpc_set_obstacles, and its E-mismatch error; off: ignored as before
    cx, cy, cyaw, sp = SC.levine()
    ctx.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
    ctx.kmpc_qp_warm_reset()
    kmpc_set_obstacles(ctx, obs[:4])
    plain = ctx.kmpc_qp_plan(x0[:8], _cfg(8))                   # off: E = 8 against obstacles for 4 is no error
    kmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid())
    with pytest.raises(F1PError, match="obstacles were set for 4 egos, this plan has 8"):
        ctx.kmpc_qp_plan(x0[:8], _cfg(8))
    with pytest.raises(ValueError):
        ctx.kmpc_qp_plan(x0[:4], _cfg(32))
    kmpc_set_obstacles(ctx, None)
    ctx.kmpc_qp_warm_reset()
    none = ctx.kmpc_qp_plan(x0[:8], _cfg(8))                    # on, nothing held: no avoidance rows
    assert np.abs(none["u"] - plain["u"]).max() <= 2e-7
    kmpc_qp_set_avoid(ctx, None)
    ctx.kmpc_qp_warm_reset()
    again = ctx.kmpc_qp_plan(x0[:8], _cfg(8))
    for k in ("steer", "speed", "status", "u", "obj"):
        assert np.array_equal(again[k], plain[k]), k
    ctx.kmpc_qp_warm_reset()


def test_plan_path_takes_the_context_obstacles(ctx):
    """kmpc_qp_plan with the switch on equals kmpc_qp_avoid on the same reference, discs and previous solution, two calls in a row"""
    x0, _, _, _, obs, _ = SC.exact_scene(8, 4)
    keep = SC.expected_status(8, 4) == 0
    x0, obs = x0[keep], obs[keep]
    cx, cy, cyaw, sp = SC.levine()
    ctx.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
    ctx.kmpc_qp_warm_reset()
    av = _abi.kmpc_qp_avoid(margin=0.05)
    kmpc_qp_set_avoid(ctx, av)
    kmpc_set_obstacles(ctx, obs)
    oa = od = None
    try:
        for step in range(2):
            got = ctx.kmpc_qp_plan(x0, _cfg(8))
            want = kmpc_qp_avoid(ctx, x0, ctx.kmpc_ref(x0, 8), obs, _cfg(8), avoid=av, oa_prev=oa, od_prev=od)
            for k in ("steer", "speed", "status", "u", "obj"):
                assert np.array_equal(got[k], want[k]), (step, k)
            oa, od = want["u"][:, :, 0].copy(), want["u"][:, :, 1].copy()
        assert (want["eps"] > 1e-3).any()
    finally:
        kmpc_set_obstacles(ctx, None)
        kmpc_qp_set_avoid(ctx, None)
        ctx.kmpc_qp_warm_reset()


# ---- 5. the class in closed loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parked", "moving"])
def test_class_closed_loop(tracks, kind):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    lev = tracks["levine"]
    cx, cy, cyaw, sp = (np.ascontiguousarray(lev[:, c]) for c in (1, 2, 3, 5))
    planner = KMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp", QP_AVOID=True))

    def plan(state, disc):
        planner.obstacles = disc[None]
        out = planner.plan(state)
        assert planner.obstacles is None
        return out

    steps = 201
    r = SC.run_scene(tracks["levine"], kind, steps, plan=plan)
    worst = max(max(ds, dv) / bar for _, ds, dv, bar in r["diffs"])
    print(f"{kind}: checked {len(r['diffs'])} of {steps}, worst diff / bar {worst:.3g}, active steps {len(r['active'])}, dmin {r['dmin']:.3f}")
    for step, ds, dv, bar in r["diffs"]:
        assert ds <= bar and dv <= bar, (step, ds, dv, bar)
    assert len(r["diffs"]) >= 0.95 * steps
    # parked: the issue's bars of the reference's own run (rows active on >= 50 steps, all of them within these 201; >= 0.30 m from the centre);
    # moving: the rows bind and the ego stays outside the disc's radius
    assert len(r["active"]) >= (50 if kind == "parked" else 1)
    assert r["dmin"] >= (0.30 if kind == "parked" else 0.45)


# ---- 6. rivals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("predict", ["velocity", "track"])
def test_rivals_equal_the_same_slots_as_obstacles(ctx, tracks, predict):
    """E = 8 on two staggered lines of vehicles along levine: planner.rivals against planner.obstacles = the slots runtime.rivals returns"""
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    from f1tenth_planning_amd.runtime import rivals_predict, rivals_set_course
    lev = tracks["levine"]
    cx, cy, cyaw, sp = (np.ascontiguousarray(lev[:, c]) for c in (1, 2, 3, 5))
    k = 300 + 22 * np.arange(8)                                  # 0.76 m apart along the line, alternately 0.2 m left and right of it
    lat = np.where(np.arange(8) % 2 == 0, 0.2, -0.2)
    x0 = np.column_stack([cx[k] - lat * np.sin(cyaw[k]), cy[k] + lat * np.cos(cyaw[k]), np.linspace(3.0, 1.0, 8), cyaw[k]])

    def make():
        return KMPCPlanner(waypoints=[cx.copy(), cy.copy(), cyaw.copy(), sp.copy()], config=mpc_config(SOLVER="qp", QP_AVOID=True))
    a, b, free = make(), make(), make()
    a.rivals = Rivals(count=2, radius=0.45, predict=predict)
    if predict == "track":
        ctx.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
        rivals_set_course(ctx, None)
        slots = rivals_predict(ctx, x0, "xyvyaw", 2, 0.45, 8 * 0.1)
    else:
        slots = rivals(ctx, x0, "xyvyaw", 2, 0.45)
    assert (slots["idx"] >= 0).all()
    got = a.plan_batch(x0)
    b.obstacles = slots["obs"]
    want = b.plan_batch(x0)
    for key in ("steer", "speed", "status"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["status"] == 0).all()
    assert (got["steer"] != free.plan_batch(x0)["steer"]).any()   # the rows matter in this scene
