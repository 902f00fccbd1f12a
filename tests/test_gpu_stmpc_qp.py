"""f1p_stmpc_qp_*: the reference's linearised dynamic-MPC QP (dynamic_mpc.py:279-1117) solved on the GPU, against the exact solutions of
the yardstick (tests/stmpc_qp_ref.py) on the reference's recorded problems (golden G17, both branches) and at scale, with KKT certificates
from the returned duals; batch invariance, bad inputs, the mixed-branch plan chain's warm-start rules and the STMPCPlanner class."""
import numpy as np
import pytest

import kmpc_qp_ref as KQ
import qp_cases as QC
import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi, synth
from f1tenth_planning_amd.runtime import Context
from test_stmpc_qp_host import g17_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def _dcfg(T=40):
    return _abi.stmpc_cfg(horizon=T)


def _kcfg(TK=8):
    """STMPCPlanner's kinematic branch config (its mpc_config's TK, DTK, Rk, Rdk, Qk, Qfk, MAX_DSTEER)"""
    return _abi.kmpc_cfg(horizon=TK)


def _bar(deg):
    return 1e-5 if deg else 1e-7


def _u_bar(c, u, lam, us, lam_s, deg):
    """how far u may lie from the exact optimum us: the bar above, or -- where the objective is weakly curved -- the distance that the two
    points' own KKT residuals allow in a strongly convex QP (mu = lambda_min(H), r = H u + g + G'lam, s = h - G u: from the two
    strong-convexity inequalities, mu |u - us|^2 <= lam's + lam_s's_s + |r - r_s| |u - us|), with a factor 2"""
    H, g, G, h = c["H"], c["g"], c["G"], c["h"]
    mu = np.linalg.eigvalsh(H).min()
    dr = np.linalg.norm((H @ u + g + G.T @ lam) - (H @ us + g + G.T @ lam_s))
    gap = np.abs(lam * (h - G @ u)).sum() + np.abs(lam_s * (h - G @ us)).sum()
    return max(_bar(deg), 2.0 * (dr + np.sqrt(dr * dr + 4.0 * mu * gap)) / (2.0 * mu))


def _fval(c, u):
    return 0.5 * u @ c["H"] @ u + c["g"] @ u


# ---- 1. the reference's recorded problems ------------------------------------------------------------------------------------------
def test_g17_cases_match_the_exact_optimum(ctx, golden):
    cases = g17_cases(golden)
    for branch, T in (("dyn", 40), ("dyn", 10), ("kin", 8)):
        cs = [c for c in cases if c["branch"] == branch and c["T"] == T]
        assert cs
        x0, ref = np.array([c["x0"] for c in cs]), np.array([c["ref"] for c in cs])
        oa, od = np.array([c["oa"] for c in cs]), np.array([c["od"] for c in cs])
        if branch == "dyn":
            out = ctx.stmpc_qp(x0, ref, _dcfg(T), oa_prev=oa, od_v_prev=od, want_x=True, want_duals=True)
            xs, rows, p = out["x"], SQ.gpu_rows(T), SQ.default_params(T)
        else:
            out = ctx.kmpc_qp(x0, ref, _kcfg(T), oa_prev=oa, od_prev=od, want_xk=True, want_duals=True)
            xs, rows, p = out["xk"], KQ.gpu_rows(T), SQ.kin_params(T)
        assert (out["status"] == 0).all(), (branch, T, out["status"])
        for e, c in enumerate(cs):
            r = c["rec"]
            lam = np.zeros(len(r["h"]))
            lam[rows] = out["duals"][e]
            z = np.concatenate([xs[e].T.ravel(), out["u"][e].ravel()])
            cert = SQ.certificate(r["P"], r["q"], r["Aeq"], r["beq"], r["G"], r["h"], z, lam)
            assert cert["primal"] <= 1e-9 and cert["dual"] >= -1e-10 and cert["comp"] <= 1e-9 and cert["stat"] <= 1e-8, (branch, T, e, cert)
            obj_rec = 0.5 * z @ r["P"] @ z + r["q"] @ z + r["r"]             # the value cvxpy would report at the GPU's point
            assert abs(out["obj"][e] - obj_rec) <= 1e-10 * (1.0 + abs(obj_rec)), (branch, T, e)
            if branch == "dyn":
                cond = SQ.condense(SQ.qp_data(c["x0"], c["ref"], c["oa"], c["od"], p), T)
            else:
                cond = KQ.condense(KQ.qp_data(c["x0"], c["ref"], c["oa"], c["od"], p), T)
            us, lam_s, deg = SQ.exact(cond, out["duals"][e])
            if not SQ.exact_ok(cond, us, lam_s):
                continue                                   # a degenerate case the helper could not settle: the certificate above decided
            ug = out["u"][e].ravel()
            bar = _u_bar(cond, ug, out["duals"][e], us, lam_s, deg)
            assert np.abs(ug - us).max() <= bar, (branch, T, e, np.abs(ug - us).max(), bar)
            fg, fs = _fval(cond, ug), _fval(cond, us)
            assert abs(fg - fs) <= 1e-10 * (1.0 + abs(fs)), (branch, T, e, fg - fs)                # the optimal value, tightly


# ---- 2. scale -----------------------------------------------------------------------------------------------------------------------
def _waypoints(ctx, tracks, name):
    t = tracks[name]
    if name == "levine":
        cx, cy, cyaw, sp = (np.ascontiguousarray(t[:, c]) for c in (1, 2, 3, 5))
    else:
        cx, cy, cyaw, sp = (np.ascontiguousarray(t[:, c]) for c in (0, 1, 3, 2))
    ctx.set_waypoints(np.column_stack([cx, cy, sp, cyaw]), cols=(0, 1, 2, 3))
    return cx, cy, cyaw, sp


def _scale_inputs(ctx, tracks, name, E, T, seed):
    """dynamic-branch states on a track: speeds 2.05..6 (a tenth at MAX_SPEED), steering up to the bounds (some exactly at them), heading
    errors up to +-0.9 rad, yaw rates and slip angles, reference speeds scaled 0.3..1.6x, a random previous solution for half the egos"""
    rng = np.random.default_rng(seed)
    cx, cy, cyaw, sp = _waypoints(ctx, tracks, name)
    k = rng.integers(0, len(cx) - 1, E)
    v = rng.uniform(2.05, 6.0, E)
    v[rng.random(E) < 0.1] = 6.0
    d = rng.uniform(-0.35, 0.35, E)
    d[rng.random(E) < 0.05] = 0.4189 * rng.choice([-1.0, 1.0])
    yaw = cyaw[k] + rng.normal(0, 0.3, E).clip(-0.9, 0.9)
    x0 = np.column_stack([cx[k] + rng.normal(0, 0.3, E), cy[k] + rng.normal(0, 0.3, E), d, v, yaw, rng.normal(0, 0.5, E),
                          rng.normal(0, 0.03, E)])
    ref = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], T)
    ref[:, 3, :] *= rng.uniform(0.3, 1.6, E)[:, None]
    warm = rng.random(E) < 0.5
    oa = np.where(warm[:, None], rng.normal(0.3, 1.0, (E, T)).clip(-2, 3), 0.0)
    odv = np.where(warm[:, None], rng.normal(0, 1.0, (E, T)).clip(-3.2, 3.2), 0.0)
    return x0, ref, oa, odv


@pytest.mark.parametrize("E,T,name", [(1024, 40, "levine"), (1024, 40, "spielberg"), (4096, 10, "levine"), (4096, 10, "spielberg")])
def test_scale_certificates(ctx, tracks, E, T, name):
    x0, ref, oa, odv = _scale_inputs(ctx, tracks, name, E, T, seed=E + T + len(name))
    out = ctx.stmpc_qp(x0, ref, _dcfg(T), oa_prev=oa, od_v_prev=odv, want_duals=True)
    # statuses 0, except at most one ego in a thousand with delta0 exactly at +-MAX_STEER whose Newton matrix breaks down just short of
    # tol: its iterate is returned with status 2 and must still certify at a looser bar
    st2 = np.flatnonzero(out["status"] != 0)
    assert (out["status"][st2] == 2).all() and len(st2) <= E // 1000, np.unique(out["status"], return_counts=True)
    assert all(abs(x0[e, 2]) == 0.4189 for e in st2), st2
    p = SQ.default_params(T)
    fam = {"rate": slice(0, 2 * T - 2), "steer": slice(2 * T - 2, 4 * T - 2), "speed": slice(4 * T - 2, 6 * T - 2),
           "steer_v": slice(6 * T - 2, 8 * T - 2), "accel": slice(8 * T - 2, 10 * T - 2)}
    binds = {f: 0 for f in fam}
    rng = np.random.default_rng(1)
    exact = set(rng.choice(E, 32, replace=False).tolist())
    for e in range(E):
        c = SQ.fast_condense(x0[e], ref[e], oa[e], odv[e], p)
        u, lam = out["u"][e].ravel(), out["duals"][e]
        cert = SQ.cond_cert(c, u, lam)
        cert["comp"] /= 1.0 + lam.max()                  # relative to the multipliers' scale: lambda ~ 1e2 times a slack within tol
        if e in st2:
            assert cert["primal"] <= 1e-9 and cert["dual"] >= -1e-10 and cert["comp"] <= 1e-8 and cert["stat"] <= 1e-8, (e, cert)
            continue
        assert SQ.cert_ok(cert), (e, cert)
        for f, s in fam.items():
            binds[f] += bool((lam[s] > 1e-6).any())
        if e in exact:
            us, lam_s, deg = SQ.exact(c, lam)
            if SQ.exact_ok(c, us, lam_s):
                assert np.abs(u - us).max() <= _u_bar(c, u, lam, us, lam_s, deg), (e, np.abs(u - us).max())
                assert abs(_fval(c, u) - _fval(c, us)) <= 1e-10 * (1.0 + abs(_fval(c, us))), e
    assert binds["steer"] > 0 and binds["steer_v"] > 0 and binds["accel"] > 0 and binds["speed"] > 0, binds


# ---- 3. batch invariance ------------------------------------------------------------------------------------------------------------
def test_batch_invariance(ctx, tracks):
    T = 40
    x0, ref, oa, odv = _scale_inputs(ctx, tracks, "levine", 4096, T, seed=77)
    keys = ("steer", "speed", "status", "u", "x", "obj", "duals", "iters")
    full = ctx.stmpc_qp(x0, ref, _dcfg(T), oa_prev=oa, od_v_prev=odv, want_x=True, want_duals=True)
    for e in (0, 5, 2001, 4095):
        one = ctx.stmpc_qp(x0[e:e + 1], ref[e:e + 1], _dcfg(T), oa_prev=oa[e:e + 1], od_v_prev=odv[e:e + 1], want_x=True, want_duals=True)
        lo = min(max(0, e - 17), 4096 - 63)
        sub = slice(lo, lo + 63)
        mid = ctx.stmpc_qp(x0[sub], ref[sub], _dcfg(T), oa_prev=oa[sub], od_v_prev=odv[sub], want_x=True, want_duals=True)
        for k in keys:
            assert np.array_equal(one[k][0], full[k][e]), (e, k)
            assert np.array_equal(mid[k][e - lo], full[k][e]), (e, k)


# ---- 4. bad inputs -----------------------------------------------------------------------------------------------------------------
def test_bad_inputs(ctx, tracks):
    T = 10
    x0, ref, oa, odv = _scale_inputs(ctx, tracks, "levine", 64, T, seed=5)
    keys = ("steer", "speed", "status", "u", "x", "obj", "duals", "iters")
    good = ctx.stmpc_qp(x0, ref, _dcfg(T), oa_prev=oa, od_v_prev=odv, want_x=True, want_duals=True)
    at = [3, 17, 30, 41, 50, 60]
    x0b, refb, oab, odvb = (np.insert(a, [3, 16, 28, 38, 46, 55], a[:1] * 0 + a[0], axis=0) for a in (x0, ref, oa, odv))
    x0b[3, 0] = np.nan                                   # NaN in x0: 3
    refb[17, 4, 5] = np.nan                              # NaN in ref: 3
    x0b[30, 3] = 6.2                                     # v0 > MAX_SPEED: 1
    x0b[41, 2] = -0.42                                   # |delta0| > MAX_STEER: 1
    x0b[50, 3] = 0.5; oab[50] = -3.0                     # the warm start brakes the prediction to v = 0 (MIN_SPEED): 3
    oab[60, 2] = np.inf                                  # non-finite warm start: 3
    out = ctx.stmpc_qp(x0b, refb, _dcfg(T), oa_prev=oab, od_v_prev=odvb, want_x=True, want_duals=True)
    assert [int(out["status"][i]) for i in at] == [3, 3, 1, 1, 3, 3]
    for i in at:
        for k in ("steer", "speed", "u", "x", "obj", "duals"):
            assert np.isnan(out[k][i]).all(), (i, k)
    keep = [i for i in range(len(x0b)) if i not in at]
    for k in keys:
        assert np.array_equal(out[k][keep], good[k]), k
    assert SQ.solve_case(x0b[50], refb[50], oab[50], odvb[50], SQ.default_params(T)) is None
    with pytest.raises(ValueError):                      # horizon > F1P_STMPC_QP_MAX_T: F1P_EINVAL
        ctx.stmpc_qp(x0[:1], ctx.stmpc_ref(x0[:1, [0, 1, 3, 4]], 45), _dcfg(45))
    empty = ctx.stmpc_qp(np.zeros((0, 7)), np.zeros((0, 7, T + 1)), _dcfg(T))
    assert empty["steer"].shape == (0,)


# ---- 5. the plan chain --------------------------------------------------------------------------------------------------------------
def _chain_track(ctx):
    """a synthetic centreline whose speed profile is 4 m/s on the first half and 1 m/s on the second: egos on the first half accelerate
    through V_KS, egos on the second half brake through it"""
    cl = synth.make_centerline(seed=4)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    rl[:, 2] = np.where(np.arange(len(rl)) < len(rl) // 2, 4.0, 1.0)
    ctx.set_waypoints(rl)
    return rl


def _host_chain_step(ctx, states, warms, p, pk, gpu):
    """one step of the host chain: every ego's plan_step, the references from the device's extraction (tested elsewhere)"""
    steer, speed, br = np.empty(len(states)), np.empty(len(states)), np.empty(len(states), int)
    rd = ctx.stmpc_ref(states[:, [0, 1, 3, 4]], p["T"], p["DT"], 0.03)
    rk = ctx.stmpc_ref(states[:, [0, 1, 3, 4]], pk["T"], pk["DTK"], 0.03)[:, [0, 1, 3, 4]]
    degs = []
    for e, s in enumerate(states):
        steer[e], speed[e], warms[e], br[e], deg = SQ.plan_step(s, warms[e], rd[e], rk[e], p, pk)
        degs.append(deg)
    return steer, speed, br, np.array(degs)


def _chain_case(off_default):
    """(dcfg, kcfg, p, pk): the defaults at T = 10, TK = 8, or an off-default pair of tests/qp_cases.py at T = 12, TK = 5 (TK <= T) with
    each branch's own time step and weights; one STMPCPlanner config holds one set of bounds and one wheelbase for both branches"""
    if not off_default:
        return _dcfg(10), _kcfg(8), SQ.default_params(10), SQ.kin_params(8)
    ds, ks = QC.stmpc_spec(403, 12), QC.kmpc_spec(404, 5)
    shared = dict(WB=0.31, MAX_STEER=0.45, MAX_SPEED=6.5, MIN_SPEED=0.0, MAX_ACCEL=4.0)
    ds.update(shared, DT=0.025)                          # (DT = 0.05 makes the reference's Euler step of the slip angle unstable: DESIGN.md 5c)
    ks.update(shared, DTK=0.05)
    return QC.stmpc_cfg(ds), QC.kmpc_cfg(ks), QC.stmpc_params(ds), QC.kmpc_params(ks)


@pytest.mark.parametrize("off_default", [False, True], ids=["default-T10-TK8", "offdefault-T12-TK5"])
def test_plan_chain_equals_the_host_chain(ctx, off_default):
    dcfg, kcfg, p, pk = _chain_case(off_default)
    T, TK, E = p["T"], pk["T"], 8
    rl = _chain_track(ctx)
    n = len(rl)
    k0 = np.array([10, 60, 110, 160, n // 2 + 10, n // 2 + 60, n // 2 + 110, n // 2 + 160])
    v = np.array([1.8, 1.9, 2.6, 3.5, 2.3, 2.15, 1.5, 3.0])
    states = np.column_stack([rl[k0, 0] + 0.05, rl[k0, 1] - 0.05, np.full(E, 0.02), v, rl[k0, 3] + 0.03, np.zeros(E), np.zeros(E)])
    ctx.stmpc_qp_warm_reset()
    warms = [None] * E
    branches = []
    for step in range(10 if off_default else 24):            # (the off-default chain has crossed V_KS both ways by then)
        got = ctx.stmpc_qp_plan(states, dcfg, kcfg, v_ks=2.0, dl=0.03, dlk=0.03)
        assert (got["status"] == 0).all(), (step, got["status"])
        steer, speed, br, deg = _host_chain_step(ctx, states, warms, p, pk, got)
        assert np.array_equal(got["branch"], br), step
        bar = np.where(deg, 1e-5, 1e-7)
        assert (np.abs(got["steer"] - steer) <= bar).all() and (np.abs(got["speed"] - speed) <= bar).all(), \
            (step, np.abs(got["steer"] - steer).max(), np.abs(got["speed"] - speed).max())
        for e in range(E):                               # the new warm start: the branch's horizon, NaN beyond
            L = T if br[e] else TK
            assert np.isnan(got["u"][e, L:]).all() and np.abs(got["u"][e, :L, 0] - warms[e][0]).max() <= 1e-4   # (weakly determined tail inputs)
        branches.append(br)
        states = np.array([SQ.plant(states[e], got["steer"][e], got["speed"][e], p) for e in range(E)])
    b = np.array(branches)
    assert ((b[:-1] == 0) & (b[1:] == 1)).any() and ((b[:-1] == 1) & (b[1:] == 0)).any()        # crossings in both directions
    w, lens = ctx.stmpc_qp_warm_get(E, T)
    assert list(lens) == [T if x else TK for x in b[-1]]
    ctx.stmpc_qp_warm_reset()
    assert (ctx.stmpc_qp_warm_get(E, T)[1] == 0).all()


# ---- 6. the class equals the batch ---------------------------------------------------------------------------------------------------
def _levine(tracks):
    lev = tracks["levine"]
    cx, cy, cyaw, sp = (np.ascontiguousarray(lev[:, c]) for c in (1, 2, 3, 5))
    return cx, cy, cyaw, sp


def test_class_plan_equals_plan_batch(tracks):
    from f1tenth_planning.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    cx, cy, cyaw, sp = _levine(tracks)
    rng = np.random.default_rng(11)
    k = rng.integers(0, len(cx) - 1, 6)
    st = np.column_stack([cx[k], cy[k], rng.uniform(-0.2, 0.2, 6), [1.0, 1.9, 2.0, 2.3, 4.0, 5.5], cyaw[k] + rng.normal(0, 0.1, 6),
                          rng.normal(0, 0.2, 6), rng.normal(0, 0.02, 6)])
    batch = STMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp"))
    out = batch.plan_batch(st)
    assert (out["status"] == 0).all() and list(out["branch"]) == [0, 0, 0, 1, 1, 1]
    for e in range(6):
        one = STMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp"))
        steer, speed = one.plan(st[e])
        assert steer == out["steer"][e] and speed == out["speed"][e], e
        L = 40 if out["branch"][e] else 8
        assert np.array_equal(one.oa, out["u"][e, :L, 0]) and np.array_equal(one.odelta_v, out["u"][e, :L, 1])
    bad = STMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp"))
    with pytest.raises(RuntimeError):
        bad.plan(np.array([cx[0], cy[0], 0.0, 6.5, cyaw[0], 0.0, 0.0]))


# ---- 7. closed loop through the class ---------------------------------------------------------------------------------------------
def test_class_closed_loop_through_v_ks_on_levine(ctx, tracks):
    from f1tenth_planning.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    cx, cy, cyaw, sp = _levine(tracks)
    planner = STMPCPlanner(waypoints=[cx, cy, cyaw, sp], config=mpc_config(SOLVER="qp"))
    _waypoints(ctx, tracks, "levine")                    # the host chain's references come from this ctx
    p, pk = SQ.default_params(40), SQ.kin_params(8)
    s = np.array([cx[0], cy[0], 0.0, 1.2, cyaw[0], 0.0, 0.0])
    warm = None
    br_seen = []
    checked = 0
    for step in range(40):
        steer, speed = planner.plan(s)
        rd = ctx.stmpc_ref(s[None, [0, 1, 3, 4]], 40, 0.025, 0.03)[0]
        rk = ctx.stmpc_ref(s[None, [0, 1, 3, 4]], 8, 0.1, 0.03)[0][[0, 1, 3, 4]]
        h_steer, h_speed, warm, br, deg = SQ.plan_step(s, warm, rd, rk, p, pk)
        assert abs(steer - h_steer) <= _bar(deg) and abs(speed - h_speed) <= _bar(deg), (step, steer - h_steer, speed - h_speed)
        checked += 1
        br_seen.append(br)
        s = SQ.plant(s, steer, speed, p)
    assert 0 in br_seen and 1 in br_seen and br_seen[0] == 0           # started below V_KS and accelerated through it
    assert checked == 40
    planner.reset()
    assert planner.oa is None
