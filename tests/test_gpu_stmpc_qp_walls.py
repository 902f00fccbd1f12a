"""f1p_stmpc_qp_walls_* and STMPCPlanner(SOLVER="qp", QP_WALLS_ST=True): the wall rows of the dynamic QP against the exact optima
of tests/stmpc_qp_walls_ref.py on the hand-made grid of tests/kmpc_qp_walls_scenes.py -- the half-planes themselves (left and right of the
direction of travel yaw + beta, not of the yaw), KKT certificates from the returned multipliers, every family of rows; the ends of the march's
eight-sample group; an ego without a candidate against the plain and the disc QPs; neighbour independence; _dev against _batch; the errors
of the three C entry points; the plan path in both branches and a grid that changes under it; track sets and rivals; the class in closed
loop beside a wall its raceline runs into.

The bars are DESIGN.md 5r's as tests/test_gpu_stmpc_qp_avoid.py applies them.  Statuses are asserted ego for ego against
stmpc_qp_walls_scenes.expected_status (status 2, the last iterate: DESIGN.md 5s "Status 2"; an ego recorded there is held to every bar of a
converged one); the closed loop may leave at most 5 % of its plans unchecked and at most 5 % at status 2.

Measured on an MI355X: no ego of any shape at status 2; worst fractions of the bars over the six shapes u 1.7e-4, n 2.2e-4, right-hand side
2.9e-3, obj 0.16, primal 3.0e-6, complementarity 6.4e-3, stationarity 0.084; the closed loop checks 200 of 200 plans, worst 0.75 of the bar,
0 path points in occupied cells with the rows on against 104 with them off."""
import ctypes as C
import math

import numpy as np
import pytest

import kmpc_qp_walls_ref as KW
import stmpc_qp_ref as SQ
import stmpc_qp_walls_ref as W
import stmpc_qp_walls_scenes as SC
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._rivals import Rivals
from f1tenth_planning_amd.runtime import (Context, F1PError, kmpc_qp_walls, rivals, stmpc_qp_avoid, stmpc_qp_set_avoid, stmpc_qp_set_walls,
                                          stmpc_qp_walls, stmpc_set_obstacles)

pytestmark = pytest.mark.gpu

WALLS = _abi.kmpc_qp_walls(n_samples=SC.N_SAMPLES)
OUT_KEYS = ("steer", "speed", "status", "u", "x", "obj", "duals", "iters", "eps", "planes", "avoid_duals")
ALL = dict(want_x=True, want_duals=True, want_planes=True, want_avoid_duals=True)
HORIZONS = (2, 24, SC.B(), SC.CAP)                               # both launch paths and the cap


def _set_grid(c):
    c.set_grid(SC.grid_image(), SC.RES, SC.ORIGIN, 128)


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        _set_grid(c)
        yield c


def _cfg(T):
    return _abi.stmpc_cfg(horizon=T)


def _shape(T):
    return T, dict(SC.shapes())[T] if T != 10 else 4


def _solve(ctx, T, M, sel=slice(None), walls=WALLS, **kw):
    x0, ref, oa, odv, obs, _ = SC.scene(T, M)
    return stmpc_qp_walls(ctx, x0[sel], ref[sel], obs[sel] if M else None, _cfg(T), walls=walls, oa_prev=oa[sel], od_v_prev=odv[sel], **ALL, **kw)


# ---- 1. planes and the exact optimum ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", SC.shapes())
def test_planes_and_exact_optimum(ctx, T, M):
    sols = SC.solutions(T, M)
    SC.assert_families(T, M, sols)
    assert not SC.edge_sensitive(sols) and SC.uncertified(sols) == 0
    assert np.array_equal(W.from_image(ctx.grid_debug_read(1)[0]), SC.grid_of()[0])       # the bitmap the kernel reads is the yardstick's grid
    out = _solve(ctx, T, M)
    print(f"T={T} M={M}: status {out['status'].tolist()} iters max {int(out['iters'].max())}")
    assert np.array_equal(out["status"], SC.expected_status(T, M)), out["status"]
    assert out["iters"].max() <= 50
    worst = dict(u=0.0, n=0.0, rhs=0.0, obj=0.0, primal=0.0, dual=0.0, comp=0.0, stat=0.0)
    for e, s in enumerate(sols):
        if s is None:                                          # status 1 / 3: NaN in every output
            for k in OUT_KEYS:
                if k not in ("status", "iters"):
                    assert np.isnan(out[k][e]).all(), (e, k)
            continue
        pl, ref_pl = out["planes"][e], s["planes"]
        assert np.array_equal(pl[:, :, 3], ref_pl[:, :, 3]), (e, SC.family_of(e), pl[:, :, 3], ref_pl[:, :, 3])
        worst["n"] = max(worst["n"], float(np.abs(pl[:, :, :2] - ref_pl[:, :, :2]).max()) / 1e-12)
        worst["rhs"] = max(worst["rhs"], float((np.abs(pl[:, :, 2] - ref_pl[:, :, 2]) / (1.0 + np.abs(ref_pl[:, :, 2]))).max()) / 1e-12)
        assert (np.abs(pl[:, :, :3] - ref_pl[:, :, :3]) <= 1e-12 * (1.0 + np.abs(ref_pl[:, :, :3]))).all(), (e, np.abs(pl - ref_pl).max())
        assert (pl[pl[:, :, 3] < 0][:, :3] == 0.0).all()
        b = s["build"]
        w = np.concatenate([out["u"][e].ravel(), [out["eps"][e]]])
        lam = W.lam_full(b, out["duals"][e], out["avoid_duals"][e])
        cert = W.cert(b, w, lam)
        rel = dict(cert); rel["comp"] /= 1.0 + lam.max()
        for k, bar in (("primal", 1e-9), ("dual", -1e-10), ("comp", 1e-9), ("stat", 1e-8)):
            worst[k] = max(worst[k], (min(rel[k], 0.0) if k == "dual" else rel[k]) / bar)
        assert W.cert_ok(cert, lam), (e, SC.family_of(e), cert)
        absent = np.setdiff1d(np.arange(2 * T), b["rows"])
        assert (out["avoid_duals"][e][absent] == 0.0).all()
        obj = 0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"]
        worst["obj"] = max(worst["obj"], abs(out["obj"][e] - obj) / (1.0 + abs(obj)) / 1e-10)
        assert abs(out["obj"][e] - obj) <= 1e-10 * (1.0 + abs(obj)), (e, out["obj"][e], obj)
        z = b["cond"]["Z"] @ out["u"][e].ravel() + b["cond"]["z0"]
        assert np.abs(out["x"][e] - z[:7 * (T + 1)].reshape(T + 1, 7).T).max() <= 1e-9
        bar = W.u_bar(b, w, lam, s["w"], s["lam"], s["degenerate"])
        d = float(np.abs(w - s["w"]).max())
        worst["u"] = max(worst["u"], d / bar)
        assert d <= bar, (e, SC.family_of(e), d, bar)
        assert abs(obj - s["obj"]) <= 1e-10 * (1.0 + abs(s["obj"])), (e, obj - s["obj"])
    print("  worst fractions of the bars:", {k: float(f"{v:.3g}") for k, v in worst.items()})


@pytest.mark.parametrize("n_samples", [1, 7, 8, 9, 256])
def test_ends_of_the_eight_sample_group(ctx, n_samples):
    """planes only, one ego of every family that has a solution, at T = 10: the march's group of eight ends before, at and after n_samples"""
    T, M = 10, 4
    x0, ref, oa, odv, obs, _ = SC.scene(T, M)
    sel = [e for e in range(len(SC.FAMILIES)) if SC.family_of(e) not in ("v0_out", "nan_state")]
    out = _solve(ctx, T, M, sel, walls=_abi.kmpc_qp_walls(n_samples=n_samples))
    assert np.isin(out["status"], (0, 2)).all()
    p, grid = SQ.default_params(T), SC.grid_of()
    slots = set()
    for i, e in enumerate(sel):
        b = W.build(x0[e], ref[e], oa[e], odv[e], obs[e], grid, p, n_samples)
        assert not b["edge"]
        assert np.array_equal(out["planes"][i][:, :, 3], b["planes"][:, :, 3]), (e, SC.family_of(e))
        assert (np.abs(out["planes"][i] - b["planes"]) <= 1e-12 * (1.0 + np.abs(b["planes"]))).all(), e
        slots |= set(b["planes"][:, :, 3].ravel().tolist())
    assert {float(W.SLOT_L), float(W.SLOT_R)} <= slots


# ---- 2. no candidate in reach ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 10, SC.CAP])
def test_no_candidate_is_the_plain_qp(ctx, T):
    x0, ref, oa, odv, _, fam = SC.scene(*_shape(T))
    sel = fam["no_wall"]
    got = stmpc_qp_walls(ctx, x0[sel], ref[sel], None, _cfg(T), walls=WALLS, oa_prev=oa[sel], od_v_prev=odv[sel], **ALL)
    plain = ctx.stmpc_qp(x0[sel], ref[sel], _cfg(T), oa_prev=oa[sel], od_v_prev=odv[sel])
    assert (got["status"] == 0).all() and (plain["status"] == 0).all()
    assert np.abs(got["u"] - plain["u"]).max() <= 2e-7 and np.abs(got["steer"] - plain["steer"]).max() <= 2e-7
    assert np.abs(got["eps"]).max() <= 1e-7 and (got["planes"][:, :, :, 3] == -1).all() and (got["planes"][:, :, :, :3] == 0).all()


def test_no_candidate_with_discs_is_the_avoidance_qp(ctx):
    T, M = 10, 4
    x0, ref, oa, odv, _, fam = SC.scene(T, M)
    sel = fam["no_wall"]
    p = SQ.default_params(T)
    obs = np.zeros((len(sel), M, 5))
    obs[:, :, 4] = -1.0
    for i, e in enumerate(sel):                                  # two discs beside the path, 0.1 and 0.3 m clear of it; the free region is 3.2 m wide
        path = SQ.predict_motion(x0[e], oa[e], odv[e], p)
        obs[i, 1] = SC._beside(path, 4, 0.35, 0.25)
        obs[i, 3] = SC._beside(path, 3, -0.6, 0.3)
    got = stmpc_qp_walls(ctx, x0[sel], ref[sel], obs, _cfg(T), walls=WALLS, oa_prev=oa[sel], od_v_prev=odv[sel], **ALL)
    want = stmpc_qp_avoid(ctx, x0[sel], ref[sel], obs, _cfg(T), oa_prev=oa[sel], od_v_prev=odv[sel], **ALL)
    assert (got["status"] == 0).all() and (want["status"] == 0).all()
    assert np.abs(got["u"] - want["u"]).max() <= 2e-7 and np.abs(got["eps"] - want["eps"]).max() <= 2e-7
    assert not np.isin(got["planes"][:, :, :, 3], (W.SLOT_L, W.SLOT_R)).any()
    assert np.array_equal(got["planes"], want["planes"]) and (want["planes"][:, :, :, 3] >= 0).all()


# ---- 3. neighbour independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", HORIZONS)
def test_neighbour_independence(ctx, T):
    """an ego alone equals the same ego inside the batch and inside the shuffled batch, bit for bit"""
    T, M = _shape(T)
    E = SC.n_egos(T)
    full = _solve(ctx, T, M)
    perm = np.random.default_rng(5).permutation(E)
    shuf = _solve(ctx, T, M, perm)
    for k in OUT_KEYS:
        assert np.array_equal(shuf[k], full[k][perm], equal_nan=True), k
    for e in range(len(SC.FAMILIES)):                            # one of every family, alone
        one = _solve(ctx, T, M, slice(e, e + 1))
        for k in OUT_KEYS:
            assert np.array_equal(one[k][0], full[k][e], equal_nan=True), (e, k)
    assert np.isin(full["planes"][:, :, :, 3], (W.SLOT_L, W.SLOT_R)).any()


# ---- 4. _dev against _batch, errors -----------------------------------------------------------------------------------------------------
def _dev_call(ctx, E, T, M=0, walls=WALLS, avoid=None, obs=True, cfg=None, inputs=None):
    """f1p_stmpc_qp_walls_dev on device buffers; inputs: None (scratch contents: the calls under test launch nothing, only the three
    required outputs are handed over) or (x0, ref, oa, odv, obs) -> every output"""
    sizes = dict(x0=56 * E, ref=56 * E * (T + 1), oa=8 * E * T, odv=8 * E * T, obs=40 * E * max(M, 1), steer=8 * E, speed=8 * E, status=4 * E,
                 u=16 * E * T, x=56 * E * (T + 1), obj=8 * E, duals=8 * E * (10 * T - 2), iters=4 * E, eps=8 * E, planes=64 * E * T,
                 avoid_duals=8 * E * (2 * T + 1))
    b = {k: ctx.alloc(max(n, 8)) for k, n in sizes.items()}
    try:
        if inputs is not None:
            for k, a in zip(("x0", "ref", "oa", "odv", "obs"), inputs):
                if a is not None and a.size:
                    b[k].upload(np.ascontiguousarray(a, np.float64))
        opt = (lambda k: b[k].ptr) if inputs is not None else (lambda k: None)
        rc = ctx.lib.f1p_stmpc_qp_walls_dev(ctx.h, b["x0"].ptr, b["ref"].ptr, opt("oa"), opt("odv"), E, C.byref(cfg or _cfg(T)), None,
                                            b["obs"].ptr if obs else None, M, None if avoid is None else C.byref(avoid),
                                            None if walls is None else C.byref(walls), b["steer"].ptr, b["speed"].ptr, b["status"].ptr,
                                            opt("u"), opt("x"), opt("obj"), opt("duals"), opt("iters"), opt("eps"), opt("planes"),
                                            opt("avoid_duals"))
        ctx._check(rc)
        ctx.sync()
        if inputs is None:
            return None
        shp = dict(steer=(E,), speed=(E,), status=(E,), u=(E, T, 2), x=(E, 7, T + 1), obj=(E,), duals=(E, 10 * T - 2), iters=(E,), eps=(E,),
                   planes=(E, T, 2, 4), avoid_duals=(E, 2 * T + 1))
        return {k: b[k].download(np.int32 if k in ("status", "iters") else np.float64, s) for k, s in shp.items()}
    finally:
        ctx.sync()
        for v in b.values():
            v.free()


@pytest.mark.parametrize("T", [10, SC.CAP])
def test_dev_equals_batch(ctx, T):
    T, M = _shape(T)
    x0, ref, oa, odv, obs, _ = SC.scene(T, M)
    want = _solve(ctx, T, M)
    got = _dev_call(ctx, len(x0), T, M, inputs=(x0, ref, oa, odv, obs))
    for k in OUT_KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


_LX = np.arange(SC.wx(4) + 0.05, SC.wx(60), 0.05)
_LINE = np.column_stack([_LX, np.full_like(_LX, SC.wy(30) + 0.7), np.full_like(_LX, 3.0), np.zeros_like(_LX)])   # 0.1 m inside the left wall
_V = np.array([3.0, 1.0, 2.6, 1.9, 2.0, 4.0, 0.8, 2.2, 1.5])   # either side of V_KS, in no order


def _line_states(n):
    rng = np.random.default_rng(11)
    return np.column_stack([SC.wx(6) + rng.uniform(0.0, 3.0, n), SC.wy(30) + rng.uniform(-0.3, 0.3, n), rng.normal(0.0, 0.02, n), _V[:n],
                            rng.normal(0.0, 0.05, n), rng.normal(0.0, 0.05, n), rng.normal(0.0, 0.01, n)])


def test_errors(ctx):
    x0, ref, oa, odv, obs, _ = SC.scene(10, 4)
    cfg = _cfg(10)
    lib = ctx.lib
    T1 = SC.CAP + 1
    # NULLs
    assert lib.f1p_stmpc_qp_set_walls(None, C.byref(WALLS)) == _abi.F1P_EINVAL
    nothing = [None] * 5 + [0] + [None] * 3 + [0] + [None] * 13
    assert lib.f1p_stmpc_qp_walls_batch(*nothing) == _abi.F1P_EINVAL and lib.f1p_stmpc_qp_walls_dev(*nothing) == _abi.F1P_EINVAL
    st, sp, su = np.empty(2), np.empty(2), np.empty(2, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    tail = [None] * 8
    for args in ([None, ptr(ref), None, None, 2, C.byref(cfg), None, None, 0, None, None, ptr(st), ptr(sp), ptr(su)],      # x0
                 [ptr(x0), None, None, None, 2, C.byref(cfg), None, None, 0, None, None, ptr(st), ptr(sp), ptr(su)],       # ref
                 [ptr(x0), ptr(ref), None, None, 2, None, None, None, 0, None, None, ptr(st), ptr(sp), ptr(su)],          # cfg
                 [ptr(x0), ptr(ref), None, None, 2, C.byref(cfg), None, None, 2, None, None, ptr(st), ptr(sp), ptr(su)],   # obs with M = 2
                 [ptr(x0), ptr(ref), None, None, 2, C.byref(cfg), None, None, 0, None, None, None, ptr(sp), ptr(su)]):     # steer
        assert lib.f1p_stmpc_qp_walls_batch(ctx.h, *args, *tail) == _abi.F1P_EINVAL
    with pytest.raises(ValueError, match="stmpc qp walls: obs is NULL"):
        _dev_call(ctx, 2, 10, M=2, obs=False)
    # the numbers
    for bad in (dict(n_samples=0), dict(n_samples=257), dict(n_samples=-1), dict(margin=np.inf), dict(margin=np.nan)):
        w = _abi.kmpc_qp_walls(**bad)
        with pytest.raises(ValueError, match="stmpc qp walls: n_samples must be in"):
            stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=w)
        with pytest.raises(ValueError, match="stmpc qp walls: n_samples must be in"):
            _dev_call(ctx, 2, 10, walls=w)
        with pytest.raises(ValueError, match="stmpc qp walls: n_samples must be in"):
            stmpc_qp_set_walls(ctx, w)
    stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=_abi.kmpc_qp_walls(n_samples=256, margin=-0.1))      # the ends of the range
    stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=_abi.kmpc_qp_walls(n_samples=1))
    stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=None)                                                  # the defaults
    with pytest.raises(ValueError):                            # the disc rows' numbers are checked as before
        stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, avoid=_abi.kmpc_qp_avoid(rho=0.0))
    # horizon 41, M = 17
    with pytest.raises(ValueError, match="F1P_STMPC_QP_AVOID_MAX_T"):
        stmpc_qp_walls(ctx, x0[:1], np.zeros((1, 7, T1 + 1)), None, _cfg(T1), walls=WALLS)
    with pytest.raises(ValueError, match="F1P_STMPC_QP_AVOID_MAX_T"):
        _dev_call(ctx, 1, T1)
    with pytest.raises(ValueError, match=r"stmpc qp walls: M must be in \[0, 16\]"):
        stmpc_qp_walls(ctx, x0[:2], ref[:2], np.zeros((2, 17, 5)), cfg, walls=WALLS)
    with pytest.raises(ValueError, match=r"stmpc qp walls: M must be in \[0, 16\]"):
        _dev_call(ctx, 2, 10, M=17)
    # the plan path: the switch, the caps with walls alone, the E mismatch of the held obstacles, off-after-on
    ctx.set_waypoints(_LINE, cols=(0, 1, 2, 3))
    kcfg = _abi.kmpc_cfg(horizon=8)
    xs = _line_states(8)
    ctx.stmpc_qp_warm_reset()
    plain = ctx.stmpc_qp_plan(xs, cfg, kcfg)
    stmpc_set_obstacles(ctx, obs[:4])
    stmpc_qp_set_walls(ctx, WALLS)
    try:
        ctx.stmpc_qp_warm_reset()
        on = ctx.stmpc_qp_plan(xs, cfg, kcfg)                     # set_avoid off: the held discs (for 4 egos) are not taken, no error
        assert np.isin(on["status"], (0, 2)).all() and set(on["branch"].tolist()) == {0, 1}
        for b in (0, 1):
            assert (on["steer"][on["branch"] == b] != plain["steer"][on["branch"] == b]).any(), b
        with pytest.raises(ValueError, match="F1P_STMPC_QP_AVOID_MAX_T"):
            ctx.stmpc_qp_plan(xs[:4], _cfg(T1), kcfg)
        with pytest.raises(ValueError, match="kinematic branch"):
            ctx.stmpc_qp_plan(xs[:4], _cfg(SC.CAP), _abi.kmpc_cfg(horizon=32))
        stmpc_qp_set_avoid(ctx, _abi.kmpc_qp_avoid())
        with pytest.raises(F1PError, match="obstacles were set for 4 egos, this plan has 8"):
            ctx.stmpc_qp_plan(xs, cfg, kcfg)
        stmpc_set_obstacles(ctx, None)
        stmpc_qp_set_avoid(ctx, None)
        # no grid, a footprint
        try:
            ctx.set_footprint((0.0, 0.2), 0.1)
            for call in (lambda: stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=WALLS), lambda: _dev_call(ctx, 2, 10),
                         lambda: ctx.stmpc_qp_plan(xs, cfg, kcfg)):
                with pytest.raises(F1PError, match=r"stmpc qp walls are a point / disc test: remove the oriented footprint \(f1p_set_footprint\)"):
                    call()
            ctx.set_footprint((), 0.0)
            ctx.set_grid(None, 0.0, (0.0, 0.0), 0)
            for call in (lambda: stmpc_qp_walls(ctx, x0[:2], ref[:2], None, cfg, walls=WALLS), lambda: _dev_call(ctx, 2, 10),
                         lambda: ctx.stmpc_qp_plan(xs, cfg, kcfg)):
                with pytest.raises(F1PError, match=r"stmpc qp walls are on but no occupancy grid is loaded \(f1p_set_grid\)"):
                    call()
        finally:
            _set_grid(ctx)
            ctx.set_footprint((), 0.0)
        # off after on: the parent's behaviour, bit for bit
        stmpc_qp_set_walls(ctx, _abi.kmpc_qp_walls(on=False))
        ctx.stmpc_qp_warm_reset()
        again = ctx.stmpc_qp_plan(xs, cfg, kcfg)
        for k in ("steer", "speed", "status", "branch", "u", "obj"):
            assert np.array_equal(again[k], plain[k], equal_nan=True), k
        ctx.stmpc_qp_plan(xs[:4], _cfg(T1), kcfg)                 # ... the plain kernel's own cap (44) holds again
    finally:
        stmpc_set_obstacles(ctx, None)
        stmpc_qp_set_avoid(ctx, None)
        stmpc_qp_set_walls(ctx, None)
        ctx.stmpc_qp_warm_reset()


# ---- 5. the plan path in both branches, and grid changes ----------------------------------------------------------------------------------
def _stateless(ctx, xs, branch, ids, T, TK, wl, obs=None, av=None):
    """every ego through the stateless wall call of its own branch, from a zero previous solution"""
    E = len(xs)
    out = dict(steer=np.full(E, np.nan), speed=np.full(E, np.nan), status=np.full(E, -1, np.int32), obj=np.full(E, np.nan), eps=np.full(E, np.nan))
    d, k = np.flatnonzero(branch == 1), np.flatnonzero(branch == 0)
    s4 = np.ascontiguousarray(xs[:, [0, 1, 3, 4]])
    ref_of = (lambda sel, T_, dt: ctx.stmpc_ref(s4[sel], T_, dt, 0.03)) if ids is None else \
             (lambda sel, T_, dt: ctx.stmpc_ref_tracks(s4[sel], ids[sel], T_, dt, 0.03))
    refs = {}
    if len(d):
        refs[1] = ref_of(d, T, 0.025)
        o = stmpc_qp_walls(ctx, xs[d], refs[1], None if obs is None else obs[d], _cfg(T), avoid=av, walls=wl, want_planes=True)
        out["planes_dyn"] = o["planes"]
        for key in ("steer", "speed", "status", "obj", "eps"):
            out[key][d] = o[key]
    if len(k):
        ref4 = np.ascontiguousarray(ref_of(k, TK, 0.1)[:, [0, 1, 3, 4]])
        o = kmpc_qp_walls(ctx, s4[k], ref4, None if obs is None else obs[k], _abi.kmpc_cfg(horizon=TK), avoid=av, walls=wl)
        for key in ("steer", "speed", "status", "obj", "eps"):
            out[key][k] = o[key]
    return out, refs


@pytest.mark.parametrize("tracks", [False, True])
def test_plan_path_both_branches_and_grid_changes(ctx, tracks):
    """f1p_stmpc_qp_plan_batch / _plan_tracks_batch under set_walls: every ego equals the stateless wall call of its own branch -- the
    kinematic ones f1p_kmpc_qp_walls_batch -- before and after the grid is inflated; the dynamic planes are the yardstick's on the bitmap in
    force at that call"""
    T, TK = 10, 8
    xs = _line_states(9)
    wl = _abi.kmpc_qp_walls(n_samples=SC.N_SAMPLES, margin=0.05)
    ctx.set_waypoints(_LINE, cols=(0, 1, 2, 3))
    ids = None
    if tracks:
        other = _LINE.copy(); other[:, 1] -= 1.45
        ctx.set_tracks([_LINE, other], cols=(0, 1, 2, 3))
        ids = (np.arange(len(xs)) % 2).astype(np.int32)
    stmpc_qp_set_walls(ctx, wl)
    p = SQ.default_params(T)
    try:
        rhs = []
        for step in range(2):
            if step == 1:
                ctx.inflate_grid(0.2)
            ctx.stmpc_qp_warm_reset()
            got = ctx.stmpc_qp_plan_tracks(xs, ids, _cfg(T), _abi.kmpc_cfg(horizon=TK)) if tracks else ctx.stmpc_qp_plan(xs, _cfg(T), _abi.kmpc_cfg(horizon=TK))
            assert np.array_equal(got["branch"], (xs[:, 3] > 2.0).astype(np.int32)) and 3 <= got["branch"].sum() <= len(xs) - 3
            want, refs = _stateless(ctx, xs, got["branch"], ids, T, TK, wl)
            assert np.isin(want["status"], (0, 2)).all(), want["status"]
            for key in ("steer", "speed", "status", "obj"):
                assert np.array_equal(got[key], want[key]), (step, key, got[key], want[key])
            grid = SC.grid_of(ctx.grid_debug_read(1)[0])
            for i, e in enumerate(np.flatnonzero(got["branch"] == 1)):
                b = W.build(xs[e], refs[1][i], np.zeros(T), np.zeros(T), None, grid, p, SC.N_SAMPLES, wall_margin=0.05)
                assert not b["edge"]
                assert np.array_equal(want["planes_dyn"][i][:, :, 3], b["planes"][:, :, 3]), (step, e)
                assert (np.abs(want["planes_dyn"][i] - b["planes"]) <= 1e-12 * (1.0 + np.abs(b["planes"]))).all(), (step, e)
            rhs.append(want["planes_dyn"][:, :, :, 2].copy())
        assert (np.abs(rhs[1] - rhs[0]) > 0.1).any()              # 0.2 m of inflation moved the contacts
        assert SC.grid_of(ctx.grid_debug_read(1)[0])[0].sum() > SC.grid_of()[0].sum()
    finally:
        ctx.inflate_grid(0.0)
        stmpc_qp_set_walls(ctx, None)
        ctx.stmpc_qp_warm_reset()
        if tracks:
            ctx.set_tracks([])


# ---- 6. track sets and rivals ----------------------------------------------------------------------------------------------------------
def _corridor_planner(**kw):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True, QP_WALL_REACH=1.0, T=10, TK=8, **kw))
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN)
    return pl


def _course(lat):
    return [_LX.copy(), np.full_like(_LX, SC.wy(30) + lat), np.zeros_like(_LX), np.full_like(_LX, 3.0)]


def test_track_sets_equal_per_track_planners():
    xs = _line_states(8)
    ids = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    tracks = [_course(0.7), _course(-0.75)]
    both, free = _corridor_planner(), _corridor_planner()
    free.config.QP_WALLS_ST = False
    for step in range(2):                                        # the second call linearises about the first one's solution
        got = both.plan_batch(xs, tracks=tracks, track_ids=ids)
        off = free.plan_batch(xs, tracks=tracks, track_ids=ids)
        if step == 0:
            singles = [_corridor_planner(), _corridor_planner()]
        for k in (0, 1):
            sel = np.flatnonzero(ids == k)
            want = singles[k].plan_batch(xs[sel], waypoints=tracks[k])
            for key in ("steer", "speed", "status", "branch", "u", "obj"):
                assert np.array_equal(got[key][sel], want[key], equal_nan=True), (step, k, key)
        assert np.isin(got["status"], (0, 2)).all() and set(got["branch"].tolist()) == {0, 1}
        assert (got["steer"] != off["steer"]).any()              # the rows matter in this scene


def test_rivals_equal_the_same_slots_as_obstacles(ctx):
    n = 6
    # (0.08 and 0.27 m from the left wall and heading into it: the straight path of a first plan crosses it, the wall rows bind)
    xs = np.column_stack([SC.wx(8) + 0.6 * np.arange(n), SC.wy(30) + np.where(np.arange(n) % 2 == 0, 0.52, 0.33), np.zeros(n), np.linspace(3.5, 1.0, n),
                          np.full(n, 0.2), np.zeros(n), np.zeros(n)])
    a, b, no_walls = _corridor_planner(QP_AVOID=True), _corridor_planner(QP_AVOID=True), _corridor_planner(QP_AVOID=True)
    no_walls.config.QP_WALLS_ST = False
    a.rivals = Rivals(count=2, radius=0.3)
    slots = rivals(ctx, xs, "st7", 2, 0.3)
    assert (slots["idx"] >= 0).all()
    got = a.plan_batch(xs, waypoints=_course(0.7))
    b.obstacles = slots["obs"]
    want = b.plan_batch(xs, waypoints=_course(0.7))
    no_walls.obstacles = slots["obs"]
    off = no_walls.plan_batch(xs, waypoints=_course(0.7))
    for key in ("steer", "speed", "status", "branch", "u"):
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert np.isin(got["status"], (0, 2)).all() and set(got["branch"].tolist()) == {0, 1} and (got["steer"] != off["steer"]).any()
    # the single-vehicle call takes the walls too
    one = _corridor_planner()
    steer, speed = one.plan(xs[0], waypoints=_course(0.7))
    ref = one._ctx.stmpc_ref(xs[:1, [0, 1, 3, 4]], 10, 0.025, 0.03)
    full = stmpc_qp_walls(one._ctx, xs[:1], ref, None, _cfg(10), walls=_abi.kmpc_qp_walls(n_samples=20))
    assert (steer, speed) == (float(full["steer"][0]), float(full["speed"][0])) and math.isfinite(steer)


# ---- 7. the class in closed loop -------------------------------------------------------------------------------------------------------
def _closed_loop(walls, check):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    L = SC.LOOP
    T, TK = L["T"], L["TK"]
    img, res, origin, wp = SC.band_track()
    c = mpc_config(SOLVER="qp", QP_WALLS_ST=walls, QP_WALL_REACH=L["reach"], QP_WALL_MARGIN=L["margin"], T=T, TK=TK)
    planner = STMPCPlanner(waypoints=wp, config=c)
    planner.set_map(img, res, origin, inflate=L["inflate"])
    p, pk = SQ.default_params(T), SQ.kin_params(TK)
    s = SC.loop_start()
    E = len(s)
    steps, inside, checked, worst, grid, n_st2, n_dyn = L["steps"], 0, 0, 0.0, None, 0, 0
    prev = [None] * E                                            # per ego (oa, odv) of the GPU's last plan, by the reference's reset rules
    for step in range(steps):
        out = planner.plan_batch(s)
        ctx = planner._ctx
        if grid is None:
            grid = (W.from_image(ctx.grid_debug_read(1)[0]), res, origin)
            assert np.array_equal(grid[0], SC.band_grid_inflated()[0])
        inside += sum(W.occupied(grid, s[e, 0], s[e, 1]) for e in range(E))
        assert np.isin(out["status"], (0, 2)).all() and (walls or (out["status"] == 0).all())
        n_st2 += int((out["status"] == 2).sum())
        n_dyn += int(out["branch"].sum())
        for e in range(E):
            dyn = bool(out["branch"][e])
            n = T if dyn else TK
            if check:
                s4 = s[e:e + 1, [0, 1, 3, 4]]
                pv = prev[e]
                if dyn:                                          # reset when len(oa) < T
                    pv = None if pv is None or len(pv[0]) < T else (pv[0][:T], pv[1][:T])
                    sol = SC.loop_check(s[e], ctx.stmpc_ref(s4, T, 0.025, 0.03)[0], pv, grid, True, T)
                    ok = sol["certified"] and not sol["edge"]
                    du = float(np.abs(out["u"][e, :T] - sol["u"][:, ::-1]).max())      # the plan's u is (oa, odelta_v), the QP's (steer_v, accel)
                else:                                            # reset when len(oa) > TK
                    pv = (np.zeros(TK), np.zeros(TK)) if pv is None or len(pv[0]) > TK else pv
                    ref4 = ctx.stmpc_ref(s4, TK, 0.1, 0.03)[0][[0, 1, 3, 4]]
                    sol = KW.solve(s4[0], ref4, pv[0], pv[1], None, grid, pk, L["n_samples"], wall_margin=L["margin"])
                    ok = KW.cert_ok(sol["cert"]) and not sol["edge"]
                    du = float(np.abs(out["u"][e, :TK] - sol["u"]).max())
                if ok:
                    bar = 1e-5 if sol["degenerate"] else 1e-7
                    dd = max(du, abs(out["steer"][e] - sol["steer"]), abs(out["speed"][e] - sol["speed"]))
                    assert dd <= bar, (step, e, dyn, dd, bar)
                    worst = max(worst, dd / bar)
                    checked += 1
            prev[e] = (out["u"][e, :n, 0].copy(), out["u"][e, :n, 1].copy())
        s = np.array([SQ.plant(s[e], out["steer"][e], out["speed"][e], p) for e in range(E)])
    return inside, checked, worst, steps * E, n_st2, n_dyn


def test_class_closed_loop_beside_a_wall():
    inside_on, checked, worst, plans, n_st2, n_dyn = _closed_loop(True, True)
    inside_off, _, _, _, _, _ = _closed_loop(False, False)
    print(f"path points in occupied active cells: QP_WALLS_ST on {inside_on}, off {inside_off} (of {plans}); checked {checked} of {plans}, "
          f"worst diff / bar {worst:.3g}, plans of status 2: {n_st2}, dynamic-branch plans {n_dyn}")
    assert checked >= 0.95 * plans
    assert n_st2 <= 0.05 * plans
    assert n_dyn >= 0.9 * plans                                  # the loop is the dynamic branch's
    assert inside_on < inside_off
