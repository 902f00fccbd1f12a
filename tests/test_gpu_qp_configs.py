"""f1p_kmpc_qp_* and f1p_stmpc_qp_* OFF the defaults of mpc_config: seeded sweeps over weights (Q != Qf, R != Rd, zero entries), bounds,
time steps, vehicle parameters and the horizons at which the kernels take another path (tests/qp_cases.py; the yardsticks are pinned to
the reference off its defaults by tests/test_qp_configs_host.py), the two packings of the short-horizon kinematic kernel, the solver
options (max_iter, tol, their range checks) and both planner classes with a non-default QP config.  Every ego of the sweeps is held to
the KKT certificate built from the device's own u and duals on the yardstick's condensed problem."""
import numpy as np
import pytest

import kmpc_qp_ref as KQ
import qp_cases as QC
import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.runtime import Context

pytestmark = pytest.mark.gpu

KEYS_K = ("steer", "speed", "status", "u", "xk", "obj", "duals", "iters")
KEYS_S = ("steer", "speed", "status", "u", "x", "obj", "duals", "iters")


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        c.set_waypoints(QC.track())
        yield c


def _kref(ctx):
    return lambda x4, T, dt: ctx.kmpc_ref(x4, T, dt, QC.DL)


def _sref(ctx):
    return lambda x4, T, dt: ctx.stmpc_ref(x4, T, dt, QC.DL)


def _kfam(T):
    return {"accel": slice(0, 2 * T), "steer": slice(2 * T, 4 * T), "rate": slice(4 * T, 6 * T - 2), "v_upper": slice(6 * T - 2, 7 * T - 2),
            "v_lower": slice(7 * T - 2, 8 * T - 2)}


def _sfam(T):
    return {"rate": slice(0, 2 * T - 2), "steer": slice(2 * T - 2, 4 * T - 2), "speed": slice(4 * T - 2, 6 * T - 2),
            "steer_v": slice(6 * T - 2, 8 * T - 2), "accel": slice(8 * T - 2, 10 * T - 2)}


def _cert(c, u, lam, relative_comp):
    cert = SQ.cond_cert(c, u, lam)
    if relative_comp:
        cert["comp"] /= 1.0 + lam.max()          # relative to the multipliers' scale, as test_gpu_stmpc_qp.test_scale_certificates
    return cert


def _fobj(c, u):
    return 0.5 * u @ c["H"] @ u + c["g"] @ u + c["c"]


def _u_bar(c, u, lam, us, lam_s, deg):
    """test_gpu_stmpc_qp._u_bar: 1e-7 (1e-5 degenerate), or the distance the two points' own KKT residuals allow where the objective
    is weakly curved"""
    H, g, G, h = c["H"], c["g"], c["G"], c["h"]
    mu = np.linalg.eigvalsh(H).min()
    dr = np.linalg.norm((H @ u + g + G.T @ lam) - (H @ us + g + G.T @ lam_s))
    gap = np.abs(lam * (h - G @ u)).sum() + np.abs(lam_s * (h - G @ us)).sum()
    return max(1e-5 if deg else 1e-7, 2.0 * (dr + np.sqrt(dr * dr + 4.0 * mu * gap)) / (2.0 * mu))


def _exact(c, lam_dev, T, own_guess):
    """the exact optimum where the helper certifies one: the active-set polish from the device's duals (a passing point IS the optimum,
    whatever produced the guess); failing that, the helper from its own guess -- with its SLSQP fallback below T = 20 only, and at
    the long horizons on the first four cases only (own_guess)"""
    try:
        r = SQ.polish(c, lam_dev)
        if r is None and own_guess:
            if T < 20:
                u, lam, deg = SQ.exact(c)
                r = (u, lam, deg) if SQ.exact_ok(c, u, lam) else None
            else:
                r = SQ.polish(c, SQ.ipm_hint(c))
    except np.linalg.LinAlgError:
        r = None
    return r


# ---- 1. the sweeps ------------------------------------------------------------------------------------------------------------------
_SWEEP = {}


def _sweep(ctx, kind, T):
    """run one horizon's cases once (cached: the per-horizon tests and the coverage test share it) -> one record per ego"""
    if (kind, T) in _SWEEP:
        return _SWEEP[(kind, T)]
    km = kind == "kmpc"
    recs = []
    for seed in (QC.KMPC_SEEDS if km else QC.STMPC_SEEDS):
        cfg, p = (QC.kmpc_case if km else QC.stmpc_case)(seed, T)
        E = QC.n_egos(seed)
        own_guess = T < (QC.KMPC_LONG if km else QC.STMPC_LONG) or seed in QC.LONG_SEEDS
        if km:
            x0, ref, oa, od = QC.kmpc_inputs(seed, p, E, _kref(ctx))
            out = ctx.kmpc_qp(x0, ref, cfg, oa_prev=oa, od_prev=od, want_xk=True, want_duals=True)
            xs, fam, nx = out["xk"], _kfam(T), 4
        else:
            x0, ref, oa, od = QC.stmpc_inputs(seed, p, E, _sref(ctx))
            out = ctx.stmpc_qp(x0, ref, cfg, oa_prev=oa, od_v_prev=od, want_x=True, want_duals=True)
            xs, fam, nx = out["x"], _sfam(T), 7
        for e in range(E):
            r = dict(seed=seed, e=e, status=int(out["status"][e]), iters=int(out["iters"][e]))
            recs.append(r)
            if r["status"] != 0:
                continue
            c = (KQ.condense(KQ.qp_data(x0[e], ref[e], oa[e], od[e], p), T) if km else
                 SQ.condense(SQ.qp_data(x0[e], ref[e], oa[e], od[e], p), T))
            u, lam = out["u"][e].ravel(), out["duals"][e]
            r["cert"] = _cert(c, u, lam, relative_comp=not km)
            f = _fobj(c, u)
            r["obj_err"] = abs(out["obj"][e] - f) / (1.0 + abs(f))
            z = c["Z"] @ u + c["z0"]
            r["x_err"] = np.abs(xs[e] - z[:nx * (T + 1)].reshape(T + 1, nx).T).max() / (1.0 + np.abs(z).max())
            r["binds"] = {k: bool((lam[s] > 1e-6).any()) for k, s in fam.items()}
            ex = _exact(c, lam, T, own_guess)
            r["exact"] = ex is not None
            r["tried"] = own_guess
            if ex is not None:
                us, lam_s, deg = ex
                r["u_err"] = float(np.abs(u - us).max())
                r["u_bar"] = (1e-5 if deg else 1e-7) if km else _u_bar(c, u, lam, us, lam_s, deg)
                r["f_err"] = abs(_fobj(c, u) - _fobj(c, us)) / (1.0 + abs(_fobj(c, us)))
                r["allowed"] = _u_bar(c, u, lam, us, lam_s, deg)
                r["mu"], r["deg"] = float(np.linalg.eigvalsh(c["H"]).min()), deg
    _SWEEP[(kind, T)] = recs
    return recs


def _check_sweep(kind, T, recs):
    ok = [r for r in recs if r["status"] == 0]
    tried = [r for r in ok if r["tried"]]
    missed = sum(not r["exact"] for r in tried)
    print(kind, T, "egos", len(recs), "status", sorted({r["status"] for r in recs}), "iters max", max(r["iters"] for r in recs),
          "stat max %.2e comp max %.2e primal max %.2e" % tuple(max(r["cert"][k] for r in ok) for k in ("stat", "comp", "primal")),
          "obj %.2e x %.2e" % (max(r["obj_err"] for r in ok), max(r["x_err"] for r in ok)),
          "exact", sum(r["exact"] for r in ok), "missed", missed, "of", len(tried),
          "u_err max %.2e" % max([r["u_err"] for r in ok if r["exact"]] or [0.0]))
    for r in ok:
        if r["exact"] and r["u_err"] > r["u_bar"]:
            print("   over the bar:", r["seed"], r["e"], "u_err %.3e bar %.1e allowed %.3e mu %.3e f_err %.2e deg %s iters %d" %
                  (r["u_err"], r["u_bar"], r["allowed"], r["mu"], r["f_err"], r["deg"], r["iters"]), r["cert"])
    bad = [(r["seed"], r["e"], r["status"]) for r in recs if r["status"] != 0]
    assert not bad, bad
    for r in recs:
        tag = (kind, T, r["seed"], r["e"])
        assert SQ.cert_ok(r["cert"]), (tag, r["cert"])
        assert r["obj_err"] <= 1e-10, (tag, r["obj_err"])
        # the device's states against Z u + z0: the bar the recorded problems' certificates put on the model equalities (primal 1e-9),
        # relative to the largest entry
        assert r["x_err"] <= 1e-9, (tag, r["x_err"])
        if r["exact"] and kind == "stmpc":
            assert r["u_err"] <= r["u_bar"], (tag, r["u_err"], r["u_bar"])
    if not (kind == "stmpc" and T == 44):        # T = 44 of the dynamic QP: the certificate alone decides (the helper settles on half)
        assert 4 * missed <= len(tried), (missed, len(tried))


@pytest.mark.parametrize("T", QC.KMPC_HORIZONS)
def test_kmpc_sweep(ctx, T):
    """24 configs per horizon, 8..32 egos each: status 0, the KKT certificate, obj, xk and -- where the helper certifies an exact
    optimum -- u, at the bars of test_gpu_kmpc_qp.  T = 2, 3 (rows that exist only for tau < T - 1), 7 | 8 | 9 (k_kmpc_qp<16> | <64>),
    16, 24 | 25 (8 * qp_lds_doubles(T) crosses sharedMemPerBlock: the launch opts in to large LDS), 31, 32 (every lane owns an input)."""
    _check_sweep("kmpc", T, _sweep(ctx, "kmpc", T))


@pytest.mark.parametrize("T", QC.KMPC_HORIZONS)
def test_kmpc_sweep_u_against_the_exact_optimum(ctx, T):
    """Where the helper certifies an exact optimum, u against it at the bars of test_gpu_kmpc_qp: 1e-7, 1e-5 at a degenerate optimum.
    This is the test of qp_ipm.h's refinement step: with the stopping rule alone 11 of the 3583 compared egos were over the bar
    (1.3e-5 .. 2.1e-5 at degenerate optima at T = 8, 16, 31; 1.3e-7 and 1.9e-7 at T = 25, 32) while passing the certificate; with
    the step the largest distance at a degenerate optimum is 7.9e-6."""
    recs = [r for r in _sweep(ctx, "kmpc", T) if r.get("exact")]
    assert len(recs) >= 300
    over = [(r["seed"], r["e"], r["u_err"], r["u_bar"]) for r in recs if r["u_err"] > r["u_bar"]]
    print("kmpc", T, "compared", len(recs), "over the bar", over)
    assert not over, over


@pytest.mark.parametrize("T", QC.STMPC_HORIZONS)
def test_stmpc_sweep(ctx, T):
    """16 configs per horizon with all seven entries of Q and Qf positive, 8..32 egos each, at the bars of test_gpu_stmpc_qp.  T = 2, 3,
    10, 28 | 29 (8 * stqp_lds_doubles(T) crosses sharedMemPerBlock), 43, 44 = F1P_STMPC_QP_MAX_T."""
    _check_sweep("stmpc", T, _sweep(ctx, "stmpc", T))


def test_every_constraint_family_binds_in_the_sweeps(ctx):
    for kind, hs in (("kmpc", QC.KMPC_HORIZONS), ("stmpc", QC.STMPC_HORIZONS)):
        n = {}
        for T in hs:
            for r in _sweep(ctx, kind, T):
                for k, b in r.get("binds", {}).items():
                    n[k] = n.get(k, 0) + b
        print(kind, n)
        assert n and all(v > 0 for v in n.values()), (kind, n)


def test_horizons_past_the_limit_raise(ctx):
    cfg, p = QC.kmpc_case(0, 33)
    x0 = QC.kmpc_inputs(0, QC.kmpc_case(0, 8)[1], 1, _kref(ctx))[0]
    with pytest.raises(ValueError, match="horizon must be <= 32"):
        ctx.kmpc_qp(x0, ctx.kmpc_ref(x0, 33, p["DTK"], QC.DL), cfg)
    cfg, p = QC.stmpc_case(0, 45)
    x0 = QC.stmpc_inputs(0, QC.stmpc_case(0, 10)[1], 1, _sref(ctx))[0]
    with pytest.raises(ValueError, match="horizon must be <= F1P_STMPC_QP_MAX_T"):
        ctx.stmpc_qp(x0, ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], 45, p["DT"], QC.DL), cfg)


# ---- 2. packing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 5, 8])
def test_packings_are_bit_identical(ctx, T):
    """one ego per wave (k_kmpc_qp<64>) against four (k_kmpc_qp<16>) against the default: every output, bit for bit.  Lanes beyond n hold
    zeros in every reduction, and the xor butterflies of width 64 add or compare them after the width-16 stages, exactly."""
    cfg, p = QC.kmpc_case(100 + T, T)
    x0, ref, oa, od = QC.kmpc_inputs(100 + T, p, 130, _kref(ctx))
    try:
        for E in (1, 2, 3, 4, 5, 63, 130):
            outs = {}
            for pack in (1, 4, 0):
                ctx.kmpc_qp_set_pack(pack)
                outs[pack] = ctx.kmpc_qp(x0[:E], ref[:E], cfg, oa_prev=oa[:E], od_prev=od[:E], want_xk=True, want_duals=True)
            assert (outs[1]["status"] == 0).all(), (E, outs[1]["status"])
            for k in KEYS_K:
                assert np.array_equal(outs[1][k], outs[4][k]), (T, E, k)
                assert np.array_equal(outs[0][k], outs[4][k]), (T, E, k)
    finally:
        ctx.kmpc_qp_set_pack(0)


def test_pack_is_ignored_past_eight_steps_and_bad_values_raise(ctx):
    cfg, p = QC.kmpc_case(109, 9)
    x0, ref, oa, od = QC.kmpc_inputs(109, p, 9, _kref(ctx))
    try:
        want = ctx.kmpc_qp(x0, ref, cfg, oa_prev=oa, od_prev=od, want_xk=True, want_duals=True)
        ctx.kmpc_qp_set_pack(4)
        got = ctx.kmpc_qp(x0, ref, cfg, oa_prev=oa, od_prev=od, want_xk=True, want_duals=True)
        assert (want["status"] == 0).all()
        for k in KEYS_K:
            assert np.array_equal(got[k], want[k]), k
        for bad in (-1, 2, 3, 5, 16, 64):
            with pytest.raises(ValueError, match="egos_per_wave must be 0, 1 or 4"):
                ctx.kmpc_qp_set_pack(bad)
    finally:
        ctx.kmpc_qp_set_pack(0)


# ---- 3. solver options ----------------------------------------------------------------------------------------------------------------
def _opts_case(ctx, kind):
    """(run(sel, opts) -> outputs of the egos sel, x0, cond(e) -> the yardstick's condensed problem, p, keys)"""
    if kind == "kmpc":
        cfg, p = QC.kmpc_case(201, 8)
        x0, ref, oa, od = QC.kmpc_inputs(201, p, 24, _kref(ctx))

        def run(sel, opts=None):
            return ctx.kmpc_qp(x0[sel], ref[sel], cfg, oa_prev=oa[sel], od_prev=od[sel], opts=opts, want_xk=True, want_duals=True)

        def cond(e):
            return KQ.condense(KQ.qp_data(x0[e], ref[e], oa[e], od[e], p), p["T"])
        return run, x0, cond, p, KEYS_K
    cfg, p = QC.stmpc_case(202, 10)
    x0, ref, oa, od = QC.stmpc_inputs(202, p, 24, _sref(ctx))

    def run(sel, opts=None):
        return ctx.stmpc_qp(x0[sel], ref[sel], cfg, oa_prev=oa[sel], od_v_prev=od[sel], opts=opts, want_x=True, want_duals=True)

    def cond(e):
        return SQ.fast_condense(x0[e], ref[e], oa[e], od[e], p)
    return run, x0, cond, p, KEYS_S


@pytest.mark.parametrize("kind", ["kmpc", "stmpc"])
def test_max_iter_zero_returns_the_start(ctx, kind):
    """status 2 ("not converged: the last iterate") with the iterate it started from, u = 0; infeasible and non-finite egos keep 1 and 3"""
    km = kind == "kmpc"
    if km:
        cfg, p = QC.kmpc_case(201, 8)
        x0, ref, oa, od = QC.kmpc_inputs(201, p, 24, _kref(ctx))
        iv = 2
    else:
        cfg, p = QC.stmpc_case(202, 10)
        x0, ref, oa, od = QC.stmpc_inputs(202, p, 24, _sref(ctx))
        iv = 3
    x0 = x0.copy()
    x0[5, iv] = p["MAX_SPEED"] + 0.25                   # infeasible: 1
    x0[11, iv] = p["MIN_SPEED"] - 0.25                  # infeasible: 1
    x0[17, 0] = np.nan                                  # non-finite: 3
    o = _abi.kmpc_qp_opts(max_iter=0)
    if km:
        out = ctx.kmpc_qp(x0, ref, cfg, oa_prev=oa, od_prev=od, opts=o, want_xk=True, want_duals=True)
    else:
        out = ctx.stmpc_qp(x0, ref, cfg, oa_prev=oa, od_v_prev=od, opts=o, want_x=True, want_duals=True)
    special = {5: 1, 11: 1, 17: 3}
    for e in range(24):
        if e in special:
            assert out["status"][e] == special[e], (e, out["status"][e])
            for k in ("steer", "speed", "u", "xk" if km else "x", "obj", "duals"):
                assert np.isnan(out[k][e]).all(), (e, k)
            continue
        assert out["status"][e] == 2 and out["iters"][e] == 0, (e, out["status"][e], out["iters"][e])
        assert (out["u"][e] == 0.0).all(), e
        assert out["speed"][e] == x0[e, iv], e
        assert out["steer"][e] == (0.0 if km else x0[e, 2]), e
        c = (KQ.condense(KQ.qp_data(x0[e], ref[e], oa[e], od[e], p), p["T"]) if km else SQ.fast_condense(x0[e], ref[e], oa[e], od[e], p))
        assert abs(out["obj"][e] - c["c"]) <= 1e-10 * (1.0 + abs(c["c"])), (e, out["obj"][e], c["c"])


@pytest.mark.parametrize("kind", ["kmpc", "stmpc"])
def test_max_iter_around_the_default_iteration_count(ctx, kind):
    """k* = the default run's iters.  max_iter = k* and k* + 5 change nothing, bit for bit; max_iter = k* - 1 returns the iterate before
    the last with status 2, and its obj is the objective at that iterate"""
    run, x0, cond, p, keys = _opts_case(ctx, kind)
    full = run(slice(None))
    assert (full["status"] == 0).all(), full["status"]
    ks = np.unique(full["iters"])
    print(kind, "k* values", ks)
    assert ks.min() >= 1
    for k in ks:
        sel = np.flatnonzero(full["iters"] == k)
        for mi in (int(k), int(k) + 5):
            got = run(sel, _abi.kmpc_qp_opts(max_iter=mi))
            for key in keys:
                assert np.array_equal(got[key], full[key][sel]), (kind, k, mi, key)
        short = run(sel, _abi.kmpc_qp_opts(max_iter=int(k) - 1))
        assert (short["status"] == 2).all() and (short["iters"] == k - 1).all(), (kind, k, short["status"], short["iters"])
        for i, e in enumerate(sel):
            for key in keys:
                assert np.isfinite(short[key][i]).all(), (kind, k, e, key)
            c = cond(e)
            f = _fobj(c, short["u"][i].ravel())
            assert abs(short["obj"][i] - f) <= 1e-10 * (1.0 + abs(f)), (kind, k, e)


@pytest.mark.parametrize("kind", ["kmpc", "stmpc"])
def test_loosened_tol_stops_earlier_at_the_documented_rule(ctx, kind):
    run, x0, cond, p, keys = _opts_case(ctx, kind)
    full = run(slice(None))
    tol = 1e-4
    got = run(slice(None), _abi.kmpc_qp_opts(tol=tol))
    assert (got["status"] == 0).all(), got["status"]
    assert (got["iters"] <= full["iters"]).all() and (got["iters"] < full["iters"]).any(), (got["iters"], full["iters"])
    for e in range(len(x0)):
        c = cond(e)
        u, lam = got["u"][e].ravel(), got["duals"][e]
        rd = np.abs(c["H"] @ u + c["g"] + c["G"].T @ lam).max()
        assert rd <= tol * (1.0 + np.abs(c["g"]).max()), (e, rd)              # (recomputation rounding ~1e-13: negligible against 1e-4)
        assert (c["h"] - c["G"] @ u).min() >= -tol * (1.0 + np.abs(c["h"]).max()) and lam.min() >= 0.0, e


def test_option_and_config_range_checks(ctx):
    """qp_opts() and validate_*_qp on every entry point"""
    kcfg, kp = QC.kmpc_case(201, 8)
    dcfg, dp = QC.stmpc_case(202, 10)
    xk, rk, _, _ = QC.kmpc_inputs(201, kp, 2, _kref(ctx))
    xd, rd, _, _ = QC.stmpc_inputs(202, dp, 2, _sref(ctx))
    entry = {"kmpc_qp": lambda o: ctx.kmpc_qp(xk, rk, kcfg, opts=o),
             "kmpc_qp_plan": lambda o: ctx.kmpc_qp_plan(xk, kcfg, dl=QC.DL, opts=o),
             "stmpc_qp": lambda o: ctx.stmpc_qp(xd, rd, dcfg, opts=o),
             "stmpc_qp_plan": lambda o: ctx.stmpc_qp_plan(xd, dcfg, kcfg, dl=QC.DL, dlk=QC.DL, opts=o)}
    try:
        for name, call in entry.items():
            for bad in (dict(max_iter=-1), dict(max_iter=1001), dict(tol=0.0), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf)):
                with pytest.raises(ValueError, match="max_iter must be in"):
                    call(_abi.kmpc_qp_opts(**bad))
            out = call(_abi.kmpc_qp_opts(max_iter=1000))
            assert (out["status"] == 0).all(), (name, out["status"])
    finally:
        ctx.kmpc_qp_warm_reset()
        ctx.stmpc_qp_warm_reset()

    def kc(**kw):
        s = QC.kmpc_spec(201, 8)
        s.update(kw)
        return QC.kmpc_cfg(s)

    def dc(**kw):
        s = QC.stmpc_spec(202, 10)
        s.update(kw)
        return QC.stmpc_cfg(s)
    kq, dq = QC.kmpc_spec(201, 8), QC.stmpc_spec(202, 10)
    for cfgs, call in (((kc, kq, "Rk", "Rdk", "Qk", "Qfk"), lambda c: ctx.kmpc_qp(xk, rk, c)),
                       ((dc, dq, "R", "Rd", "Q", "Qf"), lambda c: ctx.stmpc_qp(xd, rd, c))):
        mk, s, R, Rd, Qn, Qf = cfgs
        for r in ([0.0, s[R][1]], [s[R][0], -1.0], [np.nan, s[R][1]]):
            with pytest.raises(ValueError, match="input weights must be finite, r > 0"):
                call(mk(**{R: r}))
        with pytest.raises(ValueError, match="input weights must be finite, r > 0"):
            call(mk(**{Rd: [-0.1, s[Rd][1]]}))
        for name in (Qn, Qf):
            q = list(s[name])
            q[1] = -0.5
            with pytest.raises(ValueError, match="state weights must be finite and >= 0"):
                call(mk(**{name: q}))
        with pytest.raises(ValueError, match="max_speed >= min_speed"):
            call(mk(MAX_SPEED=1.0, MIN_SPEED=1.5))
        with pytest.raises(ValueError, match="bounds must be > 0"):
            call(mk(MAX_ACCEL=0.0))
        assert (call(mk(**{Rd: [0.0, 0.0]}))["status"] == 0).all()               # legal: rd >= 0


# ---- 4. the classes ----------------------------------------------------------------------------------------------------------------
def _course():
    rl = QC.track()
    return [np.ascontiguousarray(rl[:, k]) for k in (0, 1, 3, 2)]              # cx, cy, cyaw, sp


def test_kmpc_planner_takes_every_qp_field_of_its_config(ctx):
    """mpc_config -> f1p_kmpc_cfg (kinematic_mpc._cfg_struct) and QP_MAX_ITER / QP_TOL -> f1p_kmpc_qp_opts"""
    from f1tenth_planning.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    spec = QC.kmpc_spec(301, 5)
    spec.update(DTK=0.05, MIN_SPEED=-1.0)
    conf = mpc_config(SOLVER="qp", **QC.kmpc_config_fields(spec))
    p = KQ.params(conf)
    assert p["T"] == 5 and not np.array_equal(p["Qk"], p["Qfk"]) and not np.array_equal(p["Rk"], p["Rdk"])
    x0, ref, _, _ = QC.kmpc_inputs(301, p, 32, _kref(ctx))
    planner = KMPCPlanner(waypoints=_course(), config=conf)
    planner.reset()
    out = planner.plan_batch(x0)
    assert (out["status"] == 0).all(), out["status"]
    ref = ctx.kmpc_ref(x0, 5, 0.05, conf.dlk)                                     # the class's own reference: unscaled
    n_exact = 0
    for e in range(32):
        s = KQ.solve_case(x0[e], ref[e], None, None, p)
        if not SQ.exact_ok(s["cond"], s["u"].ravel(), s["lam"]):
            continue
        n_exact += 1
        bar = 1e-5 if s["degenerate"] else 1e-7
        assert np.abs(out["u"][e] - s["u"]).max() <= bar, (e, np.abs(out["u"][e] - s["u"]).max())
        assert abs(out["steer"][e] - s["steer"]) <= bar and abs(out["speed"][e] - s["speed"]) <= bar, e
        assert abs(out["obj"][e] - s["obj"]) <= 1e-10 * (1.0 + abs(s["obj"])), e
    assert n_exact >= 24, n_exact
    conf.QP_MAX_ITER = 0
    planner.reset()
    out0 = planner.plan_batch(x0)
    assert (out0["status"] == 2).all() and (out0["u"] == 0.0).all()
    conf.QP_MAX_ITER, conf.QP_TOL = 50, 1e-4
    planner.reset()
    loose = planner.plan_batch(x0)
    assert (loose["status"] == 0).all()
    d = np.abs(loose["u"] - out["u"]).max()
    assert 0.0 < d < 1e-2, d                                                      # an earlier iterate: near the optimum, not on it


def test_stmpc_planner_takes_every_qp_field_of_its_config(ctx):
    """both branches: states on each side of V_KS; mpc_config -> f1p_stmpc_cfg / f1p_kmpc_cfg (dynamic_mpc._dyn_cfg, _kin_cfg), the
    vehicle parameters, and QP_MAX_ITER / QP_TOL"""
    from f1tenth_planning.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    ds, ks = QC.stmpc_spec(302, 10), QC.kmpc_spec(303, 5)
    shared = dict(WB=0.31, MAX_STEER=0.45, MAX_SPEED=6.5, MIN_SPEED=0.5, MAX_ACCEL=2.5)        # one mpc_config: both branches' bounds
    ds.update(shared)
    ks.update(shared)
    fields = QC.stmpc_config_fields(ds)
    fields.update({k: v for k, v in QC.kmpc_config_fields(ks).items() if k in ("TK", "DTK", "MAX_DSTEER", "Qk", "Qfk", "Rk", "Rdk")})
    conf = mpc_config(SOLVER="qp", V_KS=2.5, **fields)
    p, pk = QC.stmpc_params(ds), QC.kmpc_params(ks)
    E = 32
    x0 = QC.stmpc_inputs(302, p, E, _sref(ctx))[0]
    x0[::2, 3] = np.linspace(0.6, 2.5, E // 2)                                    # half on the kinematic side of V_KS
    x0[::2, 5:] = 0.0
    planner = STMPCPlanner(waypoints=_course(), config=conf, params=np.array(ds["vp"]))
    planner.reset()
    out = planner.plan_batch(x0)
    assert (out["status"] == 0).all(), out["status"]
    assert np.array_equal(out["branch"], (x0[:, 3] > 2.5).astype(np.int32)) and 0 < out["branch"].sum() < E
    rd = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], 10, p["DT"], conf.dl)
    rk = ctx.stmpc_ref(x0[:, [0, 1, 3, 4]], 5, pk["DTK"], conf.dlk)[:, [0, 1, 3, 4]]
    n_exact = 0
    for e in range(E):
        steer, speed, warm, br, deg = SQ.plan_step(x0[e], None, rd[e], rk[e], p, pk, v_ks=2.5)
        assert br == out["branch"][e]
        bar = 1e-5 if deg else 1e-7
        assert abs(out["steer"][e] - steer) <= bar and abs(out["speed"][e] - speed) <= bar, (e, br, out["steer"][e] - steer, out["speed"][e] - speed)
        n_exact += 1
    assert n_exact == E
    conf.QP_MAX_ITER = 0
    planner.reset()
    out0 = planner.plan_batch(x0)
    assert (out0["status"] == 2).all()
    for e in range(E):
        L = 10 if out0["branch"][e] else 5
        assert (out0["u"][e, :L] == 0.0).all() and np.isnan(out0["u"][e, L:]).all(), e
    conf.QP_MAX_ITER, conf.QP_TOL = 50, 1e-4
    planner.reset()
    loose = planner.plan_batch(x0)
    assert (loose["status"] == 0).all()
    for b in (0, 1):
        m = out["branch"] == b
        d = np.abs(loose["steer"][m] - out["steer"][m]).max() + np.abs(loose["speed"][m] - out["speed"][m]).max()
        assert 0.0 < d < 1e-2, (b, d)
