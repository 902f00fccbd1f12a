"""The two shooting solvers (csrc/k_kmpc.hip, csrc/k_stmpc.hip) off the reference's vehicle and configuration, against tests/shoot_ref.py in
long double -- a reference written from the reference project's source, not from the kernels or the C oracle -- and at three edges: NaN / inf
controls (streamed, and generated around a NaN warm start) and stmpc_plan's model switch exactly at v_ks.

Per entry of shoot_ref.CASES (tests/test_shoot_ref_host.py freezes the seeds and lists the long-double gaps):
  1. the mixed schedule (f32 filter + fp64 decision) equals the all-fp64 kernel on every output, bit for bit;
  2. *_predict along the winner's sequence and the winner's cost lie within 16 dev of the long-double values, dev = |shoot_ref(float64) -
     shoot_ref(long double)| (cost: per ego, the largest over the winner and the seven next-lowest long-double costs -- the rollouts the
     decision is taken among; one rollout's dev alone is a single draw of a rounding walk and can sit near zero by chance, and the ego's other
     rollouts, some of which brake into the unstable range, say nothing about the winner; path: per ego and row, the largest over the steps),
     floor 64 ulp of the compared magnitude.  16: the kernel contracts to FMA and uses its own sincos (< 1 ulp) where numpy calls libm; both perturb each step by
     a few ulp and the same dynamics amplify both;
  3. best_idx is the long-double argmin (an ego may be exempt only when its long-double gap is below the cost tolerance of 2: none is);
  4. the filter's exactness condition: for every ego the filter decided (nref >= 1), the long-double minimiser r* is listed because untrusted
     (c32 = -inf) or has c32[r*] <= tmin + margin; slack = (c32[r*] - tmin) / margin <= 1;
  5. the entry reaches what it is for: v_trust above max_speed -> every ego nref == -1; speeds above v_trust -> some ego nref >= 1.
The entry that integrates below the trust speed on purpose ("stiff": dev = 43) asserts 1, 5 and the finite / non-finite pattern only.

Measured on the MI355X (worst kernel error / dev over paths and cost; largest slack; nref):

    entry           path err/dev   cost err/dev   slack   nref per ego
    mu0.3           0.64           0.97           0.00    1 1 1 1 1 1 1 1
    mu0.1           0.43           0.83           0.00    1 1 1 1 1 1 3 1
    stiff           -              -              -       -1 x 8               (identity and finite pattern only)
    car dt.025      0.97           0.66           0.00    1 1 1 1 1 1 1 1
    car dt.01       0.53           0.77           0.00    1 1 1 1 1 1 1 1
    dt.005 T80      1.02           0.56           0.00    1 1 1 1 1 1 1 1
    dt.05 T63       1.24           2.97           0.00    9 44 10 1 27 2 30 28
    dt.05 T64       1.42           0.88           0.00    25 39 7 1 11 5 4 6
    bounds low      0.97           1.19           0.00    1 2 1 1 1 1 1 1
    bounds high     1.16           0.71           0.00    5 1 33 1 23 1 1 4
    xy, r=rd=0      1.01           0.80           0.00    1 1 1 1 1 1 1 1
    yaw, r=rd=50    0.90           0.54           0.00    1 1 1 1 1 1 1 1
    yr beta 200     0.79           0.90           0.00    1 1 1 1 1 1 1 1
    mu0.3 tie       0.47           1.00           0.00    2 2 2 2 2 2 2 2
    k wb0.2         0.34           0.69           0.00    1 1 1 1 1 1 1 1
    k wb2.39        0.45           0.85           0.00    1 1 1 1 1 1 1 1

The kernel is about as close to the truth as numpy's fp64 (ratios <= 2.97 against the 16 allowed), no ego is exempt, and the slack is 0 in every
entry: the long-double minimiser is the f32 minimum of its ego, also in "mu0.3 tie", whose winner has a copy 3e-7 above it that the filter lists
beside it (nref 2 in every ego).
"""
import numpy as np
import pytest

import shoot_ref as S
from f1tenth_planning_amd import _abi

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KEYS = ("best_idx", "best_cost", "steer", "speed", "best_seq")


def _macro(src, name):
    """the default of an #ifndef-guarded float macro of a kernel source"""
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "f1tenth_planning_amd", "csrc", src)).read()
    m = re.search(r"#ifndef " + name + r"\s*\n#define " + name + r"\s+([0-9.eE+-]+)f\b", text)
    assert m, (src, name)
    return float(m.group(1))


# the filters' margins, read from the kernels (relative part per step of the horizon, capped at 0.5; absolute part)
MARGIN = {"st": (_macro("k_stmpc.hip", "F1P_ST_MARGIN_REL"), _macro("k_stmpc.hip", "F1P_ST_MARGIN_ABS")),
          "k": (_macro("k_kmpc.hip", "F1P_K4_MARGIN_REL"), _macro("k_kmpc.hip", "F1P_K4_MARGIN_ABS"))}


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        c.set_waypoints(S.centerline(), cols=(1, 2, 5, 3))
        yield c


def _both_modes(ctx, solver, x0, ref, ctrl, cfg):
    """-> (mixed outputs, all-fp64 outputs, c32 [E, R], nref [E]) through the streamed entry point"""
    E, R = x0.shape[0], cfg.n_rollouts
    set_mode, shoot = (ctx.stmpc_set_mode, ctx.stmpc_shoot) if solver == "st" else (ctx.kmpc_set_mode, ctx.kmpc_shoot)
    d_c32, d_n = ctx.alloc(4 * E * R), ctx.alloc(4 * E)
    try:
        set_mode(True, d_c32, d_n)
        mixed = shoot(x0, ref, ctrl, cfg)
        c32 = d_c32.download(np.float32, (E, R)); nref = d_n.download(np.int32, (E,))
        set_mode(False)
        plain = shoot(x0, ref, ctrl, cfg)
    finally:
        set_mode(True)
        d_c32.free(); d_n.free()
    return mixed, plain, c32, nref


def _assert_outputs(solver, cfg, x0, got, want, rows):
    """best_seq, steer and speed of egos `rows` against the long-double values.  A clamped f32 control is exact; the rate limit (previous applied
    value +- half-width) and the output map (state + control dt) are ONE fp64 sum each, whose rounding is relative to its operands, not to a
    result that may cancel: atol = 4 eps (|operand| + |operand|) from the bounds, rtol = 0."""
    if solver == "st":
        m_seq = (2 * cfg.max_steer_v, cfg.max_accel)
        m_steer = np.abs(x0[:, 2]).max() + cfg.max_steer_v * cfg.dt; m_speed = np.abs(x0[:, 3]).max() + cfg.max_accel * cfg.dt
    else:
        m_seq = (cfg.max_accel, cfg.max_steer + cfg.max_dsteer * cfg.dt)
        m_steer = m_seq[1]; m_speed = np.abs(x0[:, 2]).max() + cfg.max_accel * cfg.dt
    for ch in range(2):
        np.testing.assert_allclose(got["best_seq"][rows][:, :, ch], want["best_seq"].astype(np.float64)[rows][:, :, ch], rtol=0, atol=4 * EPS * m_seq[ch],
                                   equal_nan=True, err_msg=f"best_seq channel {ch}")
    np.testing.assert_allclose(got["steer"][rows], want["steer"].astype(np.float64)[rows], rtol=0, atol=4 * EPS * m_steer, equal_nan=True, err_msg="steer")
    np.testing.assert_allclose(got["speed"][rows], want["speed"].astype(np.float64)[rows], rtol=0, atol=4 * EPS * m_speed, equal_nan=True, err_msg="speed")


def _assert_identical(mixed, plain):
    for key in KEYS:
        np.testing.assert_array_equal(mixed[key], plain[key], err_msg=key)


def _cost_dev(ld, f64, k=8):
    """per ego: the largest |fp64 - long double| cost over the k lowest long-double costs (the winner and its nearest rivals)"""
    order = np.argsort(ld["costs"], axis=1, kind="stable")[:, :k]
    with np.errstate(invalid="ignore"):
        d = np.abs(np.take_along_axis(f64["costs"], order, 1) - np.take_along_axis(ld["costs"], order, 1)).astype(np.float64)
    return np.nanmax(np.where(np.isnan(d), 0.0, d), axis=1)


def _within(got, ld, f64, axis):
    """|got - ld| <= max(16 dev, 64 ulp of the magnitude), dev and magnitude the largest along `axis`; -> (the worst error / max(dev, 4 ulp), ok mask)"""
    ld = np.asarray(ld); got = np.asarray(got, np.longdouble)
    dev = np.abs(np.asarray(f64, np.longdouble) - ld).max(axis=axis, keepdims=True).astype(np.float64)
    mag = np.abs(ld).max(axis=axis, keepdims=True).astype(np.float64)
    err = np.abs(got - ld).astype(np.float64)
    base = np.maximum(dev, 4 * EPS * mag)
    ratio = float((err / np.where(base > 0, base, 1.0)).max())
    return ratio, err <= 16 * base


@pytest.mark.parametrize("name", list(S.CASES))
def test_off_default_configuration(ctx, name):
    cs = S.CASES[name]
    solver = cs["solver"]
    cfg, x0, ref, ctrl = S.build_case(name)
    E, T = cs["E"], cs["T"]
    mixed, plain, c32, nref = _both_modes(ctx, solver, x0, ref, ctrl, cfg)
    _assert_identical(mixed, plain)                                                                   # 1
    assert ((nref == -1) | ((nref >= 1) & (nref <= 64))).all()
    ld = S.shoot(name, x0, ref, ctrl, cfg)
    f64 = S.shoot(name, x0, ref, ctrl, cfg, np.float64)
    ar = np.arange(E)
    # 5: from the configuration alone
    vt = S.trust_speed(cfg) if solver == "st" else 0.0
    if cs["expect"] == "fallback":
        assert vt > cfg.max_speed and (nref == -1).all(), (vt, nref)
    else:
        assert (nref >= 1).any() and np.isfinite(c32).any(), nref
    seq = ld["best_seq"].astype(np.float64)                            # the winner's applied sequence as the fp64 input of the model's rollout
    if solver == "st":
        oa, od = seq[:, :, 1], seq[:, :, 0]
        path = ctx.stmpc_predict(x0, oa, od, cfg); p_ld = S.dyn_rollout(x0, oa, od, cfg); p_64 = S.dyn_rollout(x0, oa, od, cfg, np.float64)
    else:
        oa, od = seq[:, :, 0], seq[:, :, 1]
        path = ctx.kmpc_predict(x0, oa, od, cfg); p_ld = S.kin_rollout(x0, oa, od, cfg); p_64 = S.kin_rollout(x0, oa, od, cfg, np.float64)
    if cs.get("unstable"):
        assert float(np.abs(f64["costs"] - ld["costs"]).max()) > 1e-6              # the entry is what it claims to be
        np.testing.assert_array_equal(np.isfinite(plain["best_cost"]), np.isfinite(ld["best_cost"].astype(np.float64)))
        np.testing.assert_array_equal(np.isfinite(path), np.isfinite(p_ld.astype(np.float64)))
        print(f"TABLE {name:14s} unstable entry: identity and finite pattern only; nref {nref.tolist()}")
        return
    # 2: the model along the winner's sequence, and the winner's cost
    r_path, ok_path = _within(path, p_ld, p_64, 2)
    got_cost_ld = ld["costs"][ar, plain["best_idx"]]
    dev_c = _cost_dev(ld, f64)
    base_c = np.maximum(dev_c, 4 * EPS * np.abs(got_cost_ld).astype(np.float64))
    err_c = np.abs(np.asarray(plain["best_cost"], np.longdouble) - got_cost_ld).astype(np.float64)
    r_cost = float((err_c / base_c).max())
    # 3: the winner
    differs = plain["best_idx"] != ld["best_idx"]
    exempt = differs & (ld["gap"].astype(np.float64) < 16 * base_c)
    # 4: the filter's exactness condition at the long-double minimiser
    rel, ab = MARGIN[solver]
    slack = -np.inf
    for e in np.nonzero(nref >= 1)[0]:
        fin = np.isfinite(c32[e])
        assert fin.any()
        tmin = float(c32[e][fin].min())
        margin = abs(tmin) * min(rel * T, 0.5) + ab
        cstar = float(c32[e, ld["best_idx"][e]])
        if cstar == -np.inf:
            continue                                                   # untrusted: listed by construction
        assert np.isfinite(cstar), (e, cstar)
        slack = max(slack, (cstar - tmin) / margin)
    print(f"TABLE {name:14s} path {r_path:7.2f}  cost {r_cost:7.2f}  slack {slack:8.4f}  nref {nref.tolist()}  exempt {int(exempt.sum())}")
    assert ok_path.all(), ("path", r_path, np.argwhere(~ok_path)[:4].tolist())
    assert (err_c <= 16 * base_c).all(), ("cost", r_cost)
    assert not (differs & ~exempt).any() and exempt.sum() <= 1, (plain["best_idx"], ld["best_idx"])
    assert slack <= 1.0, slack
    _assert_outputs(solver, cfg, x0, plain, ld, ~differs)              # the outputs at the winner


# ---- NaN and inf controls ---------------------------------------------------------------------------------------------------------------
def _edge_case(solver, T=20):
    E, R = 12, 256
    rng = np.random.default_rng(77 if solver == "st" else 78)
    cl = S.centerline()
    k = rng.integers(0, len(cl) - 700, E)
    px, py, yaw, v = cl[k, 1] + rng.normal(0, 0.1, E), cl[k, 2] + rng.normal(0, 0.1, E), cl[k, 3] + rng.normal(0, 0.1, E), rng.uniform(3.0, 5.0, E)
    ctrl = np.empty((E, T, 2, R), np.float32)
    if solver == "st":
        cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
        x0 = np.column_stack([px, py, rng.normal(0, 0.05, E), v, yaw, rng.normal(0, 0.2, E), rng.normal(0, 0.02, E)])
        ref = S.make_ref(7, x0[:, [0, 1, 3, 4]], T, cfg.dt)
        sig = (1.5, 1.5)
    else:
        cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
        x0 = np.column_stack([px, py, v, yaw])
        ref = S.make_ref(4, x0, T, cfg.dt)
        sig = (1.5, 0.15)
    for ch in range(2):
        ctrl[:, :, ch, :] = rng.normal(0, sig[ch], (E, T, R))
    return cfg, x0, ref, ctrl


# T = 20; 21 and 5: an odd horizon's last step is the streamed kinematic filter's tail, and 5 steps are fewer chunks than its prefetch ring holds
@pytest.mark.parametrize("T", [20, 21, 5])
@pytest.mark.parametrize("solver", ["st", "k"])
def test_nan_and_inf_controls_streamed(ctx, solver, T):
    """A NaN control stays a NaN through the fp64 bounds (v > hi ? hi : (v < lo ? lo : v)), the rollout's cost is NaN and np.argmin's rule makes
    the FIRST NaN rollout the winner.  The f32 filter must hand such a rollout to fp64 instead of clamping the NaN away.  +-inf controls clamp
    to the bounds in both.  Expected values: shoot_ref in long double."""
    cfg, x0, ref, ctrl = _edge_case(solver, T)
    E, R = ctrl.shape[0], ctrl.shape[3]
    clean = S.shoot(solver, x0, ref, ctrl, cfg)
    w = clean["best_idx"]
    assert ((w >= 2) & (w <= R - 3)).sum() >= 4 and np.isfinite(clean["costs"].astype(np.float64)).all()
    cand = [e for e in range(E) if 2 <= w[e] <= R - 3]
    e_hi, e_lo, e_two, e_mid = cand[:4]
    bad = ctrl.copy()
    bad[e_hi, 0, 0, w[e_hi] + 2] = np.nan                              # step 0, channel 0, above the true winner
    bad[e_lo, T - 1, 1, w[e_lo] - 1] = np.nan                          # the last step, channel 1, below it
    bad[e_two, T // 2, 1, w[e_two] + 1] = np.nan                       # two NaN rollouts in one ego: the lower index wins
    bad[e_two, min(3, T - 2), 0, w[e_two] - 2] = np.nan
    bad[e_mid, min(7, T - 2), 0, w[e_mid]] = np.nan                                # the true winner itself
    nan_egos = [e_hi, e_lo, e_two, e_mid]
    others = [e for e in range(E) if e not in nan_egos]
    e_pinf, e_ninf, e_winf = others[:3]
    bad[e_pinf, min(2, T - 1), 0, :] = np.inf                                      # every rollout of the ego, one step
    bad[e_ninf, min(5, T - 1), 1, ::3] = -np.inf
    bad[e_winf, :, :, w[e_winf]] = np.where(np.arange(T)[:, None] % 2 == 0, np.inf, -np.inf)   # a whole rollout of infinities, alternating
    untouched = others[3:]
    want = S.shoot(solver, x0, ref, bad, cfg)
    np.testing.assert_array_equal(want["best_idx"][nan_egos], [w[e_hi] + 2, w[e_lo] - 1, w[e_two] - 2, w[e_mid]])
    assert np.isnan(want["best_cost"][nan_egos].astype(np.float64)).all() and np.isfinite(np.delete(want["best_cost"].astype(np.float64), nan_egos)).all()
    mixed0, plain0, _, _ = _both_modes(ctx, solver, x0, ref, ctrl, cfg)
    mixed, plain, c32, nref = _both_modes(ctx, solver, x0, ref, bad, cfg)
    print(solver, "nref", nref.tolist(), "best_idx fp64", plain["best_idx"].tolist(), "mixed", mixed["best_idx"].tolist(), "want", want["best_idx"].tolist())
    # the all-fp64 kernel against the reference, every key
    np.testing.assert_array_equal(plain["best_idx"], want["best_idx"])
    assert np.isnan(plain["best_cost"][nan_egos]).all()
    fin = np.isfinite(want["best_cost"].astype(np.float64))
    dev = _cost_dev(want, S.shoot(solver, x0, ref, bad, cfg, np.float64))
    tol = 16 * np.maximum(dev, 4 * EPS * np.abs(want["best_cost"].astype(np.float64)))
    assert (np.abs(plain["best_cost"] - want["best_cost"].astype(np.float64))[fin] <= tol[fin]).all()
    _assert_outputs(solver, cfg, x0, plain, want, np.arange(E))
    assert np.isfinite(plain["best_seq"][others]).all()                # +-inf came out as the clamped finite plan
    # the mixed schedule against the all-fp64 kernel, bit for bit
    _assert_identical(mixed, plain)
    for key in KEYS:
        np.testing.assert_array_equal(plain[key][untouched], plain0[key][untouched], err_msg=key)
        np.testing.assert_array_equal(mixed[key][untouched], mixed0[key][untouched], err_msg=key)


def _dev_outs(ctx, E, T):
    return dict(steer=ctx.alloc(8 * E), speed=ctx.alloc(8 * E), best_idx=ctx.alloc(4 * E), best_cost=ctx.alloc(8 * E), best_seq=ctx.alloc(8 * E * T * 2))


def _download(d, E, T):
    out = dict(steer=d["steer"].download(np.float64, (E,)), speed=d["speed"].download(np.float64, (E,)), best_idx=d["best_idx"].download(np.int32, (E,)),
               best_cost=d["best_cost"].download(np.float64, (E,)), best_seq=d["best_seq"].download(np.float64, (E, T, 2)))
    for b in d.values():
        b.free()
    return out


@pytest.mark.parametrize("collision", [False, True])
@pytest.mark.parametrize("solver", ["st", "k"])
def test_nan_in_the_warm_start_with_generated_controls(ctx, solver, collision):
    """A NaN in the warm start makes that step's control NaN in every rollout but the all-zero one: *_plan_dev (filter on generated controls)
    must equal gen_controls_dev followed by the all-fp64 shoot_dev, bit for bit."""
    cfg, x0, ref, _ = _edge_case(solver)
    E, T, R = x0.shape[0], cfg.horizon, cfg.n_rollouts
    warm = np.random.default_rng(9).normal(0, 0.1, (E, T, 2)).astype(np.float32)
    warm[2, 0, 0] = np.nan; warm[7, T - 1, 1] = np.nan
    if solver == "st":
        smp = _abi.stmpc_sampler(seed=31, call=4, use_warm=True, sigma_steer_v=1.5, sigma_accel=1.5)
        set_warm = lambda: ctx.stmpc_warm_set(warm, np.full(E, 2), T)
        get_warm = lambda: ctx.stmpc_warm_get(E, T)[0]
        set_mode, gen, shoot_dev, plan_dev = ctx.stmpc_set_mode, ctx.stmpc_gen_controls_dev, ctx.stmpc_shoot_dev, ctx.stmpc_plan_dev
    else:
        smp = _abi.kmpc_sampler(seed=31, call=4, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
        set_warm = lambda: ctx.kmpc_warm_set(warm)
        get_warm = lambda: ctx.kmpc_warm_get(E, T)
        set_mode, gen, shoot_dev, plan_dev = ctx.kmpc_set_mode, ctx.kmpc_gen_controls_dev, ctx.kmpc_shoot_dev, ctx.kmpc_plan_dev
    d_x0, d_ref, d_c = ctx.to_device(x0), ctx.to_device(ref), ctx.alloc(4 * E * T * 2 * R)
    set_col = ctx.stmpc_set_collision if solver == "st" else ctx.kmpc_set_collision
    try:
        if collision:                                                  # the occupancy test on an all-free map: the *_col kernels, nothing blocked
            cl = S.centerline()
            lo = cl[:, 1:3].min(axis=0) - 8.0; hi = cl[:, 1:3].max(axis=0) + 8.0
            res = 0.1
            ctx.set_grid(np.full((int(np.ceil((hi[1] - lo[1]) / res)), int(np.ceil((hi[0] - lo[0]) / res))), 255, np.uint8), res, (lo[0], lo[1]), 206)
            set_col(True, 2)
        set_mode(False)
        set_warm()
        gen(d_c, E, cfg, smp)
        d = _dev_outs(ctx, E, T)
        shoot_dev(d_x0, d_ref, d_c, E, cfg, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
        want = _download(d, E, T)
        got = {}
        for mixed in (True, False):
            set_mode(mixed)
            set_warm()
            d = _dev_outs(ctx, E, T)
            plan_dev(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
            got[mixed] = _download(d, E, T)
            got[mixed]["warm"] = get_warm()
    finally:
        set_mode(True)
        if collision:
            set_col(False)
            ctx.set_grid(None, 0.0, (0.0, 0.0), 0)
        d_x0.free(); d_ref.free(); d_c.free()
    print(solver, "fp64 streamed best_idx", want["best_idx"].tolist(), "plan mixed", got[True]["best_idx"].tolist())
    if collision:      # a non-finite tested point counts as occupied: a NaN that reaches a position blocks the rollout, and every rollout of that ego
        assert np.isin(want["best_idx"][[2, 7]], [0, -1]).all() and not np.isfinite(want["best_cost"][[2, 7]]).any()
    else:
        assert np.isnan(want["best_cost"][[2, 7]]).all() and (want["best_idx"][[2, 7]] == 0).all()  # rollout 0, the warm start itself, is the first NaN
    assert np.isfinite(np.delete(want["best_cost"], [2, 7])).all() and (np.delete(want["best_idx"], [2, 7]) >= 0).all()
    for mixed in (True, False):
        for key in KEYS:
            np.testing.assert_array_equal(got[mixed][key], want[key], err_msg=f"{key} mixed={mixed}")
    np.testing.assert_array_equal(got[True]["warm"], got[False]["warm"])


@pytest.mark.parametrize("solver", ["st", "k"])
def test_nonfinite_sigma_is_rejected(ctx, solver):
    """the other way a generated control could be NaN: the entry points refuse a sampler whose sigmas are not finite, nothing is launched"""
    cfg, x0, ref, _ = _edge_case(solver)
    E, T = x0.shape[0], cfg.horizon
    d_x0, d_ref, d = ctx.to_device(x0), ctx.to_device(ref), _dev_outs(ctx, E, T)
    try:
        for bad in (np.inf, np.nan):
            if solver == "st":
                smps = [_abi.stmpc_sampler(seed=1, sigma_steer_v=bad), _abi.stmpc_sampler(seed=1, sigma_accel=bad)]
                plan = ctx.stmpc_plan_dev
            else:
                smps = [_abi.kmpc_sampler(seed=1, sigma_accel=bad), _abi.kmpc_sampler(seed=1, sigma_steer=bad)]
                plan = ctx.kmpc_plan_dev
            for smp in smps:
                with pytest.raises(ValueError):
                    plan(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
    finally:
        for b in d.values():
            b.free()
        d_x0.free(); d_ref.free()


# ---- stmpc_plan's model switch at the threshold ------------------------------------------------------------------------------------------
def test_stmpc_plan_branch_exactly_at_v_ks(ctx):
    """branch = 0 (kinematic) at v <= v_ks, 1 (dynamic) above: egos at v_ks exactly and one ulp to either side; each side's outputs equal
    that branch's own entry point on the same batch (the generator's ego word is the index in the batch)."""
    E, T, R, TK, DTK, v_ks = 12, 20, 256, 8, 0.1, 2.0
    cfg, x0, _, _ = _edge_case("st")
    kcfg = _abi.kmpc_cfg(horizon=TK, n_rollouts=R, dt=DTK)
    x0[:, 3] = np.tile([v_ks, np.nextafter(v_ks, 0.0), np.nextafter(v_ks, 10.0)], E // 3)
    want_branch = np.tile([0, 0, 1], E // 3).astype(np.int32)
    smp = _abi.stmpc_sampler(seed=555, call=2, use_warm=True, sigma_steer_v=1.0, sigma_accel=1.5, sigma_steer=0.15)
    ctx.stmpc_warm_reset()
    got = ctx.stmpc_plan(x0, cfg, kcfg, smp, v_ks=v_ks)
    np.testing.assert_array_equal(got["branch"], want_branch)
    x4 = np.ascontiguousarray(x0[:, [0, 1, 3, 4]])
    dyn = want_branch == 1
    # the dynamic entry point on the whole batch, no warm start
    ctx.stmpc_warm_reset()
    ref = ctx.stmpc_ref(x4, T, cfg.dt, 0.03)
    d_x0, d_ref, d = ctx.to_device(x0), ctx.to_device(ref), _dev_outs(ctx, E, T)
    try:
        ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
    finally:
        wd = _download(d, E, T)
        d_x0.free(); d_ref.free()
    # the kinematic entry point on the whole batch, no warm start
    ctx.kmpc_warm_reset()
    refk = np.ascontiguousarray(ctx.stmpc_ref(x4, TK, DTK, 0.03)[:, [0, 1, 3, 4]])
    ksmp = _abi.kmpc_sampler(seed=555, call=2, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
    d_x0, d_ref, d = ctx.to_device(x4), ctx.to_device(refk), _dev_outs(ctx, E, TK)
    try:
        ctx.kmpc_plan_dev(d_x0, d_ref, E, kcfg, ksmp, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
    finally:
        wk = _download(d, E, TK)
        d_x0.free(); d_ref.free()
    ctx.stmpc_warm_reset(); ctx.kmpc_warm_reset()
    for key in ("steer", "speed", "best_idx", "best_cost"):
        np.testing.assert_array_equal(got[key][dyn], wd[key][dyn], err_msg=key)
        np.testing.assert_array_equal(got[key][~dyn], wk[key][~dyn], err_msg=key)
    np.testing.assert_array_equal(got["best_seq"][dyn, :T], wd["best_seq"][dyn])
    np.testing.assert_array_equal(got["best_seq"][~dyn, :TK], wk["best_seq"][~dyn])
    assert np.isnan(got["best_seq"][~dyn, TK:]).all()
    assert len(np.unique(got["best_idx"])) > 3
