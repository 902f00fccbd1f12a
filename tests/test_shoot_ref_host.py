"""tests/shoot_ref.py checked on the CPU: what tests/test_gpu_shoot_offdefault.py compares the shooting kernels against is itself right, its
cases have clear winners, and the in-kernel sampler's counter layout reuses no random word.

Goldens.  shoot_ref in long double against the reference project's own outputs (g5_g6_kmpc.npz, g12_dynamic_model.npz).  The goldens are fp64
results of T sequential steps, each a handful of roundings at the size of the state: bound 8 T eps max(1, |path|) (1 step: 8 eps max(1, |state|)).
Measured: dynamic rollout (T = 40, |path| <= 8.2) 9.6e-15 against 5.8e-13, dynamic step 1.2e-15, kinematic rollouts 1.8e-15 (T = 8) and 1.5e-14 (T = 30).

mpmath.  One rollout of the default dynamic configuration (T = 40) and one of the "dt.005 T80" entry (T = 80) at 40 digits against the long-double
cost: relative differences 4.2e-19 and 1.9e-19 -- 64 bits of mantissa lose nothing that matters over 80 steps (fp64: 5.7e-16 and 1.6e-17).  Asserted at
1e-17, one twentieth of an fp64 ulp.

Table.  The oracle's fp64 winner against the long-double argmin on every entry of shoot_ref.CASES: equal for every ego of every entry, no exemption.
The seeds are frozen here.  Per entry, the smallest long-double gap between winner and runner-up over the egos, beside the largest fp64 - long double
cost difference over all rollouts (the yardstick `dev` of the GPU test) -- the gaps stand eight and more orders above it, except in the entry that
integrates below the trust speed on purpose and in the near tie (six orders):

    entry           trust speed    speeds         smallest gap    largest |fp64 - long double| cost
    mu0.3           0.538          1.03 .. 2.11   0.233           2.5e-13
    mu0.1           0.165          0.26 .. 0.66   0.901           3.1e-13
    stiff           22.58          2.81 .. 5.07   11.7            43         (the unstable-integrator entry)
    car dt.025      7.156          8.40 .. 12.95  4.00            1.6e-11
    car dt.01       2.862          9.24 .. 13.30  1.60            3.6e-12
    dt.005 T80      0.376          2.19 .. 5.38   0.634           1.4e-11
    dt.05 T63       3.763          4.62 .. 5.82   1340            5.8e-10
    dt.05 T64       3.763          4.62 .. 5.69   353             7.3e-10
    bounds low      1.692          2.95 .. 5.50   0.0432          2.7e-12
    bounds high     2.338          3.17 .. 5.19   7.42            4.5e-12
    xy, r=rd=0      1.882          2.83 .. 5.41   0.0284          3.7e-12
    yaw, r=rd=50    1.882          2.65 .. 4.98   75.8            1.9e-11
    yr beta 200     1.882          2.64 .. 5.50   3.15            6.0e-11
    mu0.3 tie       0.538          0.96 .. 1.57   3.0e-7          1.4e-13    (a near tie on purpose: see shoot_ref.CASES)
    k wb0.2         -              0.55 .. 4.96   1.75            1.9e-12
    k wb2.39        -              0.50 .. 3.63   0.172           2.6e-12

Sampler.  The GPU generator is bit-equal to orc.kmpc_gen_controls (tests/test_gpu_kmpc_gen.py), so its independence is tested here: sample
correlations across neighbouring egos, steps, channels, rollouts, calls and seeds, each within 5 / sqrt(N) of zero (N pairs; the estimate's standard
deviation for independent draws is 1 / sqrt(N), so 5 sigma: 6e-7 per estimate).  Measured: all six below 1.9 / sqrt(N)."""
import numpy as np
import pytest

import shoot_ref as S
from f1tenth_planning_amd import _abi

EPS = np.finfo(np.float64).eps


def test_kinematic_model_against_the_goldens(golden):
    g = golden("g5_g6_kmpc.npz")
    for T in (8, 30):
        cfg = _abi.kmpc_cfg(horizon=T)
        want = g[f"roll{T}_path"]
        got = S.kin_rollout(g[f"roll{T}_x0"], g[f"roll{T}_oa"], g[f"roll{T}_od"], cfg)
        d = float(np.abs(got - want).max())
        print("kinematic rollout", T, d)
        assert d <= 8 * T * EPS * max(1.0, np.abs(want).max())
        assert float(np.abs(S.kin_rollout(g[f"roll{T}_x0"], g[f"roll{T}_oa"], g[f"roll{T}_od"], cfg, np.float64) - want).max()) <= 8 * T * EPS * max(1.0, np.abs(want).max())
    got = S.kin_rollout(g["step_state"], g["step_a"][:, None], g["step_delta"][:, None], _abi.kmpc_cfg(horizon=1))[:, :, 1]
    d = float(np.abs(got - g["step_out"]).max())
    print("kinematic step", d)
    assert d <= 8 * EPS * max(1.0, np.abs(g["step_out"]).max())


def test_dynamic_model_against_the_goldens(golden):
    g = golden("g12_dynamic_model.npz")
    cfg = _abi.stmpc_cfg()
    want = g["dyn_roll_path"]
    got = S.dyn_rollout(g["dyn_roll_x0"], g["dyn_roll_oa"], g["dyn_roll_od"], cfg)
    d = float(np.abs(got - want).max())
    print("dynamic rollout", d, np.abs(want).max())
    assert d <= 8 * cfg.horizon * EPS * max(1.0, np.abs(want).max())
    got = S.dyn_rollout(g["dyn_step_state"], g["dyn_step_a"][:, None], g["dyn_step_dv"][:, None], _abi.stmpc_cfg(horizon=1))[:, :, 1]
    d = float(np.abs(got - g["dyn_step_out"]).max())
    print("dynamic step", d)
    assert d <= 8 * EPS * max(1.0, np.abs(g["dyn_step_out"]).max())


@pytest.mark.parametrize("which", ["default T40", "dt.005 T80"])
def test_long_double_is_enough_mpmath(which):
    if which == "default T40":
        cfg = _abi.stmpc_cfg(horizon=40, n_rollouts=256)
        _, x0, ref, ctrl = S.build_case("yr beta 200")
        x0 = x0[:1]; ref = S.make_ref(7, x0[:, [0, 1, 3, 4]], 40, cfg.dt)
        ctrl = np.random.default_rng(7).normal(0, 1.5, (1, 40, 2, 256)).astype(np.float32)
    else:
        cfg, x0, ref, ctrl = S.build_case(which)
    ld = S.dyn_shoot(x0[:1], ref[:1], ctrl[:1], cfg)
    f64 = S.dyn_shoot(x0[:1], ref[:1], ctrl[:1], cfg, np.float64)
    r = int(ld["best_idx"][0])
    import mpmath as mp
    truth = S.mp_dyn_cost(x0[0], ref[0], ctrl[0, :, :, r], cfg, digits=40)
    rel_ld = float(abs(_mpf(ld["costs"][0, r]) - truth) / abs(truth))
    rel_64 = float(abs(mp.mpf(float(f64["costs"][0, r])) - truth) / abs(truth))
    print(which, "T", cfg.horizon, "long double", rel_ld, "fp64", rel_64)
    assert rel_ld <= 1e-17


def _mpf(x):
    """a long double as an mpmath number, exactly: its fp64 head plus the fp64 tail"""
    import mpmath as mp
    hi = np.float64(x)
    lo = np.float64(x - np.longdouble(hi))
    return mp.mpf(float(hi)) + mp.mpf(float(lo))


@pytest.mark.parametrize("name", list(S.CASES))
def test_table_winners_oracle_vs_long_double(orc, name):
    cs = S.CASES[name]
    cfg, x0, ref, ctrl = S.build_case(name)
    ld = S.shoot(name, x0, ref, ctrl, cfg)
    f64 = S.shoot(name, x0, ref, ctrl, cfg, np.float64)
    o = (orc.stmpc_shoot_batch if cs["solver"] == "st" else orc.kmpc_shoot_batch)(x0, ref, ctrl, cfg)
    dev = float(np.abs(f64["costs"] - ld["costs"]).max())
    vi = 3 if cs["solver"] == "st" else 2
    print(name, "trust", S.trust_speed(cfg) if cs["solver"] == "st" else None, "speeds", x0[:, vi].min(), x0[:, vi].max(), "gap", float(ld["gap"].min()), "dev", dev)
    assert np.isfinite(ld["costs"].astype(np.float64)).all()
    np.testing.assert_array_equal(o["best_idx"], ld["best_idx"])            # no exemption
    np.testing.assert_array_equal(f64["best_idx"], ld["best_idx"])
    # what the entry is for, from the configuration: the speeds against the documented trust speed
    if cs["solver"] == "st":
        vt = S.trust_speed(cfg)
        if cs["expect"] == "fallback":
            assert vt > cfg.max_speed and cs.get("unstable")
        else:
            assert x0[:, 3].min() >= 1.15 * vt and x0[:, 3].max() <= cfg.max_speed and not cs.get("unstable")
    if cs.get("near_tie"):
        # the gap is made small on purpose: still above the GPU test's cost tolerance (16 x 64 ulp of the cost covers it) in every ego, and
        # below a tenth of the absolute part of the filter's margin (2e-2), so the filter has to list both rollouts
        g = ld["gap"].astype(np.float64)
        assert (g > 16 * 64 * EPS * np.abs(ld["best_cost"].astype(np.float64))).all() and (g > 1e3 * dev).all() and (g < 2e-3).all(), g
    elif not cs.get("unstable"):
        assert float(ld["gap"].min()) > 1e6 * dev
        # the oracle's outputs at the long-double winner: the applied sequence is clamped f32 controls, exact but for the rate limit's one fp64 sum
        # (its rounding is relative to the operands: twice the larger bound covers previous value + half-width)
        b = 2 * max(cfg.max_steer_v, cfg.max_accel) if cs["solver"] == "st" else max(cfg.max_accel, cfg.max_steer + cfg.max_dsteer * cfg.dt)
        np.testing.assert_allclose(o["best_seq"], ld["best_seq"].astype(np.float64), rtol=0, atol=4 * EPS * b)
        np.testing.assert_allclose(o["best_cost"], ld["best_cost"].astype(np.float64), rtol=0, atol=16 * max(dev, 4 * EPS * float(np.abs(ld["best_cost"]).max())))
    assert sum(1 for c in S.CASES.values() if c.get("unstable")) == 1


def test_sampler_words_are_independent_across_every_axis(orc):
    E, T, R = 8, 16, 4096
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    seed, call = 20240, 3
    a = orc.kmpc_gen_controls(seed, call, E, cfg, 1.0, 1.0)
    assert (a[:, :, :, 1] == 0).all()                                   # rollout 1 is zeros, rollout 0 the (absent) warm start: excluded below
    b = orc.kmpc_gen_controls(seed, call + 1, E, cfg, 1.0, 1.0)
    c = orc.kmpc_gen_controls(seed + 1, call, E, cfg, 1.0, 1.0)
    z, zb, zc = (v[:, :, :, 2:].astype(np.float64) for v in (a, b, c))
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 0.01

    def corr(u, v):
        u = u.ravel() - u.mean(); v = v.ravel() - v.mean()
        return float((u * v).mean() / np.sqrt((u * u).mean() * (v * v).mean())), u.size

    pairs = {"egos": (z[:-1], z[1:]), "steps": (z[:, :-1], z[:, 1:]), "channels": (z[:, :, 0], z[:, :, 1]), "rollouts": (z[..., :-1], z[..., 1:]),
             "calls": (z, zb), "seeds": (z, zc)}
    for axis, (u, v) in pairs.items():
        r, n = corr(u, v)
        print(axis, "correlation", r, "in units of 1/sqrt(N)", r * np.sqrt(n), "N", n)
        assert abs(r) <= 5 / np.sqrt(n), (axis, r, n)
    # the estimator does see a reused word: the same block against itself shifted by nothing
    assert corr(z[:-1], z[:-1])[0] > 0.999
