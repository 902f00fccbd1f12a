"""The fp64 clothoid evaluation of csrc/lattice_device.h (interval_setup, interval_increment, piece_anchor / piece_advance / piece_state_at) and
the cubic generator against the high-precision reference of tests/clothoid_ref.py (fixture tests/golden/g19_clothoid_eval.npz):
k_clothoid_sample on a table aimed at the evaluator's regime switches and on the G14 goals, the planning kernels' rows, costs and winners,
the Clothoid class, and what k_clothoid_sample answers outside the arithmetic's premises.  Bars: clothoid_ref.clothoid_errors / cubic_errors."""
import os

import numpy as np
import pytest

import clothoid_ref as R
from f1tenth_planning_amd import _abi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    c = Context(0)
    c.set_waypoints(synth.make_raceline(seed=0))
    yield c
    c.close()


@pytest.fixture(scope="module")
def table_rows(ctx, fx):
    """k_clothoid_sample on the whole table, one call per station count -> list of rows [S, 4] in table order"""
    table, _ = fx
    out = [None] * len(table)
    for S in sorted({c["S"] for c in table}):
        sel = [i for i, c in enumerate(table) if c["S"] == S]
        rows = ctx.clothoid_sample(np.array([[table[i]["k0"], table[i]["dk"], table[i]["L"]] for i in sel]), S)
        for i, r in zip(sel, rows):
            out[i] = r
    return out


@pytest.fixture(scope="module")
def goal_rows(ctx, fx):
    _, G = fx
    return {S: ctx.clothoid_sample(G["params"], S) for S in R.G_S}


def test_sample_xy_on_the_regime_table(fx, table_rows):
    """x, y within 1e-12 max(1, L) of the reference on every table clothoid: nsub 1 (the one-piece path), 2 .. 15, 16, above 16 up to 1667, the
    16-piece anchor inside a station interval and on a station, S = 1 .. 1000, zero / tiny / subnormal kappa', mirrors, spirals of 15.8 and
    60 rad, L = 1e-3 .. 20.  Prints the largest error per regime, in units of the bar."""
    table, _ = fx
    worst = {}
    for c, got in zip(table, table_rows):
        exy, _ = R.clothoid_errors(got, c["rows"], c["L"])
        key = "nsub 1" if c["nsub"] == 1 else "nsub 2..15" if c["nsub"] < 16 else "nsub 16" if c["nsub"] == 16 else "nsub 17..300" if c["nsub"] <= 300 else "nsub 1667"
        for k in (key, "anchor inside an interval" if c["anchor_inside"] else "no anchor inside an interval"):
            worst[k] = max(worst.get(k, 0.0), exy)
        assert exy <= 1.0, (c["label"], exy)
    print("largest x, y error / bar per regime:", {k: f"{v:.1e}" for k, v in sorted(worst.items())})
    for c, got in zip(table, table_rows):                              # a mirror pair is a mirror image, bit for bit (sincos is odd / even)
        if c["mirror_of"] >= 0:
            np.testing.assert_array_equal(got, table_rows[c["mirror_of"]] * [1.0, -1.0, -1.0, 1.0], err_msg=c["label"])


def test_sample_xy_within_the_re_anchored_drift(fx, table_rows):
    """a sharper bar than 1e-12 where the scheme itself promises one (clothoid_ref.drift_bound: 3e-14 rad of phasor drift between the
    16-piece anchors, times L, plus the roundings of the sums): without the re-anchoring the table's long curves (251 x 16 and 1667 pieces)
    are off by up to 5 of these bounds and still inside 1e-12; a series-table entry wrong in its 10th digit shows here before it shows there"""
    table, _ = fx
    worst = max((np.abs(got[:, :2] - c["rows"][:, :2]).max() / R.drift_bound(c), c["label"]) for c, got in zip(table, table_rows))
    print(f"largest x, y error: {worst[0]:.2f} of the drift bound ({worst[1]})")
    assert worst[0] <= 1.0, worst


def test_sample_theta_kappa_within_the_rounding_of_their_terms(fx, table_rows, goal_rows):
    """theta and |kappa| of every table row and goal row within 4 * 2^-53 of the magnitude of their terms + 1e-300 (clothoid_ref.theta_kappa_rounding)"""
    table, G = fx
    for c, got in zip(table, table_rows):
        assert (np.abs(got[:, 2:] - c["rows"][:, 2:]) <= R.theta_kappa_rounding(c["k0"], c["dk"], c["L"], c["S"])).all(), c["label"]
    for S in R.G_S:
        for i, p in enumerate(G["params"]):
            assert (np.abs(goal_rows[S][i][:, 2:] - G["rows"][S][i][:, 2:]) <= R.theta_kappa_rounding(*p, S)).all()


def test_sample_theta_kappa_at_the_relative_bar(fx, table_rows, goal_rows):
    """theta and |kappa| at 1e-12 relative + 1e-300 on the table and the goals.  11 of the 213 goals have a heading of exactly 0: the true end
    heading of the fixture's (k0, dk, L) is the fit's rounding residue (7e-17 .. 1.4e-15 rad), and so is |kappa| at the inflection of those
    S-curves (the middle station of S = 3).  s * (k0 + 0.5 * s * dk) in plain doubles keeps the rounding of its terms there (~2 rad: relative
    error up to 1); k_clothoid_sample forms both sums compensated (sum_prod) and meets the bar on every value."""
    table, G = fx
    for c, got in zip(table, table_rows):
        assert R.clothoid_errors(got, c["rows"], c["L"])[1] <= 1.0, c["label"]
    for S in R.G_S:
        d = np.abs(goal_rows[S] - G["rows"][S])[..., 2:]
        bad = d > 1e-12 * np.abs(G["rows"][S][..., 2:]) + 1e-300
        print(f"S = {S}: {int(bad.sum())} of {bad.size} values miss the relative bar, largest absolute error among them {d[bad].max() if bad.any() else 0.0:.2e}")
        assert not bad.any(), S


def test_a_clothoid_gets_the_same_bits_whatever_its_neighbours(ctx, fx):
    """one thread per clothoid, 256 per workgroup: launches of 257, 256, 255 and 1 clothoids give each clothoid the same rows"""
    table, _ = fx
    P = np.array([[c["k0"], c["dk"], c["L"]] for c in table])
    P = np.concatenate([P, P[::-1], P])[:257]
    full = ctx.clothoid_sample(P, 17)
    np.testing.assert_array_equal(ctx.clothoid_sample(P[:256], 17), full[:256])
    np.testing.assert_array_equal(ctx.clothoid_sample(P[:255], 17), full[:255])
    np.testing.assert_array_equal(ctx.clothoid_sample(P[1:], 17), full[1:])                  # every clothoid in another lane
    for i in (0, 5, 100, 255, 256):
        np.testing.assert_array_equal(ctx.clothoid_sample(P[i:i + 1], 17)[0], full[i])


def test_sample_xy_on_the_g14_goals_own_parameters(fx, goal_rows):
    """the fixture's own (k0, dk, L) of every 8th G14 goal -- 42 behind the ego, 99 with |theta| > 1.3 -- evaluated by k_clothoid_sample at
    S = 2, 3, 50: x, y within 1e-12 max(1, L) of the reference"""
    _, G = fx
    for S in R.G_S:
        exy, _ = R.clothoid_errors(goal_rows[S], G["rows"][S], G["params"][:, 2])
        print(f"goals, S = {S}: largest x, y error {exy:.1e} of the bar")
        assert exy <= 1.0, S


def test_fit_then_evaluate_ends_at_the_goal(ctx, golden):
    """clothoid_g1 then clothoid_sample on all 1702 solvable G14 goals at S = 2, 3, 50: the last row is the goal (x, y within 1e-12 max(1, r), heading
    congruent to theta modulo 2 pi within 1e-12: the fit and the evaluator are each pinned at that bar), and no fitted clothoid comes near the 4096-piece cap: at S = 2 the
    largest uncapped piece count is 56 (the goal (-1, 0, 0), a full turn behind the ego)"""
    g = golden("g14_clothoid_g1.npz")
    G = g["goals"][g["ok"] == 1]
    assert len(G) == 1702
    k0, dk, L, ok = ctx.clothoid_g1(G)
    assert ok.all()
    r = np.hypot(G[:, 0], G[:, 1])
    for S in R.G_S:
        last = ctx.clothoid_sample(np.column_stack([k0, dk, L]), S)[:, -1]
        assert (np.abs(last[:, :2] - G[:, :2]).max(axis=1) <= 1e-12 * np.maximum(1.0, r)).all(), S
        assert np.abs(np.remainder(last[:, 2] - G[:, 2] + np.pi, 2 * np.pi) - np.pi).max() <= 1e-12, S
    ns = [R.nsub(k0[i], dk[i], L[i], 2) for i in range(len(G))]
    assert max(ns) == 56


def _cfg(S, generator="clothoid"):
    return _abi.lattice_cfg(lookaheads=[1.0] * 8, widths=[0.0] * 8, n_stations=S, weights=(0.3, 0.2, 0.25, 0.25), check_collision=False, generator=generator)


@pytest.fixture(scope="module")
def poses():
    return synth.make_egos(synth.make_raceline(seed=0), R.PLAN_E, seed=5)


@pytest.mark.parametrize("S", R.PLAN_S)
def test_planning_kernels_rows_costs_and_winners(ctx, fx, poses, S):
    """4 egos x 64 host goals (the fixture's goals, NaN fillers), no map, with and without prev_theta.  Mode 0 (all fp64), want_all:
    x, y of all_traj are bit for bit clothoid_sample(clothoid_g1(goals)) -- the station loop and k_clothoid_sample are one arithmetic -- which the
    tests above pin to the reference; theta and |kappa| (plain sums in the station loop, compensated in k_clothoid_sample) within the rounding
    of their terms; directly against the reference rows (S = 2, 3, 50) within the fit's 1e-9 max(1, r); all_cost against
    clothoid_ref.cost in long double at rtol 1e-10 / atol 1e-12; best_idx the reference's argmin, no ego excused.  Modes 2 and 3 (the mixed
    schedule): best_traj, best_cost, best_idx bit-equal to mode 0."""
    _, G = fx
    goals, src = R.plan_goals(G["goals"])
    k0, dk, L, ok = ctx.clothoid_g1(goals.reshape(-1, 3))
    assert (ok.reshape(src.shape) == (src >= 0)).all()
    chain = ctx.clothoid_sample(np.column_stack([k0, dk, L]), S).reshape(R.PLAN_E, R.PLAN_C, S, 4)
    Lm = np.where(src >= 0, L.reshape(src.shape), np.nan)
    tk = np.stack([R.theta_kappa_rounding(k0[i], dk[i], L[i], S) for i in range(len(L))]).reshape(R.PLAN_E, R.PLAN_C, S, 2)
    cfg = _cfg(S)
    try:
        for prev in (None, R.plan_prev_theta(S)):
            ctx.lattice_set_mode(0)
            got = ctx.lattice_plan(poses, cfg, goals=goals, prev_theta=prev, want_all=True)
            np.testing.assert_array_equal(got["all_traj"][src >= 0][..., :2], chain[src >= 0][..., :2])
            assert (np.abs(got["all_traj"] - chain)[..., 2:] <= tk)[src >= 0].all()
            assert (got["all_traj"][src < 0] == 0.0).all()
            if S in R.G_S:
                want_rows = G["rows"][S][np.maximum(src, 0)]
                r = np.hypot(goals[..., 0], goals[..., 1])[..., None, None]
                assert (np.abs(got["all_traj"] - want_rows)[..., :2] <= 1e-9 * np.maximum(1.0, r))[src >= 0].all()
            want, excused = R.plan_costs(chain, Lm, cfg, prev)
            assert not excused.any()
            np.testing.assert_array_equal(np.isinf(got["all_cost"]), src < 0)
            np.testing.assert_allclose(got["all_cost"][src >= 0], want[src >= 0], rtol=1e-10, atol=1e-12)
            np.testing.assert_array_equal(got["best_idx"], np.argmin(want, axis=1))
            np.testing.assert_array_equal(got["best_traj"], got["all_traj"][np.arange(R.PLAN_E), got["best_idx"]])
            for mode in (2, 3):
                ctx.lattice_set_mode(mode)
                mixed = ctx.lattice_plan(poses, cfg, goals=goals, prev_theta=prev)
                for k in ("best_traj", "best_cost", "best_idx"):
                    np.testing.assert_array_equal(mixed[k], got[k], err_msg=f"mode {mode}: {k}")
    finally:
        ctx.lattice_set_mode(1)


@pytest.mark.parametrize("S", R.G_S)
def test_cubic_generator_against_its_definition(ctx, fx, poses, S):
    """generator="cubic" on the same plans against clothoid_ref.cubic_rows -- a Hermite basis and a curvature formula written from the
    definition, not from the kernel: x, y 1e-12 max(1, m), theta 1e-12 absolute, |kappa| 1e-12 relative + 4 * 2^-53 cond / sp^1.5 on the stations
    with sp >= 1e-6 m^4 (at most 2 % left out); on the well-conditioned goals (clothoid_ref.cubic_plan_keep) all_cost against clothoid_ref.cost
    of the reference rows, L their chord sum, and the winner."""
    _, G = fx
    want_rows, sp, cond = G["cubic"][S]
    m = np.hypot(G["goals"][:, 0], G["goals"][:, 1])
    cfg = _cfg(S, "cubic")
    try:
        ctx.lattice_set_mode(0)
        goals, src = R.plan_goals(G["goals"])
        got = ctx.lattice_plan(poses, cfg, goals=goals, want_all=True)
        rows = np.empty_like(want_rows)
        rows[src[src >= 0]] = got["all_traj"][src >= 0]
        exy, eth, ek, out = R.cubic_errors(rows, want_rows, sp, cond, m)
        print(f"cubic S = {S}: x, y {exy:.1e}, theta {eth:.1e}, |kappa| {ek:.1e} of their bars, {100 * out:.2f} % of the stations left out")
        assert out <= 0.02 and exy <= 1.0 and eth <= 1.0 and ek <= 1.0
        goals, src = R.plan_goals(G["goals"], R.cubic_plan_keep(G))
        assert (src >= 0).sum(axis=1).min() >= 16
        ref = np.where((src >= 0)[..., None, None], want_rows[np.maximum(src, 0)], np.nan)
        L = np.array([[float(R.chord_sum(list(ref[e, k].astype(np.longdouble)))) if src[e, k] >= 0 else np.nan for k in range(R.PLAN_C)] for e in range(R.PLAN_E)])
        for prev in (None, R.plan_prev_theta(S)):
            ctx.lattice_set_mode(0)
            got = ctx.lattice_plan(poses, cfg, goals=goals, prev_theta=prev, want_all=True)
            want, excused = R.plan_costs(ref, L, cfg, prev)
            assert not excused.any()
            np.testing.assert_array_equal(np.isinf(got["all_cost"]), src < 0)
            np.testing.assert_allclose(got["all_cost"][src >= 0], want[src >= 0], rtol=1e-10, atol=1e-12)
            np.testing.assert_array_equal(got["best_idx"], np.argmin(want, axis=1))
            for mode in (2, 3):
                ctx.lattice_set_mode(mode)
                mixed = ctx.lattice_plan(poses, cfg, goals=goals, prev_theta=prev)
                for k in ("best_traj", "best_cost", "best_idx"):
                    np.testing.assert_array_equal(mixed[k], got[k], err_msg=f"mode {mode}: {k}")
    finally:
        ctx.lattice_set_mode(1)


def test_clothoid_class_against_the_fixture(ctx, fx):
    """Clothoid(x0, y0, th0, k0, dk, L): X(s), Y(s) (host quadrature) and sample(n) (k_clothoid_sample) against the reference rows moved to the
    start pose, on five table cases: x, y within 1e-12 max(1, L), theta and |kappa| within the rounding of their terms"""
    from f1tenth_planning_amd.utils.clothoid import Clothoid
    table, _ = fx
    by = {c["label"]: c for c in table}
    x0, y0, th0 = 1.0, -2.0, 0.7
    cs, sn = np.cos(th0), np.sin(th0)
    for lab in ("nsub1/k0", "nsub5/dkL", "nsub17/k0/mirror", "inflection", "spiral15.8"):
        c = by[lab]
        cl = Clothoid(x0, y0, th0, c["k0"], c["dk"], c["L"])
        want = c["rows"]
        wx, wy = x0 + cs * want[:, 0] - sn * want[:, 1], y0 + sn * want[:, 0] + cs * want[:, 1]
        bar = 1e-12 * max(1.0, c["L"])
        rows = cl.sample(c["S"], ctx)
        assert np.abs(rows[:, 0] - wx).max() <= bar and np.abs(rows[:, 1] - wy).max() <= bar, lab
        tk = R.theta_kappa_rounding(c["k0"], c["dk"], c["L"], c["S"])
        assert (np.abs(rows[:, 2] - (th0 + want[:, 2])) <= tk[:, 0] + 2.0 ** -52 * np.abs(th0 + want[:, 2])).all() and (np.abs(rows[:, 3] - want[:, 3]) <= tk[:, 1]).all(), lab
        for i in (1, c["S"] // 2, c["S"] - 1):
            s = R.stations(c["L"], c["S"])[i]
            assert abs(cl.X(s) - wx[i]) <= bar and abs(cl.Y(s) - wy[i]) <= bar, (lab, i)


def test_out_of_premise_clothoids_get_nan_rows(ctx):
    """A clothoid with more than 4096 pieces per station interval by either of interval_setup's rules (its cap would leave |a| > 0.15 or
    |b| > 0.02: (0.1, 1e4, 3) at S = 3 was off by 1.7e-4 m, (5, 1e6, 4) at S = 2 by 1e19 m), or with a parameter that is not finite: every row
    NaN, the neighbours' rows untouched, the call succeeds.  (400, 0, 10) at S = 2 -- 13334 pieces by the curvature rule alone, which the
    capped arithmetic still served to 8.7e-14 m -- is covered by the same rule: one rule, no carve-out."""
    good = np.array([[0.5, 0.2, 3.0], [3.1, -4.1, 1.5], [-0.4, 0.9, 5.5]])
    nan, inf = np.nan, np.inf
    bad = [[0.1, 1e4, 3.0], [5.0, 1e6, 4.0], [400.0, 0.0, 10.0], [nan, 0.2, 3.0], [0.5, nan, 3.0], [0.5, 0.2, nan], [inf, 0.2, 3.0], [-inf, 0.2, 3.0],
           [0.5, inf, 3.0], [0.5, -inf, 3.0], [0.5, 0.2, inf], [0.0, 0.0, inf], [1e308, 1e308, 10.0]]
    for S in (2, 3):
        alone = ctx.clothoid_sample(good, S)
        assert np.isfinite(alone).all()
        P = np.empty((2 * len(bad) + 1, 3))
        P[0::2] = good[np.arange(len(bad) + 1) % 3]
        P[1::2] = bad
        rows = ctx.clothoid_sample(P, S)
        for j, b in enumerate(bad):
            assert np.isnan(rows[2 * j + 1]).all(), (S, b)
        np.testing.assert_array_equal(rows[0::2], alone[np.arange(len(bad) + 1) % 3])
    assert R.nsub(0.1, 1e4, 3.0, 3) == 150001 and R.nsub(5.0, 1e6, 4.0, 2) > 4096 and R.nsub(400.0, 0.0, 10.0, 2) == 13334
    just = np.array([[4095.5 * 0.3 / 2.0, 0.0, 2.0], [4096.5 * 0.3 / 2.0, 0.0, 2.0]])       # 4096 pieces: served; 4097: not
    edge = ctx.clothoid_sample(just, 2)
    assert np.isfinite(edge[0]).all() and np.isnan(edge[1]).all()
    from f1tenth_planning_amd.utils.clothoid import Clothoid
    assert np.isnan(Clothoid(1.0, -2.0, 0.7, 5.0, 1e6, 4.0).sample(2, ctx)).all()
    assert np.isfinite(Clothoid(1.0, -2.0, 0.7, 0.4, 0.9, 5.5).sample(2, ctx)).all()
