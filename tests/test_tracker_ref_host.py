"""The tracker references and case builders of tests/tracker_ref.py, checked on the CPU: what tests/test_gpu_tracker_edges.py compares the kernels
against is itself right, and its cases reach the edges they are meant to reach.

LQR.  The C oracle's lqr_batch against the long-double reference on the 64-ego speed mix (speeds 0.0, -1.0, 1e-3, 20.0, -0.0, 1e-9 among them), worst
|steer difference| / max(1, |steer|) per parameter set, and the fp64 / np.linalg.pinv mode against the oracle; the iteration counts of the fp64 and the
long-double mode are equal for every ego of every set (a set where they differ would be ill-conditioned and is replaced, not loosened):

    set                                                       long double    fp64 + pinv    iterations
    defaults                                                  7.6e-16        2.2e-16        19 .. 50
    ts=0.05, q=(1,.5,.2,.1), r=0.1, max_iter=200, eps=1e-6    3.5e-16        1.1e-16        112 .. 200
    max_iter=0                                                5.9e-18        0              0
    max_iter=1                                                6.7e-18        0              1
    r=0.0                                                     1.4e-15        4.4e-16        6 .. 50
    r=1e-6, q=(10,1,10,1)                                     1.7e-16        1.2e-16        50
    ts=1e-3, max_iter=500, eps=1e-9                           4.6e-15        2.0e-16        414 .. 500
    wheelbase=0.5, ts=0.02                                    9.6e-16        3.3e-16        14 .. 50
    max_iter=7, eps=0.0                                       5.1e-17        2.8e-17        7

Both are asserted at 1e-13 -- a condition on the INPUTS: the GPU test then holds the kernel to the project's bar (rtol 1e-10) on sets whose fp64 rounding
scale is known to lie four orders below it.  The error state agrees to 6.8e-17.

Cumsum.  For (v, dt, dl) = (1.0, 0.1, 1.0) and (0.7, 0.025, 0.03) at T = 300 the sequential sum's truncated indices differ from (arange(T + 1) * dind)
.astype(int) first at j = 10, 50, 60 and j = 24, 72, 84, at 15 and 11 steps in all.

Wrong rules.  The last three tests switch a deliberately wrong rule into the reference -- the product for the cumsum, a remainder for the single wrap of
pi_2_pi, threshold 5 in the kinematic fold -- and assert that the comparison the GPU test makes on the shared cases then FAILS."""
import numpy as np
import pytest

import tracker_ref as R

LQR_SETS = dict(R.LQR_PARAM_SETS)


def _rel(a, b):
    a = np.asarray(a, R.LD); b = np.asarray(b, R.LD)
    return float(np.max(np.abs(a - b) / np.maximum(1, np.abs(b))))


@pytest.mark.parametrize("name", list(LQR_SETS))
def test_lqr_oracle_vs_long_double(orc, name):
    kw = LQR_SETS[name]
    rl, st, err = R.lqr_speed_mix()
    assert set(R.LQR_SPEEDS) <= set(st[:, 3]) and np.signbit(st[4, 3]) and st[4, 3] == 0.0
    w = orc.lqr_batch(st, err, rl, **kw)
    ld = R.lqr_ref(orc, st, err, rl, dtype=np.longdouble, **kw)
    f64 = R.lqr_ref(orc, st, err, rl, dtype=np.float64, **kw)
    print(name, "long double", _rel(w["steer"], ld["steer"]), "fp64 pinv", _rel(w["steer"], f64["steer"]), "iters", ld["iters"].min(), ld["iters"].max())
    np.testing.assert_array_equal(ld["iters"], f64["iters"])           # else: an ill-conditioned set, to be replaced
    assert ld["iters"].max() <= kw.get("max_iter", 50)
    assert _rel(w["steer"], ld["steer"]) <= 1e-13
    assert _rel(w["steer"], f64["steer"]) <= 1e-13
    for ref in (ld, f64):
        np.testing.assert_array_equal(w["near_idx"], ref["near_idx"])
        np.testing.assert_array_equal(w["speed"], ref["speed"])
        assert float(np.max(np.abs(w["err"] - ref["err"]))) <= 1e-13


def test_lqr_error_state_with_a_long_double_projection(orc):
    """lqr_ref takes the projection from the oracle's nearest_point.  Projecting onto the same segment in long double instead moves e_cog only by the fp64
    rounding of that projection: q = a + t d rounds at the size of the coordinates (eps / 2 each), t carries three roundings times |d|, p - q and the
    dot product two more times |p - q|: below 8 eps (|p| + |d| + |p - q|).  Measured: 3.3e-15 at coordinates up to 50."""
    rl, st, err = R.lqr_speed_mix()
    a = R.lqr_ref(orc, st, err, rl)
    b = R.lqr_ref(orc, st, err, rl, own_projection=True)
    w = orc.lqr_batch(st, err, rl)
    np.testing.assert_array_equal(a["iters"], b["iters"])
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for e, s_ in enumerate(st):
        pt = R.front_axle_xy(s_, 0.33)
        _, dist, _, i = orc.nearest_point(pt, rl[:, :2])
        bound = 8 * eps * (np.abs(pt).max() + np.hypot(*(rl[i + 1, :2] - rl[i, :2])) + dist)
        d = float(np.abs(b["err"][e] - w["err"][e]).max())
        worst = max(worst, d)
        assert d <= bound, (e, d, bound)
    print("own projection: worst error-state difference from the oracle", worst)
    assert worst > 0                                                    # the two projections are not the same arithmetic


def test_stanley_oracle_vs_long_double(orc):
    rl, st, tgt = R.stanley_case()
    seen = set()
    for wb in R.STANLEY_WB:
        for k in R.STANLEY_K:
            w = orc.stanley_batch(st, rl, wheelbase=wb, k_path=k)
            ld = R.stanley_ref(orc, st, rl, wheelbase=wb, k_path=k)
            np.testing.assert_array_equal(w["near_idx"], ld["near_idx"])
            np.testing.assert_array_equal(w["speed"], ld["speed"])
            assert float(np.max(np.abs(w["steer"] - ld["steer"]))) <= 1e-13
            raw = rl[ld["near_idx"], 3] - st[:, 2]                      # psi - theta before the wrap: every band of the issue is visited ...
            for b, (lo, hi) in enumerate(R.STANLEY_BANDS):
                for v in R.STANLEY_V:
                    if ((raw > lo) & (raw < hi) & (st[:, 3] == v) & (np.signbit(st[:, 3]) == np.signbit(v))).any():
                        seen.add((b, repr(v)))
    assert len(seen) == len(R.STANLEY_BANDS) * len(R.STANLEY_V)         # ... at every speed, -0.0 and 0.0 apart


def test_cumsum_cases_differ_from_the_product():
    first = {1.0: ([10, 50, 60], 15), 0.7: ([24, 72, 84], 11)}
    for v, dt, dl in R.CUMSUM_CASES:
        seq = R.ref_index_steps(v, 300, dt, dl)
        prod = (np.arange(301) * ((abs(v) * dt) / dl)).astype(int)
        d = np.nonzero(seq != prod)[0]
        assert list(d[:3]) == first[v][0] and len(d) == first[v][1]
        np.testing.assert_array_equal(prod, R.ref_index_steps(v, 300, dt, dl, _index_rule="product"))
    names = [c["name"] for c in R.ref_cases()]
    assert "cumsum_v1.0" in names and "cumsum_v0.7" in names


@pytest.mark.parametrize("kind", ["kmpc", "stmpc"])
def test_oracle_window(orc, kind):
    """inside its window the oracle is the literal numpy, bit for bit; past it only the numpy reference speaks, and without the clamp it raises"""
    n_in = 0
    for c in R.ref_cases():
        wp, st, T, dt, dl = c["wp"], c["states"], c["T"], c["dt"], c["dl"]
        inside = [R.in_oracle_window(s, len(wp), T, dt, dl) for s in st]
        if c["clamp"]:
            assert not all(inside)
            with pytest.raises(IndexError):
                R.ref_batch(orc, kind, st, wp, T, dt, dl, clamp=False)
            r = R.ref_batch(orc, kind, st, wp, T, dt, dl, clamp=True)
            xrow = r[:, 0, :]
            assert (xrow[~np.array(inside), -1] == wp[-1, 0]).all()   # clamped to il = n - 1
            continue
        assert all(inside), c["name"]
        assert R.same_bits(R.ref_batch(orc, kind, st, wp, T, dt, dl), R.oracle_ref_batch(orc, kind, st, wp, T, dt, dl)), c["name"]
        n_in += 1
    assert n_in >= 20


def _segment_distances(p, xy):
    d = np.diff(xy, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.clip(((p - xy[:-1]) * d).sum(1) / (d * d).sum(1), 0.0, 1.0)
    q = xy[:-1] + t[:, None] * d
    return np.sqrt(((p - q) ** 2).sum(1))


def test_scan_builders_tie_and_duplicate_guarantees(orc):
    wp, st, verts, wb = R.collinear_case()
    near = [R.nearest_index(orc, R.front_axle_xy(s, wb), wp) for s in st]
    assert near == [v - 1 for v in verts] and near[2] == 2 and near[4] == 4          # vertices 3 and 5: segments 2 and 4, the first minimum
    for s, v in zip(st, verts):
        assert (R.front_axle_xy(s, wb) == wp[v, :2]).all()
        assert (_segment_distances(wp[v, :2], wp[:, :2]) == 0.0).sum() == 2
    for n in R.SCAN_LENGTHS:
        variants = dict(R.scan_racelines(n))
        assert "ring" in variants and "dups" in variants and ("dup1" in variants) == (n > 70) and ("ties" in variants or n == 2)
        for name, w in variants.items():
            assert w.shape[1] == 5 and (np.diff(w[:, 2]) > 0).all() and (np.abs(w[:, 3]) <= np.pi).all()
            zero = np.nonzero((np.diff(w[:, :2], axis=0) == 0).all(1))[0]
            (_, st_a), (wb_b, st_b) = R.scan_tracker_states(w, n)
            assert len(st_a) == len(st_b) == 92
            if name == "ties":                                  # an exact tie between two segments: the front axle ON a lattice vertex
                assert len(zero) == 0
                ties = 0
                for s in st_b[-8:]:
                    p = R.front_axle_xy(s, wb_b)
                    d = _segment_distances(p, w[:, :2])
                    ties += int((d == d.min()).sum() >= 2 and d.min() == 0.0)
                    assert R.nearest_index(orc, p, w) == int(np.argmin(d))
                assert ties >= (4 if len(w) > 3 else 0)
            if name in ("dup1", "dups") and len(zero):          # the FIRST zero-length segment wins at any distance
                assert name != "dup1" or list(zero) == [n // 2]
                for s in st_a[::13]:
                    assert R.nearest_index(orc, R.front_axle_xy(s, 0.33), w) == zero[0]
                for s in st_b[::13]:
                    assert R.nearest_index(orc, R.front_axle_xy(s, wb_b), w) == zero[0]
                assert R.nearest_index(orc, R.scan_ref_states(w, n)[70, :2], w) == zero[0]
        assert len(variants["dups"]) == n and (n < 257 or len(np.nonzero((np.diff(variants["dups"][:, :2], axis=0) == 0).all(1))[0]) > 1)


def test_ref_builders_reach_their_edges(orc):
    cases = {c["name"]: c for c in R.ref_cases()}
    for T in R.REF_HORIZONS:
        for E in R.REF_BATCHES:
            assert cases[f"T{T}_E{E}"]["states"].shape == (E, 4)
    for nm in ("wrap_closed", "wrap_open"):                    # some step lands exactly on il == n, from every start index
        c = cases[nm]; n = len(c["wp"])
        starts = set()
        for s in c["states"]:
            ind = R.nearest_index(orc, s[:2], c["wp"])
            raw = ind + R.ref_index_steps(s[2], c["T"], c["dt"], c["dl"])
            assert (raw == n).any() and raw.max() > n and raw.max() < 2 * n
            starts.add(n - 1 - ind)
        assert starts == {1, 2, 5, 6}
    assert (cases["wrap_closed"]["wp"][0, :2] == cases["wrap_closed"]["wp"][-1, :2]).all()
    assert not (cases["wrap_open"]["wp"][0, :2] == cases["wrap_open"]["wp"][-1, :2]).any()
    c = cases["clamp"]; n = len(c["wp"])
    assert n == 65 and max(int(R.ref_index_steps(s[2], c["T"], c["dt"], c["dl"])[-1]) for s in c["states"]) >= 2 * n
    c = cases["fold"]                                           # cyaw[ind] - yaw at +-4.4, +-4.6, +-4.9, +-5.1; headings over [-2 pi, 4 pi]
    assert c["wp"][:, 3].min() < -np.pi and c["wp"][:, 3].max() > 3 * np.pi
    for s, d in zip(c["states"], R.FOLD_OFFSETS):
        ind = R.nearest_index(orc, s[:2], c["wp"])
        assert abs((c["wp"][ind, 3] - s[3]) - d) < 1e-9
    c = cases["speeds"]
    for kind in ("kmpc", "stmpc"):
        r = R.ref_batch(orc, kind, c["states"], c["wp"], c["T"], c["dt"], c["dl"])
        assert R.same_bits(r[0], r[1]) and R.same_bits(r[4], r[5]) and not R.same_bits(r[0], r[4])     # v < 0 as |v|
        for e in (2, 3):                                       # v = 0.0 and -0.0: every column is the one at ind
            assert (r[e] == r[e][:, :1]).all()
        if kind == "stmpc":
            assert R.same_bits(r[:, [2, 5, 6], :], np.zeros_like(r[:, [2, 5, 6], :]))


# ---- the comparisons of the GPU test fail against a deliberately wrong copy of the logic ------------------------------------------------------------
def test_wrong_rule_product_instead_of_cumsum_is_caught(orc):
    for kind in ("kmpc", "stmpc"):
        caught = []
        for c in R.ref_cases():
            right = R.ref_batch(orc, kind, c["states"], c["wp"], c["T"], c["dt"], c["dl"], clamp=c["clamp"])
            wrong = R.ref_batch(orc, kind, c["states"], c["wp"], c["T"], c["dt"], c["dl"], clamp=c["clamp"], _index_rule="product")
            if not R.same_bits(right, wrong):
                caught.append(c["name"])
        assert "cumsum_v1.0" in caught and "cumsum_v0.7" in caught, caught


def test_wrong_rule_remainder_instead_of_single_wrap_is_caught(orc):
    rl, st, tgt = R.stanley_case()
    want = orc.stanley_batch(st, rl)
    wrong = R.stanley_ref(orc, st, rl, dtype=np.float64, _wrap="remainder")
    right = R.stanley_ref(orc, st, rl, dtype=np.float64)
    assert float(np.max(np.abs(right["steer"] - want["steer"]))) <= 1e-12          # the GPU test's bar
    bad = np.abs(wrong["steer"] - want["steer"]) > 1e-12
    outer = np.abs(tgt) > 3 * np.pi
    assert bad[outer].all() and not bad[~outer].any()                               # a remainder differs exactly outside (-3 pi, 3 pi)


def test_wrong_rule_fold_threshold_5_in_the_kinematic_reference_is_caught(orc):
    c = {c["name"]: c for c in R.ref_cases()}["fold"]
    right = R.ref_batch(orc, "kmpc", c["states"], c["wp"], c["T"], c["dt"], c["dl"])
    wrong = R.ref_batch(orc, "kmpc", c["states"], c["wp"], c["T"], c["dt"], c["dl"], _fold_thr=5)
    raw = R.ref_batch(orc, "kmpc", c["states"], c["wp"], c["T"], c["dt"], c["dl"], fold=False)
    dyn = R.ref_batch(orc, "stmpc", c["states"], c["wp"], c["T"], c["dt"], c["dl"])
    differs = [not R.same_bits(right[e, 3, 0], wrong[e, 3, 0]) for e in range(len(R.FOLD_OFFSETS))]
    assert differs == [abs(d) in (4.6, 4.9) for d in R.FOLD_OFFSETS]                # between the two thresholds, column 0
    assert R.same_bits(wrong[:, 3], dyn[:, 4]) and not R.same_bits(right[:, 3], dyn[:, 4])
    folded = [not R.same_bits(right[e, 3, 0], raw[e, 3, 0]) for e in range(len(R.FOLD_OFFSETS))]
    assert folded == [abs(d) > 4.5 for d in R.FOLD_OFFSETS]
