"""k_stanley, k_lqr, k_kmpc_ref and k_stmpc_ref at their edges on the MI355X, against the CPU oracle and the plain-numpy references of
tests/tracker_ref.py (whose cases and references tests/test_tracker_ref_host.py checks without a GPU).

The four kernels run the chunk-pruned nearest-segment scan in thread layouts of their own -- 64 lanes and wave_argmin (Stanley), the same 64 times
per wave into LDS and then one thread per ego (LQR), 256 threads and block_argmin (the two reference extractions) -- so each of them is put through
  a. the scan's adversarial polylines (2 .. 9000 points, exact ties, NaN segments, far queries, front axles exactly on vertices),
  b. batches that leave a workgroup partly filled, bit-identical to the rows of a larger batch,
  c. LQR off its defaults (nine parameter sets, speeds 0, -0.0, negative, tiny; three steps with the error state carried over),
  d. Stanley around the single wrap of pi_2_pi and atan2 at v <= 0,
  e. the reference extraction's sequential cumsum, index wrap, clamp past one lap, horizons past 256 and the two fold thresholds.
Bars: indices, speeds and reference trajectories exact; Stanley steer atol 1e-12; LQR steer rtol 1e-10 + atol 1e-12 and err atol 1e-13 (the bars of
test_controllers_vs_oracle_4096).  One qualification: in the scan test (a), where queries lie up to 1.4e4 from the track, the err bar is 1e-13 times
max(1, the query's distance from the track), that is 1e-13 relative at the far queries (see _check_tracker); b and c use the flat 1e-13.  The LQR bar lies four orders above the fp64 rounding scale of these parameter sets, which the host test measures
against long double (<= 4.6e-15 relative); test_lqr_off_defaults prints the kernel's own worst difference from the oracle per set.
Non-finite speeds are not tested in the reference extraction: (int)cum is undefined for them."""
import numpy as np
import pytest

import tracker_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    c = Context(0)
    yield c
    c.close()


def _check_tracker(got, want, what, lqr=False, err_scale=None):
    """err_scale [E] (the scan's far queries): e_cog is the front axle's offset from the track, up to 1.4e4 there, times cos / sin of the heading, which
    two maths libraries may round an ulp apart; the error state's bar of 1e-13 is the bar for offsets of order 1 and scales with the offset"""
    np.testing.assert_array_equal(got["near_idx"], want["near_idx"], err_msg=f"{what} near_idx")
    np.testing.assert_array_equal(got["speed"], want["speed"], err_msg=f"{what} speed")
    nan = np.isnan(want["steer"])
    np.testing.assert_array_equal(np.isnan(got["steer"]), nan, err_msg=f"{what} NaN pattern")
    if lqr:
        np.testing.assert_allclose(got["steer"][~nan], want["steer"][~nan], rtol=1e-10, atol=1e-12, err_msg=f"{what} steer")
        np.testing.assert_array_equal(np.isnan(got["err"]), np.isnan(want["err"]), err_msg=f"{what} err NaN pattern")
        scale = np.ones(len(nan)) if err_scale is None else np.asarray(err_scale)
        assert (np.abs(got["err"] - want["err"])[~nan] <= 1e-13 * scale[~nan, None]).all(), f"{what} err"
    else:
        np.testing.assert_allclose(got["steer"][~nan], want["steer"][~nan], rtol=0, atol=1e-12, err_msg=f"{what} steer")


def _refs(ctx, kind, states, T, dt, dl):
    return ctx.kmpc_ref(states, T, dt=dt, dl=dl) if kind == "kmpc" else ctx.stmpc_ref(states, T, dt=dt, dl=dl)


# ---- a. the scan through each consumer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCAN_LENGTHS)
def test_scan_through_each_consumer(ctx, orc, n):
    for name, wp in R.scan_racelines(n):
        ctx.set_waypoints(wp)
        for wb, st in R.scan_tracker_states(wp, n):
            what = f"n={n} {name} wheelbase={wb}"
            _check_tracker(ctx.stanley(st, wheelbase=wb), orc.stanley_batch(st, wp, wheelbase=wb), what + " stanley")
            err = np.zeros((len(st), 2))
            dist = np.array([orc.nearest_point(R.front_axle_xy(s, wb), wp[:, :2])[1] for s in st])
            _check_tracker(ctx.lqr(st, err, wheelbase=wb), orc.lqr_batch(st, err, wp, wheelbase=wb), what + " lqr", lqr=True,
                           err_scale=np.maximum(1.0, np.nan_to_num(dist, nan=1.0)))
        st = R.scan_ref_states(wp, n)
        for kind in ("kmpc", "stmpc"):
            got = _refs(ctx, kind, st, 3, 0.1, 0.03)
            assert R.same_bits(got, R.ref_batch(orc, kind, st, wp, 3, 0.1, 0.03)), f"n={n} {name} {kind} vs numpy"
            assert R.same_bits(got, R.oracle_ref_batch(orc, kind, st, wp, 3, 0.1, 0.03)), f"n={n} {name} {kind} vs oracle"
            want_x = wp[[R.nearest_index(orc, s[:2], wp) for s in st], 0]
            np.testing.assert_array_equal(got[:, 0, 0], want_x)           # v = 0: the column at the nearest segment


def test_front_axle_on_a_vertex_of_a_collinear_run(ctx, orc):
    """two segments at distance exactly 0: the first one wins through wave_argmin (Stanley), the LDS hand-over (LQR) and block_argmin (references)"""
    wp, st, verts, wb = R.collinear_case()
    ctx.set_waypoints(wp)
    want = np.array(verts) - 1
    assert want[2] == 2 and want[4] == 4
    g = ctx.stanley(st, wheelbase=wb)
    np.testing.assert_array_equal(g["near_idx"], want)
    _check_tracker(g, orc.stanley_batch(st, wp, wheelbase=wb), "collinear stanley")
    g = ctx.lqr(st, np.zeros((len(st), 2)), wheelbase=wb)
    np.testing.assert_array_equal(g["near_idx"], want)
    _check_tracker(g, orc.lqr_batch(st, np.zeros((len(st), 2)), wp, wheelbase=wb), "collinear lqr", lqr=True)
    ms = np.column_stack([wp[verts, 0], wp[verts, 1], np.zeros(len(verts)), np.zeros(len(verts))])
    for kind in ("kmpc", "stmpc"):
        got = _refs(ctx, kind, ms, 3, 0.1, 0.03)
        np.testing.assert_array_equal(got[:, 3 if kind == "stmpc" else 2, 0], wp[want, 2])
        assert R.same_bits(got, R.ref_batch(orc, kind, ms, wp, 3, 0.1, 0.03))


# ---- b. ragged batches ------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batches(ctx, orc):
    rl, st, err = R.ragged_case()
    ctx.set_waypoints(rl)
    full_s = ctx.stanley(st, k_path=5.0)
    full_l = ctx.lqr(st, err)
    want_s = orc.stanley_batch(st, rl, k_path=5.0)
    want_l = orc.lqr_batch(st, err, rl)
    assert np.abs(err).min() > 0 and not np.array_equal(full_l["err"], err)
    for E in R.RAGGED_E:
        gs = ctx.stanley(st[:E], k_path=5.0)
        gl = ctx.lqr(st[:E], err[:E])
        _check_tracker(gs, {k: v[:E] for k, v in want_s.items()}, f"E={E} stanley")
        _check_tracker(gl, {k: v[:E] for k, v in want_l.items()}, f"E={E} lqr", lqr=True)
        for k in ("steer", "speed"):
            assert R.same_bits(gs[k], full_s[k][:E]), (E, "stanley", k)
            assert R.same_bits(gl[k], full_l[k][:E]), (E, "lqr", k)
        assert R.same_bits(gl["err"], full_l["err"][:E]), (E, "lqr err")
        np.testing.assert_array_equal(gs["near_idx"], full_s["near_idx"][:E])
        np.testing.assert_array_equal(gl["near_idx"], full_l["near_idx"][:E])


# ---- c. LQR off the defaults --------------------------------------------------------------------------------------------------------------------------
def _abi_kw(kw):
    kw = dict(kw)
    if "ts" in kw:
        kw["timestep"] = kw.pop("ts")
    return kw


@pytest.mark.parametrize("name", [s[0] for s in R.LQR_PARAM_SETS])
def test_lqr_off_defaults(ctx, orc, name):
    kw = dict(R.LQR_PARAM_SETS)[name]
    rl, st, err = R.lqr_speed_mix()
    ctx.set_waypoints(rl)
    worst = 0.0
    for step in range(3):                                          # three consecutive control steps: the error state carries over
        p = st.copy(); p[:, :2] += 0.05 * step
        g = ctx.lqr(p, err, **_abi_kw(kw))
        w = orc.lqr_batch(p, err, rl, **kw)
        worst = max(worst, float(np.max(np.abs(g["steer"] - w["steer"]) / np.maximum(1.0, np.abs(w["steer"])))))
        print(f"lqr {name} step {step}: worst relative steer difference from the oracle {worst:.3g}, err {float(np.max(np.abs(g['err'] - w['err']))):.3g}")
        _check_tracker(g, w, f"{name} step {step}", lqr=True)
        assert np.isfinite(g["steer"]).all()
        err = g["err"]


def test_lqr_single_raceline_rejects_bad_parameters(ctx):
    rl, st, err = R.lqr_speed_mix()
    ctx.set_waypoints(rl)
    for bad in (dict(timestep=0.0), dict(timestep=-0.01), dict(timestep=float("nan")), dict(wheelbase=0.0), dict(wheelbase=-0.33), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            ctx.lqr(st, err, **bad)
    assert np.isfinite(ctx.lqr(st, err, max_iter=0)["steer"]).all()


# ---- d. Stanley off the defaults ------------------------------------------------------------------------------------------------------------------------
def test_stanley_off_defaults(ctx, orc):
    rl, st, tgt = R.stanley_case()
    ctx.set_waypoints(rl)
    for wb in R.STANLEY_WB:
        for k in R.STANLEY_K:
            g = ctx.stanley(st, wheelbase=wb, k_path=k)
            _check_tracker(g, orc.stanley_batch(st, rl, wheelbase=wb, k_path=k), f"wheelbase={wb} k_path={k}")
            ld = R.stanley_ref(orc, st, rl, wheelbase=wb, k_path=k)                       # the single wrap, in long double
            np.testing.assert_allclose(g["steer"], ld["steer"].astype(np.float64), rtol=0, atol=1e-12)


# ---- e. reference trajectories --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kmpc", "stmpc"])
def test_reference_trajectories(ctx, orc, kind):
    for c in R.ref_cases():
        wp, st, T, dt, dl = c["wp"], c["states"], c["T"], c["dt"], c["dl"]
        ctx.set_waypoints(wp)
        got = _refs(ctx, kind, st, T, dt, dl)
        assert R.same_bits(got, R.ref_batch(orc, kind, st, wp, T, dt, dl, clamp=c["clamp"])), (c["name"], "vs numpy")
        if not c["clamp"] and all(R.in_oracle_window(s, len(wp), T, dt, dl) for s in st):
            assert R.same_bits(got, R.oracle_ref_batch(orc, kind, st, wp, T, dt, dl)), (c["name"], "vs oracle")
        if kind == "stmpc":                                         # rows 2, 5, 6 are +0.0
            assert R.same_bits(got[:, [2, 5, 6], :], np.zeros((len(st), 3, T + 1))), c["name"]
        if c["name"] == "speeds":
            assert R.same_bits(got[0], got[1]) and R.same_bits(got[4], got[5])         # v < 0 as |v|
            for e in (2, 3):                                        # v = 0.0, -0.0: every column is the one at ind
                assert (got[e] == got[e][:, :1]).all()
        if c["name"] == "clamp":
            xr = 0; far = np.abs(st[:, 2]) >= 2.0
            assert far.any() and (got[far, xr, -1] == wp[-1, 0]).all()                  # il = n - 1


def test_kmpc_yaw_fixup_off_returns_the_raw_gather(ctx, orc):
    c = {c["name"]: c for c in R.ref_cases()}["fold"]
    wp, st, T, dt, dl = c["wp"], c["states"], c["T"], c["dt"], c["dl"]
    ctx.set_waypoints(wp)
    on = ctx.kmpc_ref(st, T, dt=dt, dl=dl)
    try:
        ctx.kmpc_set_yaw_fixup(False)
        off = ctx.kmpc_ref(st, T, dt=dt, dl=dl)
        dyn = ctx.stmpc_ref(st, T, dt=dt, dl=dl)                    # the dynamic kernel has no such switch: it still folds, at 5
    finally:
        ctx.kmpc_set_yaw_fixup(True)
    assert R.same_bits(off, R.ref_batch(orc, "kmpc", st, wp, T, dt, dl, fold=False))
    assert R.same_bits(on, R.ref_batch(orc, "kmpc", st, wp, T, dt, dl))
    assert R.same_bits(dyn, R.ref_batch(orc, "stmpc", st, wp, T, dt, dl))
    assert R.same_bits(ctx.kmpc_ref(st, T, dt=dt, dl=dl), on)       # restored
    il = [R.nearest_index(orc, s[:2], wp) for s in st]
    np.testing.assert_array_equal(off[:, 3, 0], wp[il, 3])
    assert not R.same_bits(on[:, 3], off[:, 3]) and not R.same_bits(on[:, 3], dyn[:, 4])   # 4.5 and 5 side by side
