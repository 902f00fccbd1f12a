"""The rivals' prediction with the course's speed profile on the GPU (include/f1p.h "Rivals, predicted with the course's speed profile"):
k_course_time and k_rivals_predict<CourseTime> against the reference of the rule (tests/rivals_profile_ref.py) on the 70-vehicle scene of
tests/rivals_predict_ref.py with speed columns that vary along the courses -- the sweep of M, knots, wrap, track set / raceline and two horizons, the other
two layouts, the default's bytes, the host-array wrapper, a course with a NaN speed, a speed column of zeros, a replaced raceline, another min_speed, E == 1,
the error code -- and Rivals(predict="track", speed="profile") end to end on the three planner classes.  The tolerances are test_gpu_rivals_predict.compare's."""
import ctypes as C
import functools

import numpy as np
import pytest

import rivals_predict_ref as ref
import rivals_profile_ref as pref
import rivals_ref as base
from f1tenth_planning_amd import Rivals, _abi
from f1tenth_planning_amd.runtime import Context, rivals, rivals_predict, rivals_predict_dev, rivals_set_course, rivals_set_groups
from test_gpu_rivals_predict import GROUPS, KN, RIV, _mpc_course, _same, compare, moved, pack

pytestmark = pytest.mark.gpu

R0 = 0.3
E = pref.SCENE_E


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def scene(raceline):
    st, g, tid = pref.scene(raceline)
    return st, g, tid, ([pref.courses()[0]] if raceline else pref.courses())


@functools.lru_cache(maxsize=None)
def want(raceline, layout, M, knots, wrap, hs, hm, min_speed=0.5):
    from oracle import oracle
    oracle.build()
    st, g, tid, cs = scene(raceline)
    r = pref.predict(oracle, pref.as_layout(st, layout), layout, M, R0, cs, tid, hs, hm, knots, True, wrap, min_speed=min_speed, groups=g)
    r["margin"] = pref.knot_margin(r, cs, tid, wrap, min_speed)
    return r


def install(ctx, raceline, cs=None):
    """the scene's courses, races and track ids on the context"""
    st, g, tid, own = scene(raceline)
    if raceline:
        ctx.set_waypoints((cs or own)[0])
    else:
        ctx.set_tracks(cs or own)
    rivals_set_course(ctx, tid)
    rivals_set_groups(ctx, g)


def uninstall(ctx):
    rivals_set_course(ctx, None)
    rivals_set_groups(ctx, None)


def moved_share(a, b, p):
    """the share of the slots p whose (vx, vy) differ by more than 0.05 m/s between a and b"""
    return float((np.abs(a["obs"][..., 2:4] - b["obs"][..., 2:4]).max(axis=2)[p] > 0.05).mean())


def run_case(ctx, raceline, layout, M, knots, wrap, hs=0.8, hm=0.0):
    st4, g, tid, cs = scene(raceline)
    st = pref.as_layout(st4, layout)
    exp = want(raceline, layout, M, knots, wrap, hs, hm)
    assert exp["margin"] >= 1e-6                                     # the scene conditions, for this case's own knots and slots
    assert exp["predicted"].sum() > 0.9 * (exp["idx"] >= 0).sum()
    install(ctx, raceline)
    got = rivals_predict(ctx, st, layout, M, R0, hs, hm, knots, True, wrap, speed="profile")
    con = rivals_predict(ctx, st, layout, M, R0, hs, hm, knots, True, wrap, speed="constant")
    cv = rivals(ctx, st, layout, M, R0)
    uninstall(ctx)
    worst = compare(got, exp, cv, st, layout, cs, tid)
    print("worst |vx, vy| and r error", worst, "(over 1e-11: DESIGN.md 5u has to say so)" if max(worst) > 1e-11 else "", "predicted slots",
          int(exp["predicted"].sum()), "moved share", moved_share(got, con, exp["predicted"]))
    assert moved_share(got, con, exp["predicted"]) > 0.5             # on these courses the profile's prediction is not the constant-speed one
    return got, exp, cv, con


@pytest.mark.parametrize("raceline", [False, True], ids=["tracks", "raceline"])
@pytest.mark.parametrize("h", [(0.8, 0.0), (0.3, 0.4)], ids=["0.8s", "0.3s+0.4m"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "open"])
@pytest.mark.parametrize("knots", [1, 2, 8, 16])
@pytest.mark.parametrize("M", [1, 4, 16])
def test_kernels_equal_the_reference(ctx, M, knots, wrap, h, raceline):
    got, exp, cv, con = run_case(ctx, raceline, ref.XYVYAW, M, knots, wrap, *h)
    for k in ("idx", "pace", "frenet"):                              # only the map from tau to a point changes
        assert got[k].tobytes() == con[k].tobytes(), k
    assert got["obs"][..., :2].tobytes() == con["obs"][..., :2].tobytes()
    if knots == 1:
        assert (got["obs"][..., 4][exp["idx"] >= 0] == R0).all()      # no interior knot: dev = 0


@pytest.mark.parametrize("layout", [ref.POSE, ref.ST7], ids=["pose", "st7"])
def test_other_layouts(ctx, layout):
    run_case(ctx, False, layout, 4, 8, True)


def test_constant_and_the_default_give_the_same_bytes(ctx):
    st, g, tid, cs = scene(False)
    install(ctx, False)
    a = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True)
    p = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")      # (the time table in between changes nothing for the next call)
    b = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="constant")
    c = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed=_abi.RIVALS_SPEED_CONSTANT)
    uninstall(ctx)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert p["obs"].tobytes() != a["obs"].tobytes()


def test_batch_equals_dev(ctx):
    st4, g, tid, cs = scene(False)
    install(ctx, False)
    M = 4
    for layout, nm in ((ref.XYVYAW, "xyvyaw"), (ref.POSE, "pose"), (ref.ST7, "st7")):
        st = pref.as_layout(st4, layout)
        a = rivals_predict(ctx, st, nm, M, R0, 0.3, 0.4, 6, True, False, reach=5.0, min_speed=0.75, speed="profile")
        d_st, d_obs, d_pace, d_idx, d_fr = ctx.to_device(st), ctx.alloc(40 * E * M), ctx.alloc(8 * E), ctx.alloc(4 * E * M), ctx.alloc(24 * E)
        rivals_predict_dev(ctx, d_st, layout, E, M, R0, d_obs, 0.3, 0.4, 6, True, False, d_pace, d_idx, d_fr, reach=5.0, min_speed=0.75, speed="profile")
        b = dict(obs=d_obs.download(np.float64, (E, M, 5)), pace=d_pace.download(np.float64, (E,)), idx=d_idx.download(np.int32, (E, M)),
                 frenet=d_fr.download(np.float64, (E, 3)))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * E * M))
        rivals_predict_dev(ctx, d_st, nm, E, M, R0, d_obs, 0.3, 0.4, 6, True, False, reach=5.0, min_speed=0.75, speed="profile")
        assert d_obs.download(np.float64, (E, M, 5)).tobytes() == a["obs"].tobytes()
        con = rivals_predict(ctx, st, nm, M, R0, 0.3, 0.4, 6, True, False, reach=5.0, min_speed=0.75)
        assert a["obs"].tobytes() != con["obs"].tobytes() and a["idx"].tobytes() == con["idx"].tobytes()
        for buf in (d_st, d_obs, d_pace, d_idx, d_fr):
            buf.free()
    uninstall(ctx)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_course_with_one_non_finite_speed_falls_back_to_constant_speed(ctx, bad):
    """one speed of the clockwise circle is not finite: the course is usable but not profile-usable.  The slots that hold its vehicles are bit-equal to the
    speed = "constant" call's, the slots that hold the other courses' vehicles to the call on the sound courses."""
    st, g, tid, cs = scene(False)
    broken = [c.copy() for c in cs]
    broken[1][77, 2] = bad
    install(ctx, False)
    clean = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")
    install(ctx, False, broken)
    got = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")
    con = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="constant")
    install(ctx, False)
    again = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")      # the sound set again: the flag is rebuilt with the table
    uninstall(ctx)
    live = got["idx"] >= 0
    on_broken = live & (tid[np.maximum(got["idx"], 0)] == 1)
    assert on_broken.sum() > 20 and (live & ~on_broken).sum() > 40
    for k in ("idx", "pace", "frenet"):
        assert got[k].tobytes() == clean[k].tobytes() == con[k].tobytes(), k
    assert got["obs"][on_broken].tobytes() == con["obs"][on_broken].tobytes()
    assert got["obs"][~on_broken].tobytes() == clean["obs"][~on_broken].tobytes()
    assert got["obs"][on_broken].tobytes() != clean["obs"][on_broken].tobytes() and np.isfinite(got["obs"]).all()
    assert again["obs"].tobytes() == clean["obs"].tobytes()


def test_speed_column_of_zeros_is_the_floor(ctx):
    """c_k = min_speed on every segment: finite slots, the bits of a speed column that is min_speed everywhere (0.5 (0.5 + 0.5) is 0.5) -- and, the rule
    with a constant column, the constant-speed prediction of rivals at |v_j| scaled by |v_j| / 0.5: for a standing vehicle both stand"""
    st, g, tid, cs = scene(False)
    install(ctx, False, [pref.with_speed(c, 0.0) for c in cs])
    got = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")
    install(ctx, False, [pref.with_speed(c, -0.0) for c in cs])
    neg = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")
    install(ctx, False, [pref.with_speed(c, 0.5) for c in cs])
    flat = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True, speed="profile")
    cv = rivals(ctx, st, 0, 4, R0)
    uninstall(ctx)
    assert np.isfinite(got["obs"]).all() and (got["idx"] >= 0).sum() > 200
    for k in got:
        assert got[k].tobytes() == flat[k].tobytes() == neg[k].tobytes(), k
    standing = np.isin(got["idx"], [4, 9])
    assert standing.sum() > 0 and (got["obs"][standing][:, 2:4] == 0.0).all() and (got["obs"][standing][:, 4] == R0).all()
    assert got["obs"][..., :2].tobytes() == cv["obs"][..., :2].tobytes()


def test_replaced_raceline_rebuilds_the_time_table(ctx):
    """the same polyline with another speed column, then a longer raceline (the table grows), then the first again: its first answer, bit for bit"""
    from oracle import oracle
    oracle.build()
    st, g, tid, cs = scene(True)
    install(ctx, True)
    a = rivals_predict(ctx, st, 0, 4, R0, 0.8, speed="profile")
    cva = rivals(ctx, st, 0, 4, R0)
    compare(a, want(True, 0, 4, 8, True, 0.8, 0.0), cva, st, 0, cs, None)
    n = cs[0].shape[0]
    other = pref.with_speed(cs[0], 2.0 + 1.2 * np.cos(4.0 * np.pi * np.arange(n) / (n - 1)))
    exp = pref.predict(oracle, st, 0, 4, R0, [other], None, 0.8, 0.0, 8, True, True, groups=g)
    assert pref.knot_margin(exp, [other], None, True) >= 1e-6
    ctx.set_waypoints(other)
    b = rivals_predict(ctx, st, 0, 4, R0, 0.8, speed="profile")
    compare(b, exp, cva, st, 0, [other], None)
    assert a["obs"].tobytes() != b["obs"].tobytes()                    # (the arc table is the same: only the time table can tell the two apart)
    m = 301
    line = pref.with_speed(ref.circle(2.5, m, centre=(0.3, -0.2)), 2.5 + 1.0 * np.sin(2.0 * np.pi * np.arange(m) / (m - 1)))
    line[-1, 2] = line[0, 2]
    st2, g2, _ = ref.scene(True, 1, line)
    exp2 = pref.predict(oracle, st2, 0, 4, R0, [line], None, 0.8, 0.0, 8, True, True, groups=g2)
    assert pref.knot_margin(exp2, [line], None, True) >= 1e-6
    ctx.set_waypoints(line)
    c = rivals_predict(ctx, st2, 0, 4, R0, 0.8, speed="profile")
    compare(c, exp2, rivals(ctx, st2, 0, 4, R0), st2, 0, [line], None)
    ctx.set_waypoints(cs[0])
    d = rivals_predict(ctx, st, 0, 4, R0, 0.8, speed="profile")
    uninstall(ctx)
    for k in a:
        assert a[k].tobytes() == d[k].tobytes(), k


@pytest.mark.parametrize("raceline", [False, True], ids=["tracks", "raceline"])
def test_another_min_speed_rebuilds_the_time_table(ctx, raceline):
    """min_speed is the floor of the segment speeds: 2.0 floors a third of the circle (3.0 + 1.5 sin 3a goes down to 1.5), half of the clockwise circle and the
    L's corner.  The same courses, the call's min_speed alone changes -- and back"""
    st, g, tid, cs = scene(raceline)
    lo, hi = want(raceline, 0, 4, 8, True, 0.8, 0.0), want(raceline, 0, 4, 8, True, 0.8, 0.0, 2.0)
    assert lo["margin"] >= 1e-6 and hi["margin"] >= 1e-6
    install(ctx, raceline)
    a = rivals_predict(ctx, st, 0, 4, R0, 0.8, speed="profile")
    b = rivals_predict(ctx, st, 0, 4, R0, 0.8, min_speed=2.0, speed="profile")
    cvb = rivals(ctx, st, 0, 4, R0, min_speed=2.0)
    c = rivals_predict(ctx, st, 0, 4, R0, 0.8, speed="profile")
    cva = rivals(ctx, st, 0, 4, R0)
    uninstall(ctx)
    compare(a, lo, cva, st, 0, cs, tid)
    compare(b, hi, cvb, st, 0, cs, tid)
    assert a["obs"].tobytes() != b["obs"].tobytes() and lo["obs"].tobytes() != hi["obs"].tobytes()
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_e_equals_one(ctx):
    ctx.set_waypoints(pref.courses()[0])
    for layout, n in ((ref.XYVYAW, 4), (ref.POSE, 4), (ref.ST7, 7)):
        st = np.arange(1.0, n + 1.0)[None] * 0.25
        got = rivals_predict(ctx, st, layout, 3, R0, 0.8, speed="profile")
        assert (got["idx"] == -1).all() and (got["obs"] == base.EMPTY).all() and np.isfinite(got["frenet"]).all()
        assert got["pace"][0] == 1.0 / max(abs(base.columns(st, layout)[2][0]), 0.5)
    ctx.set_tracks(pref.courses())
    rivals_set_course(ctx, [2])
    got = rivals_predict(ctx, np.array([[10.2, 2.6, 1.0, 0.0]]), 0, 16, R0, 0.8, speed="profile")
    rivals_set_course(ctx, None)
    assert (got["idx"] == -1).all() and got["frenet"][0, 0] == 7.0


def test_unknown_speed_is_einval_and_nothing_is_launched():
    with Context(0) as ctx:
        Ee, M = 6, 2
        st = scene(True)[0][:Ee].copy()
        ctx.set_waypoints(pref.courses()[0])
        d_st, d_obs = ctx.to_device(st), ctx.alloc(40 * Ee * M)
        ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * Ee * M))
        obs, pace, idx, fr = np.full((Ee, M, 5), 7.0), np.full(Ee, 7.0), np.full((Ee, M), 7, np.int32), np.full((Ee, 3), 7.0)
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

        def call(dev, speed):
            pr = C.byref(_abi.rivals_predict(0.8, 0.0, 8, True, True, speed))
            if dev:
                return ctx.lib.f1p_rivals_predict_dev(ctx.h, d_st.ptr, 0, Ee, M, 0.3, np.inf, 0.5, pr, d_obs.ptr, None, None, None)
            return ctx.lib.f1p_rivals_predict_batch(ctx.h, ptr(st), 0, Ee, M, 0.3, np.inf, 0.5, pr, ptr(obs), ptr(pace), ptr(idx), ptr(fr))
        for dev in (True, False):
            for speed in (2, -1, 256, 2 ** 31 - 1):
                assert call(dev, speed) == _abi.F1P_EINVAL, (dev, speed)
                assert b"rivals: speed" in ctx.lib.f1p_last_error(ctx.h)
        with pytest.raises(ValueError, match="rivals: speed"):           # (the runtime raises F1P_EINVAL as a ValueError)
            rivals_predict(ctx, st, 0, M, 0.3, 0.8, speed=2)
        ctx.sync()
        assert (d_obs.download(np.uint8, (40 * Ee * M,)) == 0x5A).all()   # nothing was launched
        assert (obs == 7.0).all() and (pace == 7.0).all() and (idx == 7).all() and (fr == 7.0).all()
        for speed in (0, 1):                                         # ... and the two modes run
            assert call(True, speed) == _abi.F1P_OK and call(False, speed) == _abi.F1P_OK
            assert d_obs.download(np.float64, (Ee, M, 5)).tobytes() == obs.tobytes() and (idx >= 0).all() and np.isfinite(fr).all()
        d_st.free(); d_obs.free()


# ---- end to end: Rivals(predict="track", speed="profile") on the three classes ----------------------------------------------------------------------
def profile_circles():
    """test_gpu_rivals_predict's two circles of radius 2 with speed columns that vary along them"""
    a = 2.0 * np.pi * np.arange(257) / 256
    v0, v1 = 3.0 + 1.5 * np.sin(3.0 * a), 2.5 + 1.0 * np.cos(2.0 * a)
    v0[-1], v1[-1] = v0[0], v1[0]
    return [pref.with_speed(ref.circle(), v0), pref.with_speed(ref.circle(2.0, 257, centre=(0.05, 0.0)), v1)]


def _end_to_end(ctx, make, to_states, layout, horizon, plan, tracks=False):
    """A plans with Rivals(predict="track", speed="profile"), B with planner.obstacles = runtime.rivals_predict(..., speed="profile")["obs"] formed with the
    planner's own horizon, two consecutive steps with moved states; every output bit for bit.  The slots differ from the constant-speed ones."""
    A, B = make(), make()
    A.rivals = Rivals(groups=GROUPS, predict="track", speed="profile", **RIV, **KN)
    rivals_set_groups(ctx, GROUPS)
    if tracks:
        ctx.set_tracks(profile_circles())
        rivals_set_course(ctx, pack()["tid"])
    else:
        ctx.set_waypoints(profile_circles()[0])
        rivals_set_course(ctx, None)
    for step, p in enumerate((pack(), moved(pack()))):
        st = to_states(p)
        kw = dict(reach=RIV["reach"])
        r = rivals_predict(ctx, st, layout, RIV["count"], RIV["radius"], horizon[0], horizon[1], KN["knots"], True, True, speed="profile", **kw)
        con = rivals_predict(ctx, st, layout, RIV["count"], RIV["radius"], horizon[0], horizon[1], KN["knots"], True, True, **kw)
        live = r["idx"] >= 0
        assert live[:, 0].all() and np.isfinite(r["frenet"]).all() and np.isfinite(r["obs"]).all()
        assert r["obs"][live].tobytes() != con["obs"][live].tobytes() and r["idx"].tobytes() == con["idx"].tobytes()
        a = {k: np.array(v) for k, v in plan(A, st).items()}
        B.obstacles = r["obs"]
        _same(a, plan(B, st), f"step {step}")
    rivals_set_groups(ctx, None)
    rivals_set_course(ctx, None)


def test_kmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    cfg = dict(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2)

    def make():
        return KMPCPlanner(waypoints=_mpc_course(profile_circles()[0]), config=mpc_config(**cfg))
    c = mpc_config(**cfg)
    to_states = lambda p: np.column_stack([p["x"], p["y"], p["v"], p["psi"]])  # noqa: E731
    _end_to_end(ctx, make, to_states, ref.XYVYAW, (float(c.TK) * float(c.DTK), 0.0), lambda p, st: p.plan_batch(st))
    tracks = [_mpc_course(t) for t in profile_circles()]
    _end_to_end(ctx, make, to_states, ref.XYVYAW, (float(c.TK) * float(c.DTK), 0.0),
                lambda p, st: p.plan_batch(st, tracks=tracks, track_ids=pack()["tid"]), tracks=True)


def test_stmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    cfg = dict(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2, COLLISION_SUBSTEPS_K=2)

    def make():
        return STMPCPlanner(waypoints=_mpc_course(profile_circles()[0]), config=mpc_config(**cfg))

    def to_states(p):
        z = np.zeros(len(p["x"]))
        return np.column_stack([p["x"], p["y"], z, p["v"], p["psi"] - 0.01, z, z + 0.01])      # (heading = yaw + beta)
    c = mpc_config(**cfg)
    H = max(float(c.T) * float(c.DT), float(c.TK) * float(c.DTK))
    _end_to_end(ctx, make, to_states, ref.ST7, (H, 0.0), lambda p, st: p.plan_batch(st))


def test_lattice_planner_end_to_end(ctx):
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    la = np.linspace(0.6, 3.0, 8)

    def make():
        p = LatticePlanner(waypoints=profile_circles()[0], device=0)
        p.configure(lookahead_distances=la, widths=np.linspace(-1.0, 1.0, 5), num_stations=20)
        return p
    to_states = lambda p: np.column_stack([p["x"], p["y"], p["psi"], p["v"]])  # noqa: E731
    horizon = (0.0, float(max(list(la))))
    _end_to_end(ctx, make, to_states, ref.POSE, horizon, lambda p, st: p.plan_batch(st))
    tracks = profile_circles()
    _end_to_end(ctx, make, to_states, ref.POSE, horizon, lambda p, st: p.plan_batch(st, tracks=tracks, track_ids=pack()["tid"]), tracks=True)
