"""The rivals' prediction along their courses on the GPU (include/f1p.h "Rivals, predicted along the course"): k_course_arc,
k_rivals_frenet and k_rivals_predict against the numpy reference of the rule (tests/rivals_predict_ref.py) on its 70-vehicle scene -- three races and two
ungrouped egos on a circle, a clockwise circle and an open L, once as a track set with the ids mixed and once with the circle as the raceline --, every
fallback cause, the host-array wrapper, a replaced raceline, the error codes, E == 1; and Rivals(predict="track") end to end on the three planner classes."""
import ctypes as C
import functools

import numpy as np
import pytest

import rivals_predict_ref as ref
import rivals_ref as base
from f1tenth_planning_amd import Rivals, _abi
from f1tenth_planning_amd.runtime import (Context, F1PError, rivals, rivals_predict, rivals_predict_dev, rivals_set_course, rivals_set_groups)

pytestmark = pytest.mark.gpu

R0 = 0.3
E = ref.SCENE_E


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def scene(raceline):
    st, g, tid = ref.scene(raceline)
    return st, g, tid, ([ref.courses()[0]] if raceline else ref.courses())


@functools.lru_cache(maxsize=None)
def want(raceline, layout, M, knots, wrap, hs, hm):
    from oracle import oracle
    oracle.build()
    st, g, tid, cs = scene(raceline)
    r = ref.predict(oracle, ref.as_layout(st, layout), layout, M, R0, cs, tid, hs, hm, knots, True, wrap, groups=g)
    r["margin"] = ref.knot_margin(r, cs, tid, wrap)
    return r


def install(ctx, raceline):
    """the scene's courses, races and track ids on the context"""
    st, g, tid, cs = scene(raceline)
    if raceline:
        ctx.set_waypoints(cs[0])
    else:
        ctx.set_tracks(cs)
    rivals_set_course(ctx, tid)
    rivals_set_groups(ctx, g)


def uninstall(ctx):
    rivals_set_course(ctx, None)
    rivals_set_groups(ctx, None)


def compare(got, exp, cv, st, layout, cs, tid):
    """idx exact; x, y, the empty slots and pace bit-equal to f1p_rivals_dev's (cv), and so is every slot the rule leaves at constant velocity; the Frenet
    records' s0 and d within 1e-12 max(1, L), dir exact, the same NaN rows; vx, vy within 1e-9 max(1, |v_j|) and r within 1e-9 (operands below 1e2 and
    H >= 0.1: the true error is a few 1e-13, the margin absorbs contraction and the device sincos)"""
    np.testing.assert_array_equal(got["idx"], exp["idx"])
    np.testing.assert_array_equal(got["idx"], cv["idx"])
    assert got["obs"][..., :2].tobytes() == cv["obs"][..., :2].tobytes() and got["pace"].tobytes() == cv["pace"].tobytes()
    assert got["obs"][..., :2].tobytes() == exp["obs"][..., :2].tobytes() and got["pace"].tobytes() == exp["pace"].tobytes()
    empty = exp["idx"] < 0
    assert got["obs"][empty].tobytes() == cv["obs"][empty].tobytes() == exp["obs"][empty].tobytes()
    keep = ~exp["predicted"]
    assert got["obs"][keep].tobytes() == cv["obs"][keep].tobytes()
    fr, efr = got["frenet"], exp["frenet"]
    assert (np.isnan(fr) == np.isnan(efr)).all()
    L = np.array([ref.arc_table(cs[0 if tid is None else min(max(int(t), 0), len(cs) - 1)])[1][-1] for t in (np.zeros(len(fr)) if tid is None else tid)])
    live = ~np.isnan(efr[:, 0])
    assert live.sum() > 0.8 * len(fr)
    tolf = 1e-12 * np.maximum(1.0, L[live])
    assert (np.abs(fr[live, 0] - efr[live, 0]) <= tolf).all() and (np.abs(fr[live, 1] - efr[live, 1]) <= tolf).all()
    assert (fr[live, 2] == efr[live, 2]).all()
    p = exp["predicted"]
    v = base.columns(st, layout)[2]
    tol = 1e-9 * np.maximum(1.0, np.abs(v[np.maximum(exp["idx"], 0)]))
    for c in (2, 3):
        err = np.abs(got["obs"][..., c] - exp["obs"][..., c])
        assert np.isfinite(got["obs"][..., c][p]).all() and not (err[p] > tol[p]).any(), (c, err[p].max())
    errr = np.abs(got["obs"][..., 4] - exp["obs"][..., 4])
    assert not (errr[p] > 1e-9).any(), errr[p].max()
    return float(np.abs(got["obs"][..., 2:4] - exp["obs"][..., 2:4])[p].max()), float(errr[p].max())


def run_case(ctx, raceline, layout, M, knots, wrap, hs=0.8, hm=0.0):
    st4, g, tid, cs = scene(raceline)
    st = ref.as_layout(st4, layout)
    exp = want(raceline, layout, M, knots, wrap, hs, hm)
    assert exp["margin"] >= 1e-6                                     # the scene condition, for this case's own knots
    install(ctx, raceline)
    got = rivals_predict(ctx, st, layout, M, R0, hs, hm, knots, True, wrap)
    cv = rivals(ctx, st, layout, M, R0)
    uninstall(ctx)
    worst = compare(got, exp, cv, st, layout, cs, tid)
    print("worst |vx, vy| and r error", worst, "predicted slots", int(exp["predicted"].sum()))
    assert exp["predicted"].sum() > 0.9 * (exp["idx"] >= 0).sum()
    return got, exp, cv


def test_scene_properties():
    """the condition of tests/test_rivals_predict_host.py's scene test, here for the shapes this file sweeps"""
    from oracle import oracle
    oracle.build()
    from test_rivals_predict_host import scene_margin
    for raceline in (False, True):
        assert scene_margin(oracle, raceline) >= 1e-6
    st, g, tid, _ = scene(False)
    assert st.shape[0] == 70 and max((g == k).sum() for k in range(3)) > 16 and sorted(set(tid.tolist())) == [0, 1, 2]


@pytest.mark.parametrize("raceline", [False, True], ids=["tracks", "raceline"])
@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "open"])
@pytest.mark.parametrize("knots", [1, 2, 8, 16])
@pytest.mark.parametrize("M", [1, 4, 16])
def test_kernels_equal_the_reference(ctx, M, knots, wrap, raceline):
    got, exp, cv = run_case(ctx, raceline, ref.XYVYAW, M, knots, wrap)
    if knots == 1:
        assert (got["obs"][..., 4][exp["idx"] >= 0] == R0).all()      # no interior knot: dev = 0
    if knots == 8 and M == 4:
        moved = np.abs(got["obs"][..., 2:4] - cv["obs"][..., 2:4])[exp["predicted"]]
        assert (moved > 0.05).mean() > 0.5                           # on these courses the prediction is not the constant-velocity one


@pytest.mark.parametrize("layout", [ref.POSE, ref.ST7], ids=["pose", "st7"])
def test_other_layouts(ctx, layout):
    run_case(ctx, False, layout, 4, 8, True)


@pytest.mark.parametrize("raceline", [False, True], ids=["tracks", "raceline"])
def test_horizon_from_the_pace(ctx, raceline):
    """horizon_m > 0: H_i = 0.1 + 0.5 pace_i differs from ego to ego (0.18 .. 1.1 s)"""
    got, exp, cv = run_case(ctx, raceline, ref.XYVYAW, 16, 16, True, hs=0.1, hm=0.5)
    assert len(set(np.round(exp["pace"], 6).tolist())) > 50


def test_no_inflation_keeps_the_radius_bits(ctx):
    st, g, tid, cs = scene(False)
    install(ctx, False)
    a = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True)
    b = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, False, True)
    uninstall(ctx)
    assert a["obs"][..., :4].tobytes() == b["obs"][..., :4].tobytes() and a["frenet"].tobytes() == b["frenet"].tobytes()
    assert (b["obs"][..., 4][b["idx"] >= 0] == R0).all() and (a["obs"][..., 4][a["idx"] >= 0] >= R0).all()
    assert (a["obs"][..., 4] > R0 + 0.01).sum() > 20


def test_batch_equals_dev(ctx):
    st4, g, tid, cs = scene(False)
    install(ctx, False)
    M = 4
    for layout, nm in ((ref.XYVYAW, "xyvyaw"), (ref.POSE, "pose"), (ref.ST7, "st7")):
        st = ref.as_layout(st4, layout)
        a = rivals_predict(ctx, st, nm, M, R0, 0.3, 0.4, 6, True, False, reach=5.0, min_speed=0.75)
        d_st, d_obs, d_pace, d_idx, d_fr = ctx.to_device(st), ctx.alloc(40 * E * M), ctx.alloc(8 * E), ctx.alloc(4 * E * M), ctx.alloc(24 * E)
        rivals_predict_dev(ctx, d_st, layout, E, M, R0, d_obs, 0.3, 0.4, 6, True, False, d_pace, d_idx, d_fr, reach=5.0, min_speed=0.75)
        b = dict(obs=d_obs.download(np.float64, (E, M, 5)), pace=d_pace.download(np.float64, (E,)), idx=d_idx.download(np.int32, (E, M)),
                 frenet=d_fr.download(np.float64, (E, 3)))
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * E * M))
        rivals_predict_dev(ctx, d_st, nm, E, M, R0, d_obs, 0.3, 0.4, 6, True, False, reach=5.0, min_speed=0.75)     # pace, idx and frenet are optional
        assert d_obs.download(np.float64, (E, M, 5)).tobytes() == a["obs"].tobytes()
        for buf in (d_st, d_obs, d_pace, d_idx, d_fr):
            buf.free()
    uninstall(ctx)


def test_every_fallback_cause_keeps_the_constant_velocity_bits(ctx):
    """non-finite x, v and heading, |v| H >= 1e9, track ids outside the set, a course with a zero-length segment, one with an infinite and one with a NaN
    coordinate, and a NaN pace (H_i): the slots that list such a vehicle, or belong to such an ego, are f1p_rivals_dev's bits; everything else is predicted.
    The vehicle with the NaN position still blocks its race, and only its race."""
    from oracle import oracle
    oracle.build()
    st, g, tid, cs = scene(False)
    st, tid = st.copy(), tid.copy()
    dup = cs[0].copy(); dup[9] = dup[8]
    inf = cs[1].copy(); inf[20, 0] = np.inf
    nan = cs[2].copy(); nan[2, 1] = np.nan
    cs = cs + [dup, inf, nan]
    race1 = np.nonzero(g == 1)[0]
    bad = int(race1[3])
    cause = {bad: "x nan", int(race1[7]): "v nan: its own H is NaN", 2: "v inf", 5: "h nan", 8: "h inf", 11: "v H huge", 14: "id high", 20: "id low", 26: "zero-length",
             29: "L inf", 32: "L nan", 35: "y inf"}
    assert len(cause) == 12 and 36 not in cause and 23 not in cause
    st[bad, 0] = np.nan
    st[int(race1[7]), 2] = np.nan
    st[2, 2] = np.inf; st[5, 3] = np.nan; st[8, 3] = -np.inf; st[11, 2] = 2e9; st[35, 1] = np.inf
    tid[14] = 6; tid[20] = -1; tid[26] = 3; tid[29] = 4; tid[32] = 5
    with np.errstate(all="ignore"):
        exp = ref.predict(oracle, st, 0, 4, R0, cs, tid, 0.8, 0.0, 8, True, True, groups=g)
    own_cause = sorted(k for k in cause if k != 11)                  # (|v| H depends on the ego's horizon: that vehicle has a record)
    assert np.isnan(exp["frenet"][own_cause]).all() and np.isnan(exp["frenet"][:, 0]).sum() == len(cause) - 1
    ctx.set_tracks(cs)
    rivals_set_course(ctx, tid)
    rivals_set_groups(ctx, g)
    got = rivals_predict(ctx, st, 0, 4, R0, 0.8, 0.0, 8, True, True)
    cv = rivals(ctx, st, 0, 4, R0)
    clean_st = ref.scene(False)[0]
    clean = rivals_predict(ctx, clean_st, 0, 4, R0, 0.8, 0.0, 8, True, True)
    # a horizon from the pace: the NaN-speed ego's H is NaN whatever horizon_s
    got_m = rivals_predict(ctx, st, 0, 4, R0, 0.1, 0.5, 8, True, True)
    uninstall(ctx)
    ctx.set_tracks(ref.courses())
    compare(got, exp, cv, st, 0, cs, tid)
    lists_bad = np.isin(got["idx"], sorted(cause))
    own = np.zeros_like(lists_bad); own[int(race1[7])] = True
    assert lists_bad.sum() > 20
    assert got["obs"][lists_bad | own].tobytes() == cv["obs"][lists_bad | own].tobytes()
    still = np.isin(got["idx"], own_cause) | own                     # (H_i = 0.1 + 0.5 pace_i can be short enough for the vehicle at 2e9 m/s)
    assert got_m["obs"][still].tobytes() == cv["obs"][still].tobytes()
    fast = (got["idx"] == 11) & ~own
    H = 0.1 + 0.5 * got_m["pace"][:, None]
    assert fast.sum() > 0 and (got_m["obs"][fast & (2e9 * H >= 1e9)].tobytes() == cv["obs"][fast & (2e9 * H >= 1e9)].tobytes())
    assert (exp["predicted"] == ~(lists_bad | own | (got["idx"] < 0))).all()
    others = race1[race1 != bad]
    assert (got["idx"][others, 0] == bad).all() and np.isnan(got["obs"][others, 0]).any(axis=1).all()
    rest = np.nonzero((g != 1))[0]
    rest = rest[~(lists_bad | own)[rest].any(axis=1) & ~np.isin(rest, sorted(cause))]     # sound egos of the other races that list no broken vehicle
    assert rest.size > 10
    for k in ("obs", "idx", "pace"):
        assert got[k][rest].tobytes() == clean[k][rest].tobytes(), k


def test_replaced_raceline_rebuilds_the_arc_table(ctx):
    from oracle import oracle
    oracle.build()
    st, g, tid, cs = scene(True)
    install(ctx, True)
    a = rivals_predict(ctx, st, 0, 4, R0, 0.8)
    compare(a, want(True, 0, 4, 8, True, 0.8, 0.0), rivals(ctx, st, 0, 4, R0), st, 0, cs, None)
    line = ref.circle(2.5, 301, centre=(0.3, -0.2))                  # more points: the table grows
    st2, g2, _ = ref.scene(True, 1, line)
    exp = ref.predict(oracle, st2, 0, 4, R0, [line], None, 0.8, 0.0, 8, True, True, groups=g2)
    assert ref.knot_margin(exp, [line], None, True) >= 1e-6
    ctx.set_waypoints(line)
    b = rivals_predict(ctx, st2, 0, 4, R0, 0.8)
    compare(b, exp, rivals(ctx, st2, 0, 4, R0), st2, 0, [line], None)
    ctx.set_waypoints(cs[0])                                          # ... and shrinks back: the first answer, bit for bit
    c = rivals_predict(ctx, st, 0, 4, R0, 0.8)
    uninstall(ctx)
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_e_equals_one(ctx):
    ctx.set_waypoints(ref.courses()[0])
    for layout, n in ((ref.XYVYAW, 4), (ref.POSE, 4), (ref.ST7, 7)):
        st = np.arange(1.0, n + 1.0)[None] * 0.25
        got = rivals_predict(ctx, st, layout, 3, R0, 0.8)
        assert (got["idx"] == -1).all() and (got["obs"] == base.EMPTY).all() and np.isfinite(got["frenet"]).all()
        assert got["pace"][0] == 1.0 / max(abs(base.columns(st, layout)[2][0]), 0.5)
    ctx.set_tracks(ref.courses())
    rivals_set_course(ctx, [2])
    got = rivals_predict(ctx, np.array([[10.2, 2.6, 1.0, 0.0]]), 0, 16, R0, 0.8)
    rivals_set_course(ctx, None)
    assert (got["idx"] == -1).all() and got["frenet"][0, 0] == 7.0


def test_error_codes_and_nothing_launched():
    with Context(0) as ctx:
        Ee, M = 6, 2
        st = scene(True)[0][:Ee].copy()
        d_st, d_obs = ctx.to_device(st), ctx.alloc(40 * Ee * M)
        ctx.lib.f1p_memset(ctx.h, d_obs.ptr, 0x5A, C.c_size_t(40 * Ee * M))
        obs, pace, idx, fr = np.full((Ee, M, 5), 7.0), np.full(Ee, 7.0), np.full((Ee, M), 7, np.int32), np.full((Ee, 3), 7.0)
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        nan = float("nan")
        good = dict(layout=0, E=Ee, M=M, radius=0.3, reach=np.inf, min_speed=0.5, states=True, obs=True, hs=0.8, hm=0.0, knots=8, pr=True)
        bad = [dict(layout=3), dict(layout=-1), dict(M=0), dict(M=17), dict(radius=-0.1), dict(radius=nan), dict(reach=-1.0), dict(reach=nan),
               dict(min_speed=0.0), dict(min_speed=-1.0), dict(min_speed=nan), dict(states=False), dict(obs=False), dict(E=0),
               dict(knots=0), dict(knots=17), dict(knots=-3), dict(hs=-0.1), dict(hs=nan), dict(hm=-0.1), dict(hm=nan), dict(hs=0.0, hm=0.0), dict(pr=False)]

        def call(dev, **kw):
            a = dict(good, **kw)
            pr = C.byref(_abi.rivals_predict(a["hs"], a["hm"], a["knots"])) if a["pr"] else None
            if dev:
                return ctx.lib.f1p_rivals_predict_dev(ctx.h, d_st.ptr if a["states"] else None, a["layout"], a["E"], a["M"], a["radius"], a["reach"],
                                                      a["min_speed"], pr, d_obs.ptr if a["obs"] else None, None, None, None)
            return ctx.lib.f1p_rivals_predict_batch(ctx.h, ptr(st) if a["states"] else None, a["layout"], a["E"], a["M"], a["radius"], a["reach"],
                                                    a["min_speed"], pr, ptr(obs) if a["obs"] else None, ptr(pace), ptr(idx), ptr(fr))
        for dev in (True, False):
            assert call(dev) == _abi.F1P_ESTATE                      # no raceline yet
            assert b"raceline" in ctx.lib.f1p_last_error(ctx.h)
        ctx.set_waypoints(ref.courses()[0])
        for dev in (True, False):
            for kw in bad:
                assert call(dev, **kw) == _abi.F1P_EINVAL, (dev, kw)
                assert b"rivals" in ctx.lib.f1p_last_error(ctx.h)
        rivals_set_course(ctx, np.zeros(Ee, np.int32))               # courses of a track set that is not there
        for dev in (True, False):
            assert call(dev) == _abi.F1P_ESTATE
            assert b"f1p_set_track_set" in ctx.lib.f1p_last_error(ctx.h)
        ctx.set_tracks(ref.courses())
        rivals_set_course(ctx, np.zeros(Ee + 1, np.int32))           # the courses of another E
        for dev in (True, False):
            assert call(dev) == _abi.F1P_ESTATE
            assert b"f1p_rivals_set_course" in ctx.lib.f1p_last_error(ctx.h)
        with pytest.raises(F1PError) as ei:
            rivals_predict(ctx, st, 0, M, 0.3, 0.8)
        assert ei.value.code == _abi.F1P_ESTATE
        assert ctx.lib.f1p_rivals_set_course(ctx.h, ptr(np.zeros(1, np.int32)), 0) == _abi.F1P_EINVAL
        assert call(True) == _abi.F1P_ESTATE                         # a refused set leaves the courses as they were
        rivals_set_course(ctx, None)
        rivals_set_groups(ctx, np.zeros(Ee + 1, np.int32))           # what f1p_rivals_dev rejects for its state
        assert call(True) == _abi.F1P_ESTATE and b"f1p_rivals_set_groups" in ctx.lib.f1p_last_error(ctx.h)
        rivals_set_groups(ctx, None)
        ctx.sync()
        assert (d_obs.download(np.uint8, (40 * Ee * M,)) == 0x5A).all()   # nothing was launched
        assert (obs == 7.0).all() and (pace == 7.0).all() and (idx == 7).all() and (fr == 7.0).all()
        assert call(True) == _abi.F1P_OK and call(False) == _abi.F1P_OK  # ... and with everything in order the same calls run
        assert d_obs.download(np.float64, (Ee, M, 5)).tobytes() == obs.tobytes() and (idx >= 0).all() and np.isfinite(fr).all()
        d_st.free(); d_obs.free()


# ---- end to end: Rivals(predict="track") on the three classes -----------------------------------------------------------------------------------
E2E, RACES = 48, 6
GROUPS = ((np.arange(E2E) % RACES) * 10 + 3).astype(np.int32)      # six races of 8, interleaved over the batch
RIV = dict(count=3, radius=0.45, reach=6.0)
KN = dict(knots=6, inflate=True, wrap=True)


@functools.lru_cache(maxsize=None)
def pack():
    """48 vehicles on the circle of radius 2, six packs of eight spread over it: in every pack a fast vehicle closes in on a slower one ahead of it ->
    dict(x, y, psi, v, tid): tid puts the odd packs on a second circle of the same radius, 0.05 m to the side"""
    c = ref.circle()
    L = ref.arc_table(c)[1][-1]
    off = np.cumsum([0.0, 0.5, 0.7, 0.5, 0.8, 0.5, 0.9, 0.5])
    speed = np.array([5.0, 2.5, 5.0, 3.0, 4.0, 2.5, 5.0, 3.0])
    x, y, psi, v = (np.empty(E2E) for _ in range(4))
    for e in range(E2E):
        r, m = e % RACES, e // RACES
        a = ((r * L / RACES + off[m] + 0.013) % L) / 2.0
        lat = 0.1 if r == 1 else 0.0
        x[e], y[e], psi[e], v[e] = (2.0 - lat) * np.cos(a), (2.0 - lat) * np.sin(a), a + np.pi / 2, speed[m]
    return dict(x=x, y=y, psi=psi, v=v, tid=(np.arange(E2E) % RACES % 2).astype(np.int32))


def circles():
    return [ref.circle(), ref.circle(2.0, 257, centre=(0.05, 0.0))]


def moved(p, dt=0.05):
    a = np.arctan2(p["y"], p["x"]) + p["v"] * dt / 2.0
    r = np.hypot(p["x"], p["y"])
    return dict(p, x=r * np.cos(a), y=r * np.sin(a), psi=a + np.pi / 2)


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _end_to_end(ctx, make, to_states, layout, horizon, plan, tracks=None):
    """A plans with Rivals(predict="track"), B with planner.obstacles = runtime.rivals_predict(...)["obs"] formed with the planner's own horizon, two
    consecutive steps with moved states; every output bit for bit.  The slots differ from the constant-velocity ones on the circle."""
    A, B = make(), make()
    A.rivals = Rivals(groups=GROUPS, predict="track", **RIV, **KN)
    rivals_set_groups(ctx, GROUPS)
    if tracks is None:
        ctx.set_waypoints(ref.circle())
        rivals_set_course(ctx, None)
    else:
        ctx.set_tracks(circles())
        rivals_set_course(ctx, pack()["tid"])
    outs = []
    for step, p in enumerate((pack(), moved(pack()))):
        st = to_states(p)
        r = rivals_predict(ctx, st, layout, RIV["count"], RIV["radius"], horizon[0], horizon[1], KN["knots"], True, True, reach=RIV["reach"])
        cv = rivals(ctx, st, layout, RIV["count"], RIV["radius"], reach=RIV["reach"])
        live = r["idx"] >= 0
        assert live[:, 0].all() and np.isfinite(r["frenet"]).all()
        assert (np.abs(r["obs"][..., 2:4] - cv["obs"][..., 2:4])[live] > 0.05).mean() > 0.5 and (r["obs"][..., 4][live] > RIV["radius"] + 1e-3).mean() > 0.5
        a = {k: np.array(v) for k, v in plan(A, st).items()}
        B.obstacles = r["obs"]
        b = plan(B, st)
        _same(a, b, f"step {step}")
        outs.append((st, r, a))
    rivals_set_groups(ctx, None)
    rivals_set_course(ctx, None)
    V = make()
    V.rivals = Rivals(groups=GROUPS, **RIV)
    v = {k: np.array(x) for k, x in plan(V, outs[0][0]).items()}
    print("egos whose plan differs from the constant-velocity rivals' plan:", int(sum((outs[0][2][k] != v[k]).reshape(E2E, -1).any(axis=1) for k in ("steer", "speed")).astype(bool).sum()))
    return outs, A, B


def _mpc_course(c):
    return [c[:, 0].copy(), c[:, 1].copy(), c[:, 3].copy(), c[:, 2].copy()]


def test_kmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    cfg = dict(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2)

    def make():
        return KMPCPlanner(waypoints=_mpc_course(ref.circle()), config=mpc_config(**cfg))
    c = mpc_config(**cfg)
    to_states = lambda p: np.column_stack([p["x"], p["y"], p["v"], p["psi"]])  # noqa: E731
    _end_to_end(ctx, make, to_states, ref.XYVYAW, (float(c.TK) * float(c.DTK), 0.0), lambda p, st: p.plan_batch(st))
    tracks = [_mpc_course(t) for t in circles()]
    _end_to_end(ctx, make, to_states, ref.XYVYAW, (float(c.TK) * float(c.DTK), 0.0),
                lambda p, st: p.plan_batch(st, tracks=tracks, track_ids=pack()["tid"]), tracks=True)


def test_stmpc_planner_end_to_end(ctx):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    cfg = dict(N_ROLLOUTS=128, SEED=5, COLLISION_SUBSTEPS=2, COLLISION_SUBSTEPS_K=2)

    def make():
        return STMPCPlanner(waypoints=_mpc_course(ref.circle()), config=mpc_config(**cfg))

    def to_states(p):
        z = np.zeros(E2E)
        return np.column_stack([p["x"], p["y"], z, p["v"], p["psi"] - 0.01, z, z + 0.01])      # (heading = yaw + beta)
    c = mpc_config(**cfg)
    H = max(float(c.T) * float(c.DT), float(c.TK) * float(c.DTK))
    _end_to_end(ctx, make, to_states, ref.ST7, (H, 0.0), lambda p, st: p.plan_batch(st))


def test_lattice_planner_end_to_end(ctx):
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    la = np.linspace(0.6, 3.0, 8)

    def make():
        p = LatticePlanner(waypoints=ref.circle(), device=0)
        p.configure(lookahead_distances=la, widths=np.linspace(-1.0, 1.0, 5), num_stations=20)
        return p
    to_states = lambda p: np.column_stack([p["x"], p["y"], p["psi"], p["v"]])  # noqa: E731
    horizon = (0.0, float(max(list(la))))
    outs, A, B = _end_to_end(ctx, make, to_states, ref.POSE, horizon, lambda p, st: p.plan_batch(st))
    st, r, a = outs[1]
    assert r["pace"].tobytes() == (1.0 / np.maximum(np.abs(st[:, 3]), B.obstacle_min_speed)).tobytes()      # the lattice's pace likewise
    keys = ("steer", "speed", "status")
    for st, r, a in outs:                                            # step_batch: the same feed
        got = {k: np.array(v) for k, v in A.step_batch(st).items()}
        B.obstacles = r["obs"]
        _same(got, {k: np.array(v) for k, v in B.step_batch(st).items()}, "step_batch")
        _same({k: got[k] for k in keys}, {k: a[k] for k in keys}, "step_batch against plan_batch")
    tracks = circles()
    _end_to_end(ctx, make, to_states, ref.POSE, horizon, lambda p, st: p.plan_batch(st, tracks=tracks, track_ids=pack()["tid"]), tracks=True)
