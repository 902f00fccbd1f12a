"""STMPCPlanner on track sets (f1p_stmpc_ref_tracks_*, f1p_stmpc_qp_plan_tracks_batch, k_stmpc_ref_tracks): every ego follows its own
course.

Bar: each ego's outputs are BIT-identical (tobytes) to the raceline entry point on a second context whose raceline is that ego's track,
fed the same states and holding the same warm start; against the oracle's reference extraction bit-exact, and against the host QP
yardstick (tests/stmpc_qp_ref.py) at the bars of tests/test_gpu_stmpc_qp.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi, synth
from f1tenth_planning_amd.runtime import Context, _ptr

pytestmark = pytest.mark.gpu
T, DT, DL = 40, 0.025, 0.03
TK, DTK, DLK = 8, 0.1, 0.03
PLAN_KEYS = ("steer", "speed", "status", "branch", "u", "obj")


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def ref_ctx():
    """the raceline side of the comparisons"""
    with Context(0) as c:
        yield c


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), what


def _same_warm(a, b, what):
    """two stmpc_qp_warm_get results: the same lengths and the same (oa, odelta_v) over each ego's length (the steps past it are not part
    of the warm start: a kinematic plan writes TK of the W steps)"""
    (wa, na), (wb, nb) = a, b
    _same(na, nb, (what, "len"))
    for e in range(len(na)):
        _same(wa[e, :na[e]], wb[e, :nb[e]], (what, e))


def _turn(rl, ang, dx, dy):
    """a moved and turned copy of a raceline [x, y, v, psi, kappa]; the heading column is NOT wrapped back into [-pi, pi]"""
    c, s = np.cos(ang), np.sin(ang)
    out = rl.copy()
    out[:, 0] = c * rl[:, 0] - s * rl[:, 1] + dx
    out[:, 1] = s * rl[:, 0] + c * rl[:, 1] + dy
    out[:, 3] = rl[:, 3] + ang
    return out


def _lane(rl, off):
    out = rl.copy()
    out[:, 0] -= off * np.sin(rl[:, 3]); out[:, 1] += off * np.cos(rl[:, 3])
    out[:, 2] = rl[:, 2] * (1.0 + 0.1 * off)
    return out


@pytest.fixture(scope="module")
def ref_tracks():
    """K = 3 courses [x, y, v, psi, kappa] from the synthetic raceline: the raceline itself, a moved and turned copy whose headings run
    past +pi (the ego yaw is wrapped, so the +-5 fold fires), and a short open piece of 300 rows (the index walk wraps)"""
    rl = synth.make_raceline(seed=0)
    return [np.ascontiguousarray(t) for t in (rl, _turn(rl, 0.9, 7.0, -4.0), rl[200:500].copy())]


def _ref_egos(tracks, E, seed):
    """states [E, 4] = (x, y, v, yaw) near a row of the ego's own track, yaw wrapped into [-pi, pi]; on the short track a third of the egos
    sit near its end at 8 m/s (T 40 at 6.67 rows a step walks 267 rows: one wrap)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(tracks), E).astype(np.int32)
    st = np.empty((E, 4))
    for k, t in enumerate(tracks):
        m = ids == k
        n = int(m.sum())
        j = rng.integers(0, t.shape[0] - 1, n)
        if k == 2:
            end = rng.random(n) < 0.35
            j[end] = rng.integers(t.shape[0] - 40, t.shape[0] - 1, int(end.sum()))
        st[m, 0] = t[j, 0] + rng.normal(0, 0.15, n)
        st[m, 1] = t[j, 1] + rng.normal(0, 0.15, n)
        st[m, 2] = rng.uniform(0.5, 8.0, n)
        if k == 2:
            st[m, 2] = np.where(end, 8.0, st[m, 2])
        yaw = t[j, 3] + rng.normal(0, 0.05, n)
        st[m, 3] = np.arctan2(np.sin(yaw), np.cos(yaw))
    return ids, st


def _set_raceline(c, t):
    c.set_waypoints(np.ascontiguousarray(t[:, :4]), cols=(0, 1, 2, 3))


def _per_track_ref(ref_ctx, tracks, ids, st, horizon, dt, dl):
    out = np.empty((len(ids), 7, horizon + 1))
    for k, t in enumerate(tracks):
        m = ids == k
        if m.any():
            _set_raceline(ref_ctx, t)
            out[m] = ref_ctx.stmpc_ref(st[m], horizon, dt, dl)
    return out


# ---- 1. the reference per track -----------------------------------------------------------------------------------------------------
def test_ref_equals_per_track_raceline(ctx, ref_ctx, ref_tracks, orc):
    ctx.set_tracks([t[:, :4] for t in ref_tracks], cols=(0, 1, 2, 3))
    ids, st = _ref_egos(ref_tracks, 4096, seed=1)
    for horizon, dt, dl in ((T, DT, DL), (TK, DTK, DLK)):
        got = ctx.stmpc_ref_tracks(st, ids, horizon, dt, dl)
        _same(got, _per_track_ref(ref_ctx, ref_tracks, ids, st, horizon, dt, dl), (horizon, dt, dl))
        assert (got[:, [2, 5, 6]] == 0.0).all()
    got = ctx.stmpc_ref_tracks(st, ids, T, DT, DL)
    # the fold fired on the turned track (a gathered heading no longer in its column), the walk wrapped on the short one
    m1 = ids == 1
    assert (~np.isin(got[m1, 4], ref_tracks[1][:, 3])).any(axis=1).sum() > 10
    short = ref_tracks[2]
    m2 = (ids == 2) & (st[:, 2] == 8.0)
    assert m2.sum() > 50
    first = np.array([np.argmin(np.hypot(short[:, 0] - r[0, 0], short[:, 1] - r[1, 0])) for r in got[m2]])
    last = np.array([np.argmin(np.hypot(short[:, 0] - r[0, -1], short[:, 1] - r[1, -1])) for r in got[m2]])
    assert (last < first).sum() > 20
    # the oracle on each ego's own track: 64 egos, bit-exact
    rng = np.random.default_rng(2)
    pick = np.concatenate([np.nonzero(m1)[0][:16], np.nonzero(m2)[0][:16], rng.choice(len(ids), 32, replace=False)])
    for e in pick:
        t = ref_tracks[ids[e]]
        r0 = orc.calc_ref_trajectory_dynamic(st[e], t[:, 0], t[:, 1], t[:, 3], t[:, 2], T)
        np.testing.assert_array_equal(got[e], r0)


# ---- 2. the _dev twin, bad ids, 65 536 egos on 256 tracks ----------------------------------------------------------------------------
def test_ref_dev_bad_ids_and_scale(ctx, ref_ctx, ref_tracks):
    ctx.set_tracks([t[:, :4] for t in ref_tracks], cols=(0, 1, 2, 3))
    ids, st = _ref_egos(ref_tracks, 1000, seed=3)
    want = ctx.stmpc_ref_tracks(st, ids, T, DT, DL)
    d_st, d_id, d_ref = ctx.to_device(st), ctx.to_device(ids), ctx.alloc(8 * 1000 * 7 * (T + 1))
    try:
        ctx.stmpc_ref_tracks_dev(d_st, d_id, 1000, T, d_ref, DT, DL)
        ctx.sync()
        _same(d_ref.download(np.float64, (1000, 7, T + 1)), want, "_dev")
    finally:
        for b in (d_st, d_id, d_ref):
            b.free()
    bad = ids.copy()
    bad[[0, 500, 999]] = [-1, len(ref_tracks), np.iinfo(np.int32).min]
    got = ctx.stmpc_ref_tracks(st, bad, T, DT, DL)
    assert np.isnan(got[[0, 500, 999]]).all()
    keep = np.ones(1000, bool); keep[[0, 500, 999]] = False
    _same(got[keep], want[keep], "neighbours of bad ids")
    # 65 536 egos on 256 tracks: lanes and turned copies of the raceline, spot-checked against per-track contexts
    rl = ref_tracks[0]
    big = [_turn(_lane(rl, 0.02 * (k % 16) - 0.15), 0.05 * (k // 16), 0.3 * k, -0.2 * k)[:, :4] for k in range(256)]
    ctx.set_tracks(big, cols=(0, 1, 2, 3))
    rng = np.random.default_rng(4)
    E = 65536
    ids = rng.integers(0, 256, E).astype(np.int32)
    j = rng.integers(0, rl.shape[0] - 1, E)
    bigarr = np.stack(big)
    pts = bigarr[ids, j]
    st = np.column_stack([pts[:, 0] + rng.normal(0, 0.1, E), pts[:, 1] + rng.normal(0, 0.1, E), rng.uniform(0.5, 7.0, E),
                          np.arctan2(np.sin(pts[:, 3]), np.cos(pts[:, 3]))])
    got = ctx.stmpc_ref_tracks(st, ids, T, DT, DL)
    for k in (0, 1, 77, 128, 255):
        m = ids == k
        _set_raceline(ref_ctx, big[k])
        _same(got[m], ref_ctx.stmpc_ref(st[m], T, DT, DL), ("65536 egos", k))


# ---- 3. the QP plan chain against per-track contexts --------------------------------------------------------------------------------
def _chain_tracks():
    """courses whose speed profile is 4 m/s on the first half and 1 m/s on the second: egos accelerate and brake through V_KS"""
    cl = synth.make_centerline(seed=4)
    rl = np.ascontiguousarray(cl[:, [1, 2, 5, 3, 4]])
    rl[:, 2] = np.where(np.arange(len(rl)) < len(rl) // 2, 4.0, 1.0)
    return [np.ascontiguousarray(t) for t in (rl, _lane(rl, 0.3), _turn(rl, 1.1, 3.0, 2.0), _turn(_lane(rl, -0.25), -0.6, -2.0, 1.0))]


def _chain_egos(tracks, per, seed):
    rng = np.random.default_rng(seed)
    K = len(tracks)
    ids = np.repeat(np.arange(K, dtype=np.int32), per)
    rng.shuffle(ids)
    E = len(ids)
    st = np.zeros((E, 7))
    for e in range(E):
        t = tracks[ids[e]]
        n = len(t)
        k0 = rng.integers(10, n // 2 - 200) if rng.random() < 0.5 else rng.integers(n // 2 + 10, n - 200)
        st[e] = [t[k0, 0] + rng.normal(0, 0.05), t[k0, 1] + rng.normal(0, 0.05), rng.normal(0, 0.02), rng.uniform(1.5, 3.2),
                 t[k0, 3] + rng.normal(0, 0.03), 0.0, 0.0]
    return ids, st


def test_qp_plan_chain_equals_per_track_contexts(ctx):
    tracks = _chain_tracks()
    ids, states = _chain_egos(tracks, 12, seed=5)
    E, K = len(ids), len(tracks)
    Tq, W = 10, 10
    dcfg, kcfg = _abi.stmpc_cfg(horizon=Tq), _abi.kmpc_cfg(horizon=TK)
    p = SQ.default_params(Tq)
    ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
    ctx.stmpc_qp_warm_reset()
    per = [Context(0) for _ in range(K)]
    try:
        for k in range(K):
            _set_raceline(per[k], tracks[k])
        branches = []
        for step in range(30):
            got = ctx.stmpc_qp_plan_tracks(states, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
            for k in range(K):
                m = ids == k
                want = per[k].stmpc_qp_plan(states[m], dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
                for key in PLAN_KEYS:
                    _same(got[key][m], want[key], (step, k, key))
            assert (got["status"] != _abi.ST_BAD_TRACK).all()
            branches.append(got["branch"].copy())
            states = np.array([SQ.plant(states[e], got["steer"][e], got["speed"][e], p) if got["status"][e] in (0, 2) else states[e]
                               for e in range(E)])
        b = np.array(branches)
        assert ((b[:-1] == 0) & (b[1:] == 1)).any() and ((b[:-1] == 1) & (b[1:] == 0)).any()        # crossings in both directions
        w, n = ctx.stmpc_qp_warm_get(E, W)
        for k in range(K):
            m = ids == k
            _same_warm((w[m], n[m]), per[k].stmpc_qp_warm_get(int(m.sum()), W), ("warm", k))
    finally:
        for c in per:
            c.close()


# ---- 4. against the host yardstick --------------------------------------------------------------------------------------------------
def test_qp_plan_against_the_host_yardstick(ctx):
    tracks = _chain_tracks()
    ids, states = _chain_egos(tracks, 2, seed=6)
    E = len(ids)
    Tq = 10
    dcfg, kcfg = _abi.stmpc_cfg(horizon=Tq), _abi.kmpc_cfg(horizon=TK)
    p, pk = SQ.default_params(Tq), SQ.kin_params(TK)
    ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
    ctx.stmpc_qp_warm_reset()
    warms = [None] * E
    for step in range(6):
        got = ctx.stmpc_qp_plan_tracks(states, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
        assert (got["status"] == 0).all(), (step, got["status"])
        rd = ctx.stmpc_ref_tracks(states[:, [0, 1, 3, 4]], ids, Tq, p["DT"], DL)
        rk = ctx.stmpc_ref_tracks(states[:, [0, 1, 3, 4]], ids, TK, pk["DTK"], DLK)[:, [0, 1, 3, 4]]
        for e in range(E):
            steer, speed, warms[e], br, deg = SQ.plan_step(states[e], warms[e], rd[e], rk[e], p, pk)
            bar = 1e-5 if deg else 1e-7
            assert got["branch"][e] == br, (step, e)
            assert abs(got["steer"][e] - steer) <= bar and abs(got["speed"][e] - speed) <= bar, (step, e, got["steer"][e] - steer)
        states = np.array([SQ.plant(states[e], got["steer"][e], got["speed"][e], p) for e in range(E)])


# ---- 5. bad ids in the plan ---------------------------------------------------------------------------------------------------------
def test_qp_plan_bad_ids_keep_their_warm_start(ctx, ref_ctx):
    tracks = _chain_tracks()
    ids, states = _chain_egos(tracks, 3, seed=7)
    E, K, Tq = len(ids), len(tracks), 10
    dcfg, kcfg = _abi.stmpc_cfg(horizon=Tq), _abi.kmpc_cfg(horizon=TK)
    rng = np.random.default_rng(8)
    warm = rng.normal(0, 0.3, (E, Tq, 2))
    lens = rng.choice([0, TK, Tq], E).astype(np.int32)
    badpos = np.array([2, 7, 11])
    bad = ids.copy()
    bad[badpos] = [-1, K, np.iinfo(np.int32).min]
    ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
    ctx.stmpc_qp_warm_set(warm, lens)
    got = ctx.stmpc_qp_plan_tracks(states, bad, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
    assert (got["status"][badpos] == _abi.ST_BAD_TRACK).all() and (got["branch"][badpos] == -1).all()
    for key in ("steer", "speed", "obj", "u"):
        assert np.isnan(got[key][badpos]).all(), key
    w, n = ctx.stmpc_qp_warm_get(E, Tq)
    _same(w[badpos], warm[badpos], "bad egos' warm start")
    _same(n[badpos], lens[badpos], "bad egos' lengths")
    keep = np.setdiff1d(np.arange(E), badpos)
    ref_ctx.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
    ref_ctx.stmpc_qp_warm_set(warm[keep], lens[keep])
    want = ref_ctx.stmpc_qp_plan_tracks(states[keep], ids[keep], dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
    for key in PLAN_KEYS:
        _same(got[key][keep], want[key], key)
    _same_warm((w[keep], n[keep]), ref_ctx.stmpc_qp_warm_get(len(keep), Tq), "warm")


# ---- 6. one warm start for raceline and track plans ---------------------------------------------------------------------------------
def test_raceline_and_track_plans_share_the_warm_start(ctx, ref_ctx):
    rl = _chain_tracks()[0]
    _, states = _chain_egos([rl], 10, seed=9)
    ids = np.zeros(len(states), np.int32)
    Tq = 10
    dcfg, kcfg = _abi.stmpc_cfg(horizon=Tq), _abi.kmpc_cfg(horizon=TK)
    p = SQ.default_params(Tq)
    _set_raceline(ctx, rl)
    ctx.set_tracks([rl[:, :4]], cols=(0, 1, 2, 3))
    _set_raceline(ref_ctx, rl)
    ctx.stmpc_qp_warm_reset(); ref_ctx.stmpc_qp_warm_reset()
    for step in range(8):
        if step % 2:
            got = ctx.stmpc_qp_plan_tracks(states, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
        else:
            got = ctx.stmpc_qp_plan(states, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
        want = ref_ctx.stmpc_qp_plan(states, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
        for key in PLAN_KEYS:
            _same(got[key], want[key], (step, key))
        states = np.array([SQ.plant(s, got["steer"][e], got["speed"][e], p) for e, s in enumerate(states)])
    _same_warm(ctx.stmpc_qp_warm_get(len(states), Tq), ref_ctx.stmpc_qp_warm_get(len(states), Tq), "warm")


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def _plan_rc(c, x0, ids, dcfg, kcfg, steer=True):
    E = len(ids)
    out = [np.empty(E), np.empty(E), np.empty(E, np.int32), np.empty(E, np.int32)]
    return c.lib.f1p_stmpc_qp_plan_tracks_batch(c.h, _ptr(x0), _ptr(ids), E, C.byref(dcfg), C.byref(kcfg), 2.0, DL, DLK, None,
                                                _ptr(out[0]) if steer else None, _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), None, None)


def _ref_rc(c, st, ids):
    ref = np.empty((len(ids), 7, T + 1))
    return c.lib.f1p_stmpc_ref_tracks_batch(c.h, _ptr(st), _ptr(ids), len(ids), T, DT, DL, _ptr(ref))


def test_errors():
    tracks = _chain_tracks()
    ids, x0 = _chain_egos(tracks, 2, seed=10)
    st4 = np.ascontiguousarray(x0[:, [0, 1, 3, 4]])
    dcfg, kcfg = _abi.stmpc_cfg(horizon=10), _abi.kmpc_cfg(horizon=TK)
    with Context(0) as c:                                     # no raceline at any point
        assert _plan_rc(c, x0, ids, dcfg, kcfg) == _abi.F1P_ESTATE                       # no track set
        assert _ref_rc(c, st4, ids) == _abi.F1P_ESTATE
        c.set_tracks([t[:, :3] for t in tracks])                                         # no heading column
        assert _plan_rc(c, x0, ids, dcfg, kcfg) == _abi.F1P_ESTATE
        assert _ref_rc(c, st4, ids) == _abi.F1P_ESTATE
        c.set_tracks([t[:, :4] for t in tracks], cols=(0, 1, 2, 3))
        assert _plan_rc(c, x0, ids, _abi.stmpc_cfg(horizon=6), kcfg) == _abi.F1P_EINVAL  # TK > T
        assert _plan_rc(c, x0, ids, dcfg, kcfg, steer=False) == _abi.F1P_EINVAL         # steer NULL
        assert _plan_rc(c, x0[:0], ids[:0], dcfg, kcfg) == _abi.F1P_OK                   # E = 0
        assert _ref_rc(c, st4, ids) == _abi.F1P_OK
        out = c.stmpc_qp_plan_tracks(x0, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)       # a track set and no raceline: plans
        assert (out["status"] != _abi.ST_BAD_TRACK).all() and (out["status"] == 0).sum() >= len(ids) // 2, out["status"]
        assert np.isfinite(out["steer"][out["status"] == 0]).all()


# ---- 8. shooting on track references ------------------------------------------------------------------------------------------------
def test_shooting_on_track_references(ctx, ref_ctx, ref_tracks):
    ctx.set_tracks([t[:, :4] for t in ref_tracks], cols=(0, 1, 2, 3))
    ids, st = _ref_egos(ref_tracks, 96, seed=11)
    rng = np.random.default_rng(12)
    E, R = len(ids), 512
    x0 = np.column_stack([st[:, 0], st[:, 1], rng.normal(0, 0.05, E), np.clip(st[:, 2], 2.2, 6.0), st[:, 3], rng.normal(0, 0.2, E),
                          rng.normal(0, 0.02, E)])
    s4 = x0[:, [0, 1, 3, 4]]
    dcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    ctrl = synth.make_controls(E, T, R, seed=13, sigma_a=2.0, sigma_d=2.5, max_accel=3.2, max_steer=4.0)
    got = ctx.stmpc_shoot(x0, ctx.stmpc_ref_tracks(s4, ids, T, DT, DL), ctrl, dcfg)
    kcfg = _abi.kmpc_cfg(horizon=TK, n_rollouts=R)
    kctrl = synth.make_controls(E, TK, R, seed=14)
    gotk = ctx.kmpc_shoot(s4, np.ascontiguousarray(ctx.stmpc_ref_tracks(s4, ids, TK, DTK, DLK)[:, [0, 1, 3, 4]]), kctrl, kcfg)
    for k, t in enumerate(ref_tracks):
        m = ids == k
        _set_raceline(ref_ctx, t)
        want = ref_ctx.stmpc_shoot(x0[m], ref_ctx.stmpc_ref(s4[m], T, DT, DL), ctrl[m], dcfg)
        for key in want:
            _same(got[key][m], want[key], ("stmpc_shoot", k, key))
        wantk = ref_ctx.kmpc_shoot(s4[m], np.ascontiguousarray(ref_ctx.stmpc_ref(s4[m], TK, DTK, DLK)[:, [0, 1, 3, 4]]), kctrl[m], kcfg)
        for key in wantk:
            _same(gotk[key][m], wantk[key], ("kmpc_shoot", k, key))


# ---- 9. the class ------------------------------------------------------------------------------------------------------------------
def _courses(tracks):
    """[x, y, v, psi, kappa] rows -> the class's waypoints format [x, y, yaw, v]"""
    return [[t[:, 0].copy(), t[:, 1].copy(), t[:, 3].copy(), t[:, 2].copy()] for t in tracks]


def test_class_plan_batch_equals_one_planner_per_ego(tracks):
    from f1tenth_planning.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    lev = tracks["levine"][:, [1, 2, 5, 3, 4]]
    trs = [np.ascontiguousarray(t) for t in (lev, _lane(lev, 0.2), _turn(lev, 0.8, 2.0, -1.0))]
    courses = _courses(trs)
    rng = np.random.default_rng(15)
    E = 6
    ids = np.array([0, 1, 2, 2, 1, 0], np.int32)
    st = np.zeros((E, 7))
    for e in range(E):
        t = trs[ids[e]]
        k0 = rng.integers(0, len(t) - 300)
        st[e] = [t[k0, 0], t[k0, 1], 0.0, [1.2, 1.9, 2.4, 1.5, 3.0, 2.1][e], t[k0, 3] + rng.normal(0, 0.05), 0.0, 0.0]
    p = SQ.default_params(40)
    batch = STMPCPlanner(config=mpc_config(SOLVER="qp"))
    ones = [STMPCPlanner(waypoints=courses[ids[e]], config=mpc_config(SOLVER="qp")) for e in range(E)]
    s = st.copy()
    first = None
    for step in range(20):
        out = batch.plan_batch(s, tracks=courses, track_ids=ids)
        if first is None:
            first = {k: v.copy() for k, v in out.items()}
        for e in range(E):
            try:
                steer, speed = ones[e].plan(s[e])
            except RuntimeError:
                assert out["status"][e] in (1, 3), (step, e)
                continue
            assert steer == out["steer"][e] and speed == out["speed"][e], (step, e)
            L = 40 if out["branch"][e] else 8
            assert np.array_equal(ones[e].oa, out["u"][e, :L, 0]) and np.array_equal(ones[e].odelta_v, out["u"][e, :L, 1]), (step, e)
        s = np.array([SQ.plant(s[e], out["steer"][e], out["speed"][e], p) if out["status"][e] in (0, 2) else s[e] for e in range(E)])
    assert (out["status"] != _abi.ST_BAD_TRACK).all()
    batch.reset()                                           # the chain starts again from zeros
    again = batch.plan_batch(st, tracks=courses, track_ids=ids)
    for key in first:
        _same(again[key], first[key], ("after reset", key))


# ---- 10. MultiContext ---------------------------------------------------------------------------------------------------------------
def test_multicontext_two_ranges(ref_tracks):
    from f1tenth_planning_amd.runtime import MultiContext
    tracks = _chain_tracks()
    ids, x0 = _chain_egos(tracks, 25, seed=16)
    dcfg, kcfg = _abi.stmpc_cfg(horizon=10), _abi.kmpc_cfg(horizon=TK)
    p = SQ.default_params(10)
    mc = MultiContext([0, 0])
    a = Context(0)
    try:
        cols = [t[:, :4] for t in tracks]
        mc.set_tracks(cols, cols=(0, 1, 2, 3)); a.set_tracks(cols, cols=(0, 1, 2, 3))
        s4 = x0[:, [0, 1, 3, 4]]
        _same(mc.stmpc_ref_tracks(s4, ids, T, DT, DL), a.stmpc_ref_tracks(s4, ids, T, DT, DL), "ref")
        for step in range(4):
            got = mc.stmpc_qp_plan_tracks(x0, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
            want = a.stmpc_qp_plan_tracks(x0, ids, dcfg, kcfg, v_ks=2.0, dl=DL, dlk=DLK)
            for key in PLAN_KEYS:
                _same(got[key], want[key], (step, key))
            x0 = np.array([SQ.plant(s, want["steer"][e], want["speed"][e], p) for e, s in enumerate(x0)])
    finally:
        mc.close(); a.close()


# ---- 11. the example ----------------------------------------------------------------------------------------------------------------
def test_example_tracks_flag():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "control", "dynamic_mpc.py"), "--solver", "qp", "--tracks", "4",
                        "--steps", "60"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "4 vehicle(s)" in r.stdout
