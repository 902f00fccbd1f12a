"""f1p_kmpc_set_collision: the shooting MPC's rollouts tested against the occupancy grid -- against the expected results composed from the
oracle (tests/kmpc_collision_ref.py), mixed against plain fp64 (bit for bit, all three regimes of the filter), streamed against
generated controls, over a warm-start chain, independent of the batch, switched off, with an inflated grid, the rejections and the class."""
import warnings

import numpy as np
import pytest

import kmpc_collision_ref as K
from f1tenth_planning_amd import _abi, synth

pytestmark = pytest.mark.gpu

SHAPES = [(48, 8, 128, 1), (48, 8, 128, 4), (16, 30, 512, 2), (1, 8, 64, 1)]          # (E, T, R, n_sub)
SEED, CALL = 11, 3
KEYS = ("steer", "speed", "best_idx", "best_cost", "best_seq")


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c
        c.kmpc_set_collision(False)


_scenes, _expected = {}, {}


def _scene(orc, name, E, T):
    """scene + oracle reference, built once per (name, E, T) and left unchanged"""
    key = (name, E, T)
    if key not in _scenes:
        s = dict(a=K.scene_a, b=K.scene_b, c=K.scene_corridor)[name](E, T)
        s["ref"] = K.oracle_ref(orc, s["x0"], s["wp"], T)
        _scenes[key] = s
    return _scenes[key]


def _want(orc, name, E, T, R, n_sub, grid=None):
    key = (name, E, T, R, n_sub, grid is not None)
    if key not in _expected:
        s = _scene(orc, name, E, T)
        _expected[key] = K.expected(orc, s["x0"], s["ref"], _abi.kmpc_cfg(horizon=T, n_rollouts=R), grid or s["grid"], n_sub, SEED, CALL,
                                    warm=K.warm_start(E, T))
    return _expected[key]


def _install(ctx, s, inflate=0.0):
    img, res, ox, oy, occ = s["grid"]
    ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
    ctx.set_grid(img, res, (ox, oy), occ)
    if inflate:
        ctx.inflate_grid(inflate)


def _plan(ctx, x0, ref, cfg, warm, mixed=True, seed=SEED, call=CALL, want_cost=True, streamed=False, fill=None):
    """f1p_kmpc_plan_dev (or gen_controls + shoot_dev) on device buffers -> outputs, the warm start it left, n_refined"""
    E, T, R = x0.shape[0], cfg.horizon, cfg.n_rollouts
    smp = _abi.kmpc_sampler(seed=seed, call=call, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
    if warm is None:
        ctx.kmpc_warm_reset()
    else:
        ctx.kmpc_warm_set(warm)
    d_x0, d_ref = ctx.to_device(x0), ctx.to_device(ref)
    sizes = dict(steer=8 * E, speed=8 * E, best_idx=4 * E, best_cost=8 * E, best_seq=16 * E * T)
    d = {k: ctx.alloc(v) for k, v in sizes.items()}
    if fill is not None:
        for k in d:
            d[k].upload(np.full(sizes[k], fill, np.uint8))
    d_nref = ctx.alloc(4 * E)
    d_nref.upload(np.full(E, -99, np.int32))
    ctx.kmpc_set_mode(mixed, None, d_nref)
    try:
        if streamed:
            d_ctrl = ctx.alloc(4 * E * T * 2 * R)
            ctx.kmpc_gen_controls_dev(d_ctrl, E, cfg, smp)
            ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
        else:
            ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"] if want_cost else None, d["best_seq"])
        ctx.sync()
    finally:
        ctx.kmpc_set_mode(True)
    out = dict(steer=d["steer"].download(np.float64, (E,)), speed=d["speed"].download(np.float64, (E,)),
               best_idx=d["best_idx"].download(np.int32, (E,)), best_cost=d["best_cost"].download(np.float64, (E,)),
               best_seq=d["best_seq"].download(np.float64, (E, T, 2)), n_refined=d_nref.download(np.int32, (E,)))
    if not streamed:
        out["warm"] = ctx.kmpc_warm_get(E, T)
    for b in list(d.values()) + [d_x0, d_ref, d_nref]:
        b.free()
    return out


def _check_against(got, want, keys=KEYS + ("warm",)):
    ok = ~want["fragile"]
    assert ok.any()
    np.testing.assert_array_equal(got["best_idx"][ok], want["best_idx"][ok])
    for k in keys:
        if k == "best_idx":
            continue
        if k == "warm":
            np.testing.assert_array_equal(got[k][ok], want[k][ok])
        else:
            np.testing.assert_allclose(got[k][ok], want[k][ok], rtol=1e-12, atol=1e-12, err_msg=k)
    ab = want["all_blocked"] & ok                                       # exactly the ALL_BLOCKED outputs
    assert (got["best_idx"][ab] == -1).all() and (got["best_cost"][ab] == np.inf).all() and (got["steer"][ab] == 0).all()
    assert (got["speed"][ab] == 0).all() and (got["best_seq"][ab] == 0).all()
    if "warm" in keys:
        assert (got["warm"][ab] == 0).all()


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", SHAPES)
def test_plan_equals_the_expected_results(ctx, orc, E, T, R, n_sub, mixed):
    s = _scene(orc, "a", E, T)
    want = _want(orc, "a", E, T, R, n_sub)
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    got = _plan(ctx, s["x0"], s["ref"], _abi.kmpc_cfg(horizon=T, n_rollouts=R), K.warm_start(E, T), mixed=mixed)
    _check_against(got, want)
    if E > 1:
        assert want["all_blocked"].any() and (want["best_idx"] != want["free_idx"]).mean() >= 0.25
    if not mixed:
        assert (got["n_refined"] == -1).all()


def test_mixed_is_bit_identical_to_plain_fp64_in_all_three_regimes(ctx, orc):
    """scenes A, B and the corridor; T = 8 and 31 (time-parallel tail, lane groups of 32), 40 (groups of 64), 64 (serial tail); n_sub 1 and
    16.  Across them the filter's three regimes are reached -- several survivors refined, a single survivor, everything in fp64 -- and the
    corridor has egos for which the filter proves nothing."""
    E, R = 48, 128
    seen, corridor_fallback = set(), False
    for T in (8, 31, 40, 64):
        cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
        for name in ("a", "b", "c"):
            s = _scene(orc, name, E, T)
            _install(ctx, s)
            for n_sub in (1, 16):
                ctx.kmpc_set_collision(True, n_sub)
                outs = []
                for mixed in (True, False):
                    outs.append(_plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T), mixed=mixed))
                for k in KEYS + ("warm",):
                    np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=f"{k} T={T} scene={name} n_sub={n_sub}")
                # best_cost == NULL: a single survivor is emitted on the filter's word, unrefined
                bare = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T), want_cost=False)
                for k in KEYS + ("warm",):
                    if k != "best_cost":
                        np.testing.assert_array_equal(bare[k], outs[1][k], err_msg=f"{k} without best_cost T={T} scene={name} n_sub={n_sub}")
                n = outs[0]["n_refined"]
                assert (n != -99).all() and (outs[1]["n_refined"] == -1).all()
                seen |= {"refined" if v > 1 else ("single" if v == 1 else "fallback") for v in n}
                corridor_fallback |= name == "c" and bool((n == -1).any())
    assert seen == {"refined", "single", "fallback"} and corridor_fallback


@pytest.mark.parametrize("T,R,n_sub", [(8, 128, 4), (30, 256, 1), (70, 64, 2)])
def test_streamed_equals_generated(ctx, orc, T, R, n_sub):
    """f1p_kmpc_gen_controls_dev + f1p_kmpc_shoot_dev == f1p_kmpc_plan_dev bit for bit, in both modes of the context (streamed shooting with
    the test on is fp64 whatever the mode)"""
    E = 40
    s = _scene(orc, "a", E, T)
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    gen = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T))
    for mixed in (True, False):
        st = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T), mixed=mixed, streamed=True)
        for k in KEYS:
            np.testing.assert_array_equal(gen[k], st[k], err_msg=k)
    assert (gen["best_idx"] == -1).any() and (gen["best_idx"] > 0).any()


def test_warm_start_chain_equals_the_expected_chain(ctx, orc):
    """four plan_batch calls (reference extraction on the device, warm start carried on the context) against the helper's chain, ego by ego;
    an ego is compared until its first fragile call.  The chain holds an ego that is all-blocked in one call and free in the next: it was
    stopped (speed 0) and its warm start zeroed."""
    E, T, R, n_sub = 24, 8, 128, 2
    s = _scene(orc, "a", E, T)
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    x, warm = s["x0"].copy(), K.warm_start(E, T)
    ctx.kmpc_warm_set(warm)
    alive, prev_blocked, freed = np.ones(E, bool), None, 0
    for call in range(4):
        smp = _abi.kmpc_sampler(seed=1234, call=call, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
        got = ctx.kmpc_plan(x, cfg, smp)
        got["warm"] = ctx.kmpc_warm_get(E, T)
        want = K.expected(orc, x, ctx.kmpc_ref(x, T), cfg, s["grid"], n_sub, 1234, call, warm=warm)
        alive &= ~want["fragile"]
        chk = {k: (v[alive] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
        _check_against({k: v[alive] for k, v in got.items()}, chk)
        if prev_blocked is not None:
            freed += int((prev_blocked & ~want["all_blocked"] & alive).sum())
        prev_blocked = want["all_blocked"] & alive
        spd = np.where(alive, want["speed"], got["speed"])             # (an ego that was fragile follows the device: it is no longer compared)
        warm = np.where(alive[:, None, None], want["warm"], got["warm"])
        x[:, 2] = spd
        x[:, 0] += 0.1 * spd * np.cos(x[:, 3]); x[:, 1] += 0.1 * spd * np.sin(x[:, 3])
    assert freed >= 1 and alive.mean() > 0.5


def test_a_plan_does_not_depend_on_the_batch_around_it(ctx, orc):
    T, R, n_sub = 8, 128, 4
    s = _scene(orc, "a", 300, T)
    want = _want(orc, "a", 48, T, R, n_sub)
    pick = int(np.nonzero((want["best_idx"] != want["free_idx"]) & ~want["all_blocked"])[0][0])     # an ego that takes a detour
    ego = _scene(orc, "a", 48, T)["x0"][pick]
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    ref0 = K.oracle_ref(orc, ego[None], s["wp"], T)
    first = None
    for E in (1, 63, 300):
        x0 = s["x0"][:E].copy(); x0[0] = ego
        got = _plan(ctx, x0, np.concatenate([ref0, s["ref"][1:E]]), cfg, None)
        one = {k: got[k][0] for k in KEYS + ("warm",)}
        if first is None:
            first = one
            assert one["best_idx"] >= 0
        for k in one:
            np.testing.assert_array_equal(one[k], first[k], err_msg=f"{k} E={E}")


def test_collision_off_is_what_it_was(ctx, orc):
    """the switch turned on and off once leaves no trace: the same inputs and call counter give the same bits, and they are the oracle's plan;
    in open space the test changes nothing either"""
    E, T, R = 48, 8, 128
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "a", E, T)
    _install(ctx, s)
    ctx.kmpc_set_collision(False)
    before = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T))
    ctx.kmpc_set_collision(True, 4)
    on = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T))
    ctx.kmpc_set_collision(False)
    after = _plan(ctx, s["x0"], s["ref"], cfg, K.warm_start(E, T))
    for k in KEYS + ("warm", "n_refined"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    assert (on["best_idx"] != before["best_idx"]).mean() >= 0.25
    want = orc.kmpc_plan_batch(s["x0"], s["ref"], cfg, SEED, CALL, 1.5, 0.15, warm=K.warm_start(E, T), nthreads=8)
    np.testing.assert_array_equal(after["best_idx"], want["best_idx"])
    for k in ("steer", "speed", "best_cost", "best_seq"):
        np.testing.assert_allclose(after[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)
    np.testing.assert_array_equal(after["warm"], want["warm"])
    b = _scene(orc, "b", E, T)
    _install(ctx, b)
    off = _plan(ctx, b["x0"], b["ref"], cfg, K.warm_start(E, T))
    ctx.kmpc_set_collision(True, 4)
    on = _plan(ctx, b["x0"], b["ref"], cfg, K.warm_start(E, T))
    for k in KEYS + ("warm",):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)


def test_inflation_is_honoured(ctx, orc):
    """f1p_inflate_grid(r) makes the point test a disc test: the result is the helper's on orc.inflate_image's grid"""
    E, T, R, n_sub, r = 48, 8, 128, 1, 0.15
    s = _scene(orc, "a", E, T)
    img, res, ox, oy, occ = s["grid"]
    fat = orc.inflate_image(img, res, occ, r, nthreads=8)
    want = _want(orc, "a", E, T, R, n_sub, grid=(fat, res, ox, oy, occ))
    thin = _want(orc, "a", E, T, R, n_sub)
    assert (want["best_idx"] != thin["best_idx"]).any()                 # the inflation decides some plans
    _install(ctx, s, inflate=r)
    ctx.kmpc_set_collision(True, n_sub)
    for mixed in (True, False):
        _check_against(_plan(ctx, s["x0"], s["ref"], _abi.kmpc_cfg(horizon=T, n_rollouts=R), K.warm_start(E, T), mixed=mixed), want)
    ctx.inflate_grid(0.0)


def test_the_four_rejections(ctx, orc):
    """each returns its error code and a text, launches nothing and leaves the outputs untouched"""
    E, T, R = 8, 8, 64
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "a", E, T)

    def rejected(code, text, streamed):
        from f1tenth_planning_amd.runtime import F1PError
        E_, smp = E, _abi.kmpc_sampler(seed=1, call=0, use_warm=False)
        d_x0, d_ref = ctx.to_device(s["x0"]), ctx.to_device(s["ref"])
        d = [ctx.alloc(n) for n in (8 * E_, 8 * E_, 4 * E_, 8 * E_, 16 * E_ * T)]
        for b, n in zip(d, (8 * E_, 8 * E_, 4 * E_, 8 * E_, 16 * E_ * T)):
            b.upload(np.full(n, 0x5A, np.uint8))
        d_ctrl = ctx.to_device(synth.make_controls(E_, T, R))
        with pytest.raises(F1PError, match=text) as ei:
            if streamed:
                ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E_, cfg, *d)
            else:
                ctx.kmpc_plan_dev(d_x0, d_ref, E_, cfg, smp, *d)
        assert ei.value.code == code
        ctx.sync()
        for b, n in zip(d, (8 * E_, 8 * E_, 4 * E_, 8 * E_, 16 * E_ * T)):
            assert (b.download(np.uint8, (n,)) == 0x5A).all()
        with pytest.raises(F1PError, match=text):
            ctx.kmpc_plan(s["x0"], cfg, smp)

    ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
    ctx.set_grid(None, 0, (0, 0), 0)                                    # 1. no grid
    ctx.kmpc_set_collision(True, 2)
    for streamed in (False, True):
        rejected(_abi.F1P_ESTATE, "no occupancy grid", streamed)
    _install(ctx, s)
    ctx.set_footprint((-0.1, 0.1), 0.15)                                # 2. an oriented footprint
    for streamed in (False, True):
        rejected(_abi.F1P_ESTATE, "f1p_inflate_grid", streamed)
    ctx.set_footprint((), 0.0)
    ctx.kmpc_set_groups(2)                                              # 3. forced workgroups per ego
    rejected(_abi.F1P_ESTATE, "f1p_kmpc_set_groups", False)
    ctx.kmpc_set_groups(0)
    for bad in (0, 17, -3):                                             # 4. n_sub outside [1, 16]: the switch stays as it was
        assert ctx.lib.f1p_kmpc_set_collision(ctx.h, 1, bad) == _abi.F1P_EINVAL
        assert b"n_sub must be in [1, 16]" in ctx.lib.f1p_last_error(ctx.h)
        with pytest.raises(ValueError, match="n_sub"):
            ctx.kmpc_set_collision(True, bad)
    got = _plan(ctx, s["x0"], s["ref"], cfg, None, fill=0x5A)             # ... and with everything in order the same call plans
    assert np.isfinite(got["steer"]).all() and (got["best_idx"] >= -1).all() and (got["best_idx"] < R).all()
    ctx.kmpc_set_collision(False)


def test_planner_class(orc):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    E, T, R, n_sub = 48, 8, 128, 4
    s = _scene(orc, "a", E, T)
    img, res, ox, oy, occ = s["grid"]
    wp = s["wp"]
    course = [wp[:, 0].copy(), wp[:, 1].copy(), wp[:, 3].copy(), wp[:, 2].copy()]
    thresh = 1.0 - occ / 255.0 + 1e-9                                   # -> occupied_below == occ
    outs = {}
    for col in (False, True):
        pl = KMPCPlanner(waypoints=[c.copy() for c in course], config=mpc_config(TK=T, N_ROLLOUTS=R, SEED=5, COLLISION=col, COLLISION_SUBSTEPS=n_sub))
        pl.set_map(img, res, (ox, oy, 0.0), occupied_thresh=thresh)
        assert pl._map[3] == occ
        outs[col] = pl.plan_batch(s["x0"])
        pl2 = KMPCPlanner(config=mpc_config(TK=T, N_ROLLOUTS=R, SEED=5, COLLISION=col, COLLISION_SUBSTEPS=n_sub))
        pl2.set_map(img, res, (ox, oy, 0.0), occupied_thresh=thresh)
        trk = pl2.plan_batch(s["x0"], tracks=[[c.copy() for c in course]], track_ids=np.zeros(E, np.int32))
        for k in KEYS:                                                  # the test does not depend on the course's source
            np.testing.assert_array_equal(trk[k], outs[col][k], err_msg=k)
        if col:
            one = pl2.plan_batch(s["x0"][:1], tracks=[[c.copy() for c in course]], track_ids=[0])
            assert one["best_idx"].shape == (1,)
            pl3 = KMPCPlanner(waypoints=[c.copy() for c in course], config=pl.config)
            pl3.set_map(img, res, (ox, oy, 0.0), occupied_thresh=thresh)
            e = 3                                                       # placed in front of an obstacle: blocked whatever the controls
            assert outs[True]["best_idx"][e] == -1
            x = s["x0"][e]
            with pytest.warns(RuntimeWarning, match="blocked"):
                assert pl3.plan(np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0])) == (0.0, 0.0)
            e = int(np.nonzero((outs[True]["best_idx"] == outs[False]["best_idx"]))[0][0])   # an ego with open road ahead
            x = s["x0"][e]
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                st, sp = pl3.plan(np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0]))
            assert not [w for w in rec if "blocked" in str(w.message)]
            assert abs(st) <= 0.4189 + 1e-12 and sp > 0.0
    blocked = outs[True]["best_idx"] == -1
    assert blocked.any() and (outs[False]["best_idx"] >= 0).all()
    assert (outs[True]["steer"][blocked] == 0).all() and (outs[True]["speed"][blocked] == 0).all() and np.isinf(outs[True]["best_cost"][blocked]).all()
    assert (outs[True]["best_idx"] != outs[False]["best_idx"]).mean() >= 0.25
