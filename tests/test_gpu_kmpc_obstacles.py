"""f1p_kmpc_set_obstacles: the shooting MPC's rollouts tested against moving discs -- against the expected results composed from the oracle
and the numpy disc rule (tests/kmpc_obstacle_ref.py), mixed against plain fp64 (bit for bit, all three regimes of the filter, with and
without the grid), streamed against generated controls, nothing live against nothing set, the hand cases on the rule, a warm-start chain with
moving obstacles, independence of the batch, the borrowed device array, track sets, the rejections and the class."""
import warnings

import numpy as np
import pytest

import kmpc_obstacle_ref as O
from f1tenth_planning_amd import _abi, synth
from f1tenth_planning_amd.runtime import kmpc_set_obstacles, kmpc_set_obstacles_dev

pytestmark = pytest.mark.gpu

SHAPES = [(48, 8, 128, 1), (48, 8, 128, 4), (16, 30, 512, 2), (1, 8, 64, 1)]          # (E, T, R, n_sub)
SEED, CALL = 11, 3
KEYS = ("steer", "speed", "best_idx", "best_cost", "best_seq")


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c
        kmpc_set_obstacles(c, None)
        c.kmpc_set_collision(False)


@pytest.fixture(autouse=True)
def _clean(request):
    """every test starts and ends with no obstacles, the occupancy test off and one substep"""
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.kmpc_set_groups(0)
        kmpc_set_obstacles(c, None)
        c.kmpc_set_collision(False, 1)
        c.kmpc_set_mode(True)


_scenes, _expected = {}, {}


def _scene(orc, name, E, T, M=4):
    """scene + oracle reference, built once per key and left unchanged.  "t": traffic in open space; "a": traffic's obstacles around scene
    A's egos, on scene A's grid"""
    key = (name, E, T, M)
    if key not in _scenes:
        if name == "t":
            s = O.scene_traffic(E, T, M=M)
        else:
            s = O.scene_a(E, T)
            s["obs"] = O.traffic(s["x0"], T, M=M)
        if M == 16:                                                     # sixteen LIVE discs per ego
            s["obs"] = O.crowd16(s["x0"], T)
        s["ref"] = O.oracle_ref(orc, s["x0"], s["wp"], T)
        _scenes[key] = s
    return _scenes[key]


def _want(orc, name, E, T, R, n_sub, grid=False):
    key = (name, E, T, R, n_sub, grid)
    if key not in _expected:
        s = _scene(orc, name, E, T)
        _expected[key] = O.expected(orc, s["x0"], s["ref"], _abi.kmpc_cfg(horizon=T, n_rollouts=R), s["obs"], n_sub, SEED, CALL,
                                    warm=O.warm_start(E, T), grid=s["grid"] if grid else None)
    return _expected[key]


def _install(ctx, s, grid=True):
    img, res, ox, oy, occ = s["grid"]
    ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
    if grid:
        ctx.set_grid(img, res, (ox, oy), occ)
    else:
        ctx.set_grid(None, 0, (0, 0), 0)


def _plan(ctx, x0, ref, cfg, warm, mixed=True, seed=SEED, call=CALL, want_cost=True, streamed=False, fill=None, sigma=(1.5, 0.15)):
    """f1p_kmpc_plan_dev (or gen_controls + shoot_dev) on device buffers -> outputs, the warm start it left, n_refined"""
    E, T, R = x0.shape[0], cfg.horizon, cfg.n_rollouts
    smp = _abi.kmpc_sampler(seed=seed, call=call, use_warm=True, sigma_accel=sigma[0], sigma_steer=sigma[1])
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
    if streamed:
        d_ctrl.free()
    return out


def _check_against(got, want, keys=KEYS + ("warm",)):
    """tests/test_gpu_kmpc_collision.py's bars: the index equal, the fp64 outputs to 1e-12, the warm start equal, exact ALL_BLOCKED outputs"""
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
    ab = want["all_blocked"] & ok
    assert (got["best_idx"][ab] == -1).all() and (got["best_cost"][ab] == np.inf).all() and (got["steer"][ab] == 0).all()
    assert (got["speed"][ab] == 0).all() and (got["best_seq"][ab] == 0).all()
    if "warm" in keys:
        assert (got["warm"][ab] == 0).all()


def _same(a, b, keys=KEYS + ("warm",), msg=""):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k} {msg}")


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", SHAPES)
def test_plan_equals_the_expected_results(ctx, orc, E, T, R, n_sub, mixed):
    s = _scene(orc, "t", E, T)
    want = _want(orc, "t", E, T, R, n_sub)
    _install(ctx, s, grid=False)                                        # obstacles need no grid
    ctx.kmpc_set_collision(False, n_sub)
    kmpc_set_obstacles(ctx, s["obs"])
    got = _plan(ctx, s["x0"], s["ref"], _abi.kmpc_cfg(horizon=T, n_rollouts=R), O.warm_start(E, T), mixed=mixed)
    _check_against(got, want)
    if E > 1:
        assert want["all_blocked"].any() and (want["best_idx"] != want["free_idx"]).mean() >= 0.25
    if not mixed:
        assert (got["n_refined"] == -1).all()


def test_mixed_is_bit_identical_to_plain_fp64_in_all_three_regimes(ctx, orc):
    """traffic without a grid, traffic on an open-space grid with the occupancy test on, and traffic's obstacles on scene A's grid with the
    occupancy test on; T = 8 and 31 (time-parallel tail, lane groups of 32), 40 (groups of 64), 64 (serial tail); n_sub 1 and 16; M 1, 4
    and 16.  Across them the filter's three regimes are reached: several survivors refined, a single survivor, everything in fp64."""
    E, R = 48, 128
    seen = set()
    for T in (8, 31, 40, 64):
        cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
        for name, grid, collide in (("t", False, False), ("t", True, True), ("a", True, True)):
            for M in (1, 4, 16):
                s = _scene(orc, name, E, T, M=4 if M == 1 else M)
                obs = s["obs"][:, :1] if M == 1 else s["obs"]
                _install(ctx, s, grid=grid)
                for n_sub in (1, 16):
                    ctx.kmpc_set_collision(collide, n_sub)
                    kmpc_set_obstacles(ctx, np.ascontiguousarray(obs))
                    outs = [_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed) for mixed in (True, False)]
                    _same(outs[0], outs[1], msg=f"T={T} scene={name} grid={grid} M={M} n_sub={n_sub}")
                    # best_cost == NULL: a single survivor is emitted on the filter's word, unrefined
                    bare = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), want_cost=False)
                    _same(bare, outs[1], keys=tuple(k for k in KEYS + ("warm",) if k != "best_cost"),
                          msg=f"without best_cost T={T} scene={name} grid={grid} M={M} n_sub={n_sub}")
                    n = outs[0]["n_refined"]
                    assert (n != -99).all() and (outs[1]["n_refined"] == -1).all()
                    seen |= {"refined" if v > 1 else ("single" if v == 1 else "fallback") for v in n}
                    if name == "t":
                        assert (outs[0]["best_idx"] == -1).any() or M == 1
    assert seen == {"refined", "single", "fallback"}


@pytest.mark.parametrize("T,R,n_sub,collide", [(8, 128, 4, False), (30, 256, 1, True), (70, 64, 2, False)])
def test_streamed_equals_generated(ctx, orc, T, R, n_sub, collide):
    """f1p_kmpc_gen_controls_dev + f1p_kmpc_shoot_dev == f1p_kmpc_plan_dev bit for bit with obstacles set, in both modes of the context
    (streamed shooting with obstacles is fp64 whatever the mode), without the grid and with it"""
    E = 40
    s = _scene(orc, "a" if collide else "t", E, T)
    _install(ctx, s, grid=collide)
    ctx.kmpc_set_collision(collide, n_sub)
    kmpc_set_obstacles(ctx, s["obs"])
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    gen = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    for mixed in (True, False):
        st = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed, streamed=True)
        _same(gen, st, keys=KEYS)
    assert (gen["best_idx"] == -1).any() and (gen["best_idx"] > 0).any()


def test_nothing_live_is_nothing_set_is_the_plan_without_obstacles(ctx, orc):
    """every slot empty (negative and NaN radii, NaN rows behind them) == obstacles cleared == the plan of a context that never had any,
    bit for bit in every output and in n_refined's verdict; and that plan is the oracle's"""
    E, T, R = 48, 8, 128
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    before = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    empty = np.empty((E, 5, 5)); empty[:] = O.EMPTY; empty[:, 1, 4] = np.nan; empty[:, 3, :4] = np.nan
    ctx.kmpc_set_collision(False, 4)
    kmpc_set_obstacles(ctx, empty)
    for mixed in (True, False):
        _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed), before, msg=f"empty slots, mixed={mixed}")
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), before, keys=KEYS, msg="empty slots, streamed")
    kmpc_set_obstacles(ctx, s["obs"])
    on = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    assert (on["best_idx"] != before["best_idx"]).mean() >= 0.25
    quiet = np.zeros(E, bool); quiet[4::5] = True                       # the scene's egos without a live slot, among egos with some
    for k in KEYS + ("warm",):
        np.testing.assert_array_equal(on[k][quiet], before[k][quiet], err_msg=k)
    kmpc_set_obstacles(ctx, None)
    after = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    _same(after, before, keys=KEYS + ("warm", "n_refined"), msg="cleared")
    want = orc.kmpc_plan_batch(s["x0"], s["ref"], cfg, SEED, CALL, 1.5, 0.15, warm=O.warm_start(E, T), nthreads=8)
    np.testing.assert_array_equal(after["best_idx"], want["best_idx"])
    for k in ("steer", "speed", "best_cost", "best_seq"):
        np.testing.assert_allclose(after[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)
    np.testing.assert_array_equal(after["warm"], want["warm"])


@pytest.mark.parametrize("n_sub", [1, 4])
def test_grid_on_with_an_empty_list_is_the_occupancy_kernels_result(ctx, orc, n_sub):
    E, T, R = 48, 8, 128
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "a", E, T)
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    col = {m: _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=m) for m in (True, False)}
    col_st = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True)
    assert (col[True]["best_idx"] == -1).any()
    empty = np.empty((E, 2, 5)); empty[:] = O.EMPTY
    kmpc_set_obstacles(ctx, empty)
    for m in (True, False):
        _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=m), col[m], msg=f"mixed={m}")
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), col_st, keys=KEYS)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", [(48, 8, 128, 4), (16, 30, 512, 2)])
def test_grid_and_obstacles_against_the_helper_with_both_rules(ctx, orc, E, T, R, n_sub, mixed):
    s = _scene(orc, "a", E, T)
    want = _want(orc, "a", E, T, R, n_sub, grid=True)
    _install(ctx, s)
    ctx.kmpc_set_collision(True, n_sub)
    kmpc_set_obstacles(ctx, s["obs"])
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    got = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed)
    _check_against(got, want)
    if mixed:                                                           # each rule decides some plans
        kmpc_set_obstacles(ctx, None)
        grid_only = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
        ctx.kmpc_set_collision(False, n_sub)
        kmpc_set_obstacles(ctx, s["obs"])
        obs_only = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
        assert (got["best_idx"] != grid_only["best_idx"]).any() and (got["best_idx"] != obs_only["best_idx"]).any()


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", [(48, 8, 128, 4), (16, 30, 512, 2)])
def test_sixteen_live_discs_against_the_helper(ctx, orc, E, T, R, n_sub, mixed):
    """every slot of every ego live and within reach: the whole LDS table, the ballot's compaction and the filter's slot loop at n_live 16"""
    s = _scene(orc, "t", E, T, M=16)
    assert (s["obs"][:, :, 4] >= 0).all()
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    key = ("crowd", E, T, R, n_sub)
    if key not in _expected:
        _expected[key] = O.expected(orc, s["x0"], s["ref"], cfg, s["obs"], n_sub, SEED, CALL, warm=O.warm_start(E, T))
    _install(ctx, s, grid=False)
    ctx.kmpc_set_collision(False, n_sub)
    kmpc_set_obstacles(ctx, s["obs"])
    _check_against(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed), _expected[key])


@pytest.mark.parametrize("case", O.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_on_the_device(ctx, case):
    """zero controls, so every rollout is the straight line p_t = (0.25 t, 0): blocked means best_idx -1, free means rollout 0 -- through
    the generated plan in both modes (sigma 0, no warm start) and through the streamed entry point"""
    _, x0, T, n_sub, obs, blocked = case
    R = 4
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    x0 = np.array([x0]); ref = np.zeros((1, 4, T + 1))
    ctx.kmpc_set_collision(False, n_sub)
    kmpc_set_obstacles(ctx, np.array([obs], np.float64))
    want = -1 if blocked else 0
    for mixed in (True, False):
        got = _plan(ctx, x0, ref, cfg, None, mixed=mixed, sigma=(0.0, 0.0))
        assert got["best_idx"][0] == want, f"generated, mixed={mixed}"
        assert (got["speed"][0] == 0.0) == blocked and (got["best_cost"][0] == np.inf) == blocked
    got = ctx.kmpc_shoot(x0, ref, np.zeros((1, T, 2, R), np.float32), cfg)
    assert got["best_idx"][0] == want, "streamed"


def test_chain_with_moving_obstacles_equals_the_expected_chain(ctx, orc):
    """four plan_batch calls (reference extraction on the device, warm start carried on the context), the obstacles advanced at their
    velocities between calls, against the helper's chain, ego by ego until an ego's first fragile call.  The parked disc on the first
    station of egos 3::8 is taken away after the first call: those egos are all-blocked, stopped, their warm start zeroed -- and free in
    the next call."""
    E, T, R, n_sub = 24, 8, 128, 2
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    ctx.kmpc_set_collision(False, n_sub)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    x, warm, obs = s["x0"].copy(), O.warm_start(E, T), s["obs"].copy()
    ctx.kmpc_warm_set(warm)
    alive, prev_blocked, freed = np.ones(E, bool), None, 0
    for call in range(4):
        smp = _abi.kmpc_sampler(seed=1234, call=call, use_warm=True, sigma_accel=1.5, sigma_steer=0.15)
        kmpc_set_obstacles(ctx, obs)
        got = ctx.kmpc_plan(x, cfg, smp)
        got["warm"] = ctx.kmpc_warm_get(E, T)
        want = O.expected(orc, x, ctx.kmpc_ref(x, T), cfg, obs, n_sub, 1234, call, warm=warm)
        alive &= ~want["fragile"]
        chk = {k: (v[alive] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
        _check_against({k: v[alive] for k, v in got.items()}, chk)
        if prev_blocked is not None:
            now_free = prev_blocked & ~want["all_blocked"] & alive
            freed += int(now_free.sum())
            assert (warm[now_free] == 0).all() and (x[now_free, 2] == 0).all()   # what the all-blocked call left them with
        prev_blocked = want["all_blocked"] & alive
        spd = np.where(alive, want["speed"], got["speed"])             # (an ego that was fragile follows the device: it is no longer compared)
        warm = np.where(alive[:, None, None], want["warm"], got["warm"])
        x[:, 2] = spd
        x[:, 0] += 0.1 * spd * np.cos(x[:, 3]); x[:, 1] += 0.1 * spd * np.sin(x[:, 3])
        obs[:, :, 0] += 0.1 * obs[:, :, 2]; obs[:, :, 1] += 0.1 * obs[:, :, 3]
        obs[:, 3] = O.EMPTY
    assert freed >= 1 and alive.mean() > 0.5


def test_a_plan_does_not_depend_on_the_batch_around_it(ctx, orc):
    T, R, n_sub = 8, 128, 4
    s = _scene(orc, "t", 300, T)
    want = _want(orc, "t", 48, T, R, n_sub)
    pick = int(np.nonzero((want["best_idx"] != want["free_idx"]) & ~want["all_blocked"])[0][0])     # an ego that takes a detour
    s48 = _scene(orc, "t", 48, T)
    ego, ego_obs = s48["x0"][pick], s48["obs"][pick]
    _install(ctx, s, grid=False)
    ctx.kmpc_set_collision(False, n_sub)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    ref0 = O.oracle_ref(orc, ego[None], s["wp"], T)
    first = None
    for E in (1, 63, 300):
        x0 = s["x0"][:E].copy(); x0[0] = ego
        obs = s["obs"][:E].copy(); obs[0] = ego_obs
        kmpc_set_obstacles(ctx, obs)
        got = _plan(ctx, x0, np.concatenate([ref0, s["ref"][1:E]]), cfg, None)
        one = {k: got[k][0] for k in KEYS + ("warm",)}
        if first is None:
            first = one
            assert one["best_idx"] >= 0
        for k in one:
            np.testing.assert_array_equal(one[k], first[k], err_msg=f"{k} E={E}")


def test_a_borrowed_device_array_equals_the_copied_one(ctx, orc):
    """f1p_kmpc_set_obstacles_dev: the same plan, and the array rewritten in place is the next plan's"""
    E, T, R, n_sub = 48, 8, 128, 2
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    ctx.kmpc_set_collision(False, n_sub)
    moved = s["obs"].copy(); moved[:, :, 0] += 0.3 * moved[:, :, 2]; moved[:, :, 1] += 0.3 * moved[:, :, 3]; moved[:, 3] = O.EMPTY
    want = []
    for obs in (s["obs"], moved):
        kmpc_set_obstacles(ctx, obs)
        want.append(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)))
    assert (want[0]["best_idx"] != want[1]["best_idx"]).any()
    d_obs = ctx.to_device(s["obs"])
    kmpc_set_obstacles_dev(ctx, d_obs, E, s["obs"].shape[1])
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), want[0])
    d_obs.upload(moved)                                                 # in place, no second set
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), want[1])
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), want[1], keys=KEYS)
    with pytest.raises(ValueError, match="E and M"):
        kmpc_set_obstacles_dev(ctx, d_obs)
    kmpc_set_obstacles_dev(ctx, None)
    d_obs.free()
    kmpc_set_obstacles(ctx, None)
    off = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    assert (off["best_idx"] >= 0).all()


def test_the_rejections(ctx, orc):
    """each returns its error code and a text, launches nothing and leaves the outputs untouched"""
    from f1tenth_planning_amd.runtime import F1PError
    E, T, R = 8, 8, 64
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    obs = s["obs"]

    def rejected(code, text, streamed, E_):
        smp = _abi.kmpc_sampler(seed=1, call=0, use_warm=False)
        d_x0, d_ref = ctx.to_device(s["x0"][:E_]), ctx.to_device(s["ref"][:E_])
        sizes = (8 * E_, 8 * E_, 4 * E_, 8 * E_, 16 * E_ * T)
        d = [ctx.alloc(n) for n in sizes]
        for b, n in zip(d, sizes):
            b.upload(np.full(n, 0x5A, np.uint8))
        d_ctrl = ctx.to_device(synth.make_controls(E_, T, R))
        with pytest.raises(F1PError, match=text) as ei:
            if streamed:
                ctx.kmpc_shoot_dev(d_x0, d_ref, d_ctrl, E_, cfg, *d)
            else:
                ctx.kmpc_plan_dev(d_x0, d_ref, E_, cfg, smp, *d)
        assert ei.value.code == code
        ctx.sync()
        for b, n in zip(d, sizes):
            assert (b.download(np.uint8, (n,)) == 0x5A).all()
        with pytest.raises(F1PError, match=text):
            ctx.kmpc_plan(s["x0"][:E_], cfg, smp)
        for b in d + [d_x0, d_ref, d_ctrl]:
            b.free()

    for bad in (17, -1, 100):                                           # 1. M outside [1, 16]: nothing changes
        big = np.zeros((E, max(bad, 1), 5))
        assert ctx.lib.f1p_kmpc_set_obstacles(ctx.h, big.ctypes.data, E, bad) == _abi.F1P_EINVAL
        assert b"M must be in [1, 16]" in ctx.lib.f1p_last_error(ctx.h)
        d_big = ctx.to_device(big)
        assert ctx.lib.f1p_kmpc_set_obstacles_dev(ctx.h, d_big.ptr, E, bad) == _abi.F1P_EINVAL
        d_big.free()
    with pytest.raises(ValueError, match="M must be"):
        kmpc_set_obstacles(ctx, np.zeros((E, 17, 5)))
    with pytest.raises(ValueError, match=r"\[E, M, 5\]"):
        kmpc_set_obstacles(ctx, np.zeros((E, 4)))
    kmpc_set_obstacles(ctx, obs)                                         # 2. a plan of another E
    for streamed in (False, True):
        rejected(_abi.F1P_ESTATE, "obstacles were set for 8 egos", streamed, 5)
    with pytest.raises(F1PError, match="f1p_kmpc_set_obstacles") as ei:  # 3. forced workgroups per ego, either way round
        ctx.kmpc_set_groups(2)
    assert ei.value.code == _abi.F1P_ESTATE
    kmpc_set_obstacles(ctx, None)
    ctx.kmpc_set_groups(2)
    with pytest.raises(F1PError, match="f1p_kmpc_set_groups") as ei:
        kmpc_set_obstacles(ctx, obs)
    assert ei.value.code == _abi.F1P_ESTATE
    ctx.kmpc_set_groups(0)
    kmpc_set_obstacles(ctx, obs)
    kmpc_set_obstacles(ctx, np.zeros((E, 0, 5)))                         # M == 0 clears
    free = _plan(ctx, s["x0"], s["ref"], cfg, None, fill=0x5A)
    assert (free["best_idx"] >= 0).all()
    kmpc_set_obstacles(ctx, obs)                                         # ... and with everything in order the same call plans
    got = _plan(ctx, s["x0"], s["ref"], cfg, None, fill=0x5A)
    assert np.isfinite(got["steer"]).all() and (got["best_idx"] >= -1).all() and (got["best_idx"] < R).all() and (got["best_idx"] == -1).any()


def test_planner_class(orc):
    from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config
    E, T, R, n_sub = 48, 8, 128, 4
    s = _scene(orc, "t", E, T)
    wp, obs = s["wp"], s["obs"]
    course = [wp[:, 0].copy(), wp[:, 1].copy(), wp[:, 3].copy(), wp[:, 2].copy()]
    conf = mpc_config(TK=T, N_ROLLOUTS=R, SEED=5, COLLISION_SUBSTEPS=n_sub)

    def planner(waypoints=True, obstacles=None):
        pl = KMPCPlanner(waypoints=[c.copy() for c in course] if waypoints else None, config=conf)
        assert pl.obstacles is None
        pl.obstacles = obstacles
        return pl

    free = planner().plan_batch(s["x0"])
    with_obs = planner(obstacles=obs).plan_batch(s["x0"])
    blocked = with_obs["best_idx"] == -1
    assert blocked.any() and (free["best_idx"] >= 0).all() and (with_obs["best_idx"] != free["best_idx"]).mean() >= 0.25
    assert (with_obs["steer"][blocked] == 0).all() and (with_obs["speed"][blocked] == 0).all() and np.isinf(with_obs["best_cost"][blocked]).all()
    trk = planner(False, obs).plan_batch(s["x0"], tracks=[[c.copy() for c in course]], track_ids=np.zeros(E, np.int32))
    for k in KEYS:                                                      # tracks= with obstacles: the test does not depend on the course's source
        np.testing.assert_array_equal(trk[k], with_obs[k], err_msg=k)
    pl = planner(obstacles=obs)                                         # the obstacles are one call's: it takes them
    first = pl.plan_batch(s["x0"])
    assert pl.obstacles is None
    for k in KEYS:
        np.testing.assert_array_equal(first[k], with_obs[k], err_msg=k)
    pl.reset()
    again = pl.plan_batch(s["x0"])
    for k in KEYS:
        np.testing.assert_array_equal(again[k], free[k], err_msg=k)
    # controls= with obstacles: the streamed kernel
    ctrl = synth.make_controls(E, T, R)
    st_free = planner().plan_batch(s["x0"], controls=ctrl)
    st_obs = planner(obstacles=obs).plan_batch(s["x0"], controls=ctrl)
    assert (st_obs["best_idx"] == -1).any() and (st_free["best_idx"] >= 0).all()
    quiet = np.zeros(E, bool); quiet[4::5] = True
    np.testing.assert_array_equal(st_obs["best_idx"][quiet], st_free["best_idx"][quiet])
    # plan(): the warning and (0, 0) on all-blocked; an open road otherwise
    e = int(np.nonzero(blocked)[0][0])
    pl3 = planner(obstacles=obs[e])
    x = s["x0"][e]
    with pytest.warns(RuntimeWarning, match="blocked"):
        assert pl3.plan(np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0])) == (0.0, 0.0)
    assert pl3.obstacles is None
    with warnings.catch_warnings(record=True) as rec:                   # the same vehicle without them (a batch plan, then plan(): no leftovers)
        warnings.simplefilter("always")
        st, sp = pl3.plan(np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0]))
    assert not [w for w in rec if "blocked" in str(w.message)]
    assert abs(st) <= 0.4189 + 1e-12 and sp > 0.0
    e = int(np.nonzero(~blocked & (with_obs["best_idx"] != free["best_idx"]))[0][0])      # a detour
    x = s["x0"][e]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        st, sp = planner(obstacles=obs[e]).plan(np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0]))
    assert not [w for w in rec if "blocked" in str(w.message)]
    assert abs(st) <= 0.4189 + 1e-12 and sp > 0.0
