"""f1p_stmpc_set_obstacles: the dynamic MPC's shooting rollouts tested against moving discs -- against the expected results composed from
the oracle and the numpy disc rule (tests/stmpc_obstacle_ref.py), mixed against plain fp64 (bit for bit, all three regimes of the filter,
with and without the grid), streamed against generated controls, nothing live against nothing set, both rules together, plan_batch with
both branches (and permuted), a chain with moving discs, independence of the batch, the borrowed device array, the hand cases on the rule,
the two obstacle states kept apart (also when one of them is cleared), the rejections and the class."""
import warnings

import numpy as np
import pytest

import stmpc_obstacle_ref as O
from f1tenth_planning_amd import _abi, synth
from f1tenth_planning_amd.runtime import kmpc_set_obstacles, stmpc_set_obstacles, stmpc_set_obstacles_dev

pytestmark = pytest.mark.gpu

SHAPES = [(48, 40, 128, 1), (48, 40, 128, 4), (16, 64, 256, 2), (1, 40, 64, 1)]       # (E, T, R, n_sub)
SEED, CALL = 11, 3
KEYS = ("steer", "speed", "best_idx", "best_cost", "best_seq")
TK = 8


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c


@pytest.fixture(autouse=True)
def _clean(request):
    """every test ends with no obstacles in either state, the occupancy tests off and the default substeps"""
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.kmpc_set_groups(0)
        stmpc_set_obstacles(c, None)
        kmpc_set_obstacles(c, None)
        c.stmpc_set_collision(False)
        c.kmpc_set_collision(False, 1)
        c.stmpc_set_mode(True)


_scenes, _expected = {}, {}


def _scene(orc, name, E, T, M=4):
    """scene + oracle reference, built once per key and left unchanged.  "t": traffic around scene B's egos (its image has no occupied cell);
    "d": the same egos and discs on scene D's map.  M 16: crowd16"""
    key = (name, E, T, M)
    if key not in _scenes:
        s = O.scene_traffic(E, T, M=M, grid="b" if name == "t" else "d")
        s["ref"] = O.oracle_ref(orc, s["x0"], s["wp"], T)
        _scenes[key] = s
    return _scenes[key]


def _want(orc, name, E, T, R, n_sub, M=4, grid=False):
    key = (name, E, T, R, n_sub, M, grid)
    if key not in _expected:
        s = _scene(orc, name, E, T, M)
        _expected[key] = O.expected(orc, s["x0"], s["ref"], _abi.stmpc_cfg(horizon=T, n_rollouts=R), s["obs"], n_sub, SEED, CALL,
                                    warm=O.warm_start(E, T), grid=s["grid"] if grid else None)
    return _expected[key]


def _install(ctx, s, grid=True):
    img, res, ox, oy, occ = s["grid"]
    ctx.set_waypoints(s["wp"], cols=(0, 1, 2, 3))
    if grid:
        ctx.set_grid(img, res, (ox, oy), occ)
    else:
        ctx.set_grid(None, 0, (0, 0), 0)


def _sampler(seed=SEED, call=CALL, use_warm=True, sig=None):
    return _abi.stmpc_sampler(seed=seed, call=call, use_warm=use_warm, **(sig or O.SIG))


def _plan(ctx, x0, ref, cfg, warm, mixed=True, seed=SEED, call=CALL, streamed=False, fill=None, sig=None):
    """f1p_stmpc_plan_dev (or gen_controls + shoot_dev) on device buffers -> outputs, the warm start it left, n_refined"""
    E, T, R = x0.shape[0], cfg.horizon, cfg.n_rollouts
    smp = _sampler(seed, call, sig=sig)
    if warm is None:
        ctx.stmpc_warm_reset()
    else:
        ctx.stmpc_warm_set(warm, np.full(E, 2), T)
    d_x0, d_ref = ctx.to_device(x0), ctx.to_device(ref)
    sizes = dict(steer=8 * E, speed=8 * E, best_idx=4 * E, best_cost=8 * E, best_seq=16 * E * T)
    d = {k: ctx.alloc(v) for k, v in sizes.items()}
    if fill is not None:
        for k in d:
            d[k].upload(np.full(sizes[k], fill, np.uint8))
    d_nref = ctx.alloc(4 * E)
    d_nref.upload(np.full(E, -99, np.int32))
    ctx.stmpc_set_mode(mixed, None, d_nref)
    d_ctrl = None
    try:
        if streamed:
            d_ctrl = ctx.alloc(4 * E * T * 2 * R)
            ctx.stmpc_gen_controls_dev(d_ctrl, E, cfg, smp)
            ctx.stmpc_shoot_dev(d_x0, d_ref, d_ctrl, E, cfg, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
        else:
            ctx.stmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"], d["best_seq"])
        ctx.sync()
    finally:
        ctx.stmpc_set_mode(True)
    out = dict(steer=d["steer"].download(np.float64, (E,)), speed=d["speed"].download(np.float64, (E,)),
               best_idx=d["best_idx"].download(np.int32, (E,)), best_cost=d["best_cost"].download(np.float64, (E,)),
               best_seq=d["best_seq"].download(np.float64, (E, T, 2)), n_refined=d_nref.download(np.int32, (E,)))
    if not streamed:
        out["warm"], out["tag"] = ctx.stmpc_warm_get(E, T)
    for b in list(d.values()) + [d_x0, d_ref, d_nref] + ([d_ctrl] if d_ctrl is not None else []):
        b.free()
    return out


def _check_against(got, want, warm=True):
    """tests/test_gpu_stmpc_collision.py's bars: the index, the applied sequence, steer, speed and the next warm start exact, the cost to 1e-10"""
    ok = ~want["fragile"]
    assert ok.any()
    np.testing.assert_array_equal(got["best_idx"][ok], want["best_idx"][ok])
    np.testing.assert_allclose(got["best_cost"][ok], want["best_cost"][ok], rtol=1e-10, atol=1e-9)
    for k in ("best_seq", "steer", "speed") + (("warm",) if warm else ()):
        np.testing.assert_array_equal(got[k][ok], want[k][ok], err_msg=k)
    ab = want["all_blocked"] & ok                                       # exactly the ALL_BLOCKED outputs
    assert (got["best_idx"][ab] == -1).all() and (got["best_cost"][ab] == np.inf).all() and (got["steer"][ab] == 0).all()
    assert (got["speed"][ab] == 0).all() and (got["best_seq"][ab] == 0).all()
    if warm:
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
    ctx.stmpc_set_collision(False, n_sub)
    stmpc_set_obstacles(ctx, s["obs"])
    got = _plan(ctx, s["x0"], s["ref"], _abi.stmpc_cfg(horizon=T, n_rollouts=R), O.warm_start(E, T), mixed=mixed)
    _check_against(got, want)
    assert (got["tag"] == 2).all()                                      # an all-blocked ego's tag stays its branch's
    if E > 1:
        assert want["all_blocked"].any() and ((want["best_idx"] != want["free_idx"]) & ~want["all_blocked"]).any()
    if not mixed:
        assert (got["n_refined"] == -99).all()                          # the plain-fp64 kernel has no filter to report


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", SHAPES[:3])
def test_sixteen_live_discs_against_the_helper(ctx, orc, E, T, R, n_sub, mixed):
    """every slot of every ego live: the whole LDS table, the ballot's compaction, the filter's slot loop and the refinement's table at 16"""
    s = _scene(orc, "t", E, T, M=16)
    assert (s["obs"][:, :, 4] >= 0).all()
    want = _want(orc, "t", E, T, R, n_sub, M=16)
    _install(ctx, s, grid=False)
    ctx.stmpc_set_collision(False, n_sub)
    stmpc_set_obstacles(ctx, s["obs"])
    _check_against(_plan(ctx, s["x0"], s["ref"], _abi.stmpc_cfg(horizon=T, n_rollouts=R), O.warm_start(E, T), mixed=mixed), want)


def test_mixed_is_bit_identical_to_plain_fp64_in_all_three_regimes(ctx, orc):
    """traffic without a grid, traffic on scene B's open grid with the occupancy test on, and traffic's discs on scene D's grid with the
    occupancy test on; T = 8, 40, 63 (time-parallel refinement), 64 (serial refinement); n_sub 1 and 16; M 1, 4 and 16 (crowd16).  Across
    them the filter's three regimes are reached: refined with a small list, no FREE rollout (-1 and all blocked: the parked disc), more than
    64 survivors (-1 for an ego WITHOUT a live slot and without a grid, where the coasting rollout 1 is trusted and FREE, so "no FREE
    rollout" cannot be the reason; reached with a braking warm start: most rollouts fall below the trust speed and are listed)."""
    E, R = 32, 128
    refined = no_free = many = False
    quiet = np.zeros(E, bool); quiet[4::5] = True
    for T in (8, 40, 63, 64):
        cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
        brake = O.warm_start(E, T)
        brake[:, :, 1] -= 2.5
        for name, grid in (("t", False), ("t", True), ("d", True)):
            for M in (1, 4, 16):
                s = _scene(orc, name, E, T, M=4 if M == 1 else M)
                obs = np.ascontiguousarray(s["obs"][:, :1] if M == 1 else s["obs"])
                _install(ctx, s, grid=grid)
                for n_sub, warm in ((1, O.warm_start(E, T)), (16, O.warm_start(E, T)), (1, brake)):
                    ctx.stmpc_set_collision(grid, n_sub)
                    stmpc_set_obstacles(ctx, obs)
                    outs = [_plan(ctx, s["x0"], s["ref"], cfg, warm, mixed=m) for m in (True, False)]
                    _same(outs[0], outs[1], keys=KEYS + ("warm", "tag"), msg=f"T={T} scene={name} grid={grid} M={M} n_sub={n_sub}")
                    n = outs[0]["n_refined"]
                    assert (n != -99).all() and (n >= -1).all() and (n <= 64).all() and (outs[1]["n_refined"] == -99).all()
                    refined |= bool(((n >= 1) & (n <= 8)).any())
                    no_free |= bool(((n == -1) & (outs[0]["best_idx"] == -1)).any())   # all blocked: certainly no FREE rollout
                    if not grid and M == 4:
                        many |= bool((n[quiet] == -1).any())
                    if M > 1:
                        assert (outs[0]["best_idx"] == -1).any()
    assert refined and no_free and many


@pytest.mark.parametrize("T,R,n_sub,collide", [(8, 128, 4, False), (40, 256, 1, True), (70, 64, 2, False)])
def test_streamed_equals_generated(ctx, orc, T, R, n_sub, collide):
    """f1p_stmpc_gen_controls_dev + f1p_stmpc_shoot_dev == f1p_stmpc_plan_dev bit for bit with obstacles set, in both modes of the context
    (streamed shooting with obstacles is fp64 whatever the mode), without the grid and with it"""
    E = 40
    s = _scene(orc, "d" if collide else "t", E, T)
    _install(ctx, s, grid=collide)
    ctx.stmpc_set_collision(collide, n_sub)
    stmpc_set_obstacles(ctx, s["obs"])
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    for mixed in (True, False):
        gen = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed)
        st = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed, streamed=True)
        _same(gen, st, keys=KEYS, msg=f"mixed={mixed}")
    assert (gen["best_idx"] == -1).any() and (gen["best_idx"] > 0).any()


def test_nothing_live_is_nothing_set_is_the_plan_without_obstacles(ctx, orc):
    """every slot empty (negative and NaN radii, NaN rows behind them) == obstacles cleared == the plan of a context that never had any,
    bit for bit; an ego without a live slot among egos with some likewise"""
    from f1tenth_planning_amd.runtime import Context
    E, T, R = 48, 40, 128
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    with Context(0) as fresh:
        _install(fresh, s, grid=False)
        never = _plan(fresh, s["x0"], s["ref"], cfg, O.warm_start(E, T))
        never_st = _plan(fresh, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True)
    _install(ctx, s, grid=False)
    empty = np.empty((E, 5, 5)); empty[:] = O.EMPTY; empty[:, 1, 4] = np.nan; empty[:, 3, :4] = np.nan
    ctx.stmpc_set_collision(False, 4)
    stmpc_set_obstacles(ctx, empty)
    for mixed in (True, False):
        _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed), never, msg=f"empty slots, mixed={mixed}")
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), never_st, keys=KEYS, msg="empty slots, streamed")
    stmpc_set_obstacles(ctx, s["obs"])
    on = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    assert (on["best_idx"] != never["best_idx"]).mean() >= 0.25
    quiet = np.zeros(E, bool); quiet[4::5] = True                       # the scene's egos without a live slot, among egos with some
    for k in KEYS + ("warm",):
        np.testing.assert_array_equal(on[k][quiet], never[k][quiet], err_msg=k)
    stmpc_set_obstacles(ctx, None)
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), never, keys=KEYS + ("warm", "n_refined"), msg="cleared")
    stmpc_set_obstacles(ctx, s["obs"])
    stmpc_set_obstacles(ctx, np.zeros((E, 0, 5)))                        # M == 0 clears
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), never, keys=KEYS + ("warm", "n_refined"), msg="M == 0")


@pytest.mark.parametrize("n_sub", [1, 4])
def test_grid_on_with_an_empty_list_is_the_occupancy_kernels_result(ctx, orc, n_sub):
    E, T, R = 48, 40, 128
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "d", E, T)
    _install(ctx, s)
    ctx.stmpc_set_collision(True, n_sub)
    col = {m: _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=m) for m in (True, False)}
    col_st = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True)
    assert (col[True]["best_idx"] == -1).any()
    empty = np.empty((E, 2, 5)); empty[:] = O.EMPTY
    stmpc_set_obstacles(ctx, empty)
    for m in (True, False):
        _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=m), col[m], msg=f"mixed={m}")
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), col_st, keys=KEYS)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("E,T,R,n_sub", [(48, 40, 128, 4), (16, 64, 256, 2)])
def test_grid_and_obstacles_against_the_helper_with_both_rules(ctx, orc, E, T, R, n_sub, mixed):
    s = _scene(orc, "d", E, T)
    want = _want(orc, "d", E, T, R, n_sub, grid=True)
    _install(ctx, s)
    ctx.stmpc_set_collision(True, n_sub)
    stmpc_set_obstacles(ctx, s["obs"])
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    got = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), mixed=mixed)
    _check_against(got, want)
    if mixed:                                                           # each rule decides some plans
        stmpc_set_obstacles(ctx, None)
        grid_only = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
        ctx.stmpc_set_collision(False, n_sub)
        stmpc_set_obstacles(ctx, s["obs"])
        obs_only = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
        assert (got["best_idx"] != grid_only["best_idx"]).any() and (got["best_idx"] != obs_only["best_idx"]).any()


def _batch(ctx, x0, dcfg, kcfg, seed, call):
    out = ctx.stmpc_plan(x0, dcfg, kcfg, _sampler(seed, call))
    out["warm"], out["tag"] = ctx.stmpc_warm_get(x0.shape[0], dcfg.horizon, kcfg.horizon)
    return out


def _check_half(got, want, Tb, dyn):
    """one branch's egos of a plan_batch against the helper (the kinematic bars are test_gpu_kmpc_collision's)"""
    ids = want["ids"]
    g = dict(steer=got["steer"][ids], speed=got["speed"][ids], best_idx=got["best_idx"][ids], best_cost=got["best_cost"][ids],
             best_seq=got["best_seq"][ids, :Tb], warm=got["warm"][ids, :Tb])
    if dyn:
        _check_against(g, want)
    else:
        ok = ~want["fragile"]
        assert ok.any()
        np.testing.assert_array_equal(g["best_idx"][ok], want["best_idx"][ok])
        for k in ("steer", "speed", "best_cost", "best_seq"):
            np.testing.assert_allclose(g[k][ok], want[k][ok], rtol=1e-12, atol=1e-12, err_msg=k)
        np.testing.assert_array_equal(g["warm"][ok], want["warm"][ok])
        ab = want["all_blocked"] & ok
        assert (g["best_idx"][ab] == -1).all() and (g["best_cost"][ab] == np.inf).all() and (g["steer"][ab] == 0).all()
        assert (g["speed"][ab] == 0).all() and (g["best_seq"][ab] == 0).all() and (g["warm"][ab] == 0).all()
    assert (got["tag"][ids] == (2 if dyn else 1)).all()                 # an all-blocked ego's tag is its branch's too


@pytest.mark.parametrize("n_sub,n_sub_k", [(1, 2), (4, 1)])
def test_plan_batch_tests_both_branches(ctx, orc, n_sub, n_sub_k):
    """the mixed batch against both halves of the helper; then the egos AND their obstacle rows permuted together (with the grid on as well):
    each ego's result is the helper's for its new place -- an obstacle row indexed by a branch's compact index would follow the wrong ego"""
    E, T, R = 48, 40, 128
    s = O.scene_mixed()
    dcfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=TK, n_rollouts=R)
    _install(ctx, s)
    perm = np.random.default_rng(4).permutation(E)
    for x0, obs, collide in ((s["x0"], s["obs"], False), (np.ascontiguousarray(s["x0"][perm]), np.ascontiguousarray(s["obs"][perm]), True)):
        ctx.stmpc_set_collision(collide, n_sub, n_sub_k)
        stmpc_set_obstacles(ctx, obs)
        ctx.stmpc_warm_reset()
        got = _batch(ctx, x0, dcfg, kcfg, SEED, CALL)
        branch, d, k = O.expected_batch(orc, x0, s["wp"], dcfg, kcfg, obs, n_sub, n_sub_k, SEED, CALL, grid=s["grid"] if collide else None)
        np.testing.assert_array_equal(got["branch"], branch)
        _check_half(got, d, T, True)
        _check_half(got, k, TK, False)
        assert (d["all_blocked"] & ~d["fragile"]).any() and (k["all_blocked"] & ~k["fragile"]).any()
        assert ((d["best_idx"] != d["free_idx"]) & ~d["all_blocked"]).any() and ((k["best_idx"] != k["free_idx"]) & ~k["all_blocked"]).any()
        assert np.isnan(got["best_seq"][k["ids"], TK:]).all()


def test_chain_with_moving_obstacles_equals_the_expected_chain(ctx, orc):
    """four plan_batch calls (reference extraction on the device, warm start carried on the context), the discs advanced at their velocities
    between calls, against the helper's chain, ego by ego until an ego's first fragile call.  The parked disc on the first station of egos
    3::8 is taken away after the first call: those egos are all-blocked and stopped, their warm start zeroed -- and free in the next call
    (put back at 2.5 m/s, so that they stay in the dynamic branch)."""
    E, T, R, n_sub = 24, 40, 128, 2
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    ctx.stmpc_set_collision(False, n_sub, 2)
    dcfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=TK, n_rollouts=R)
    x, warm, obs = s["x0"].copy(), np.zeros((E, T, 2), np.float32), s["obs"].copy()
    ctx.stmpc_warm_reset()
    alive, prev_blocked, freed = np.ones(E, bool), None, 0
    for call in range(4):
        stmpc_set_obstacles(ctx, obs)
        got = _batch(ctx, x, dcfg, kcfg, 1234, call)
        assert (got["branch"] == 1).all() and (got["tag"] == 2).all()
        want = O.expected(orc, x, O.oracle_ref(orc, x, s["wp"], T), dcfg, obs, n_sub, 1234, call, warm=warm)
        alive &= ~want["fragile"]
        _check_against({k: got[k][alive] for k in KEYS + ("warm",)}, {k: v[alive] for k, v in want.items()})
        if prev_blocked is not None:
            now_free = prev_blocked & ~want["all_blocked"] & alive
            freed += int(now_free.sum())
            assert (warm[now_free] == 0).all()                           # what the all-blocked call left them with
        prev_blocked = want["all_blocked"] & alive
        assert (got["speed"][prev_blocked] == 0).all() and (got["warm"][prev_blocked] == 0).all()
        warm = np.where(alive[:, None, None], want["warm"], got["warm"])   # (an ego that was fragile follows the device: it is no longer compared)
        spd = np.maximum(np.where(alive, want["speed"], got["speed"]), 2.5)
        x[:, 0] += O.DT * spd * np.cos(x[:, 4]); x[:, 1] += O.DT * spd * np.sin(x[:, 4]); x[:, 3] = spd
        obs[:, :, 0] += O.DT * obs[:, :, 2]; obs[:, :, 1] += O.DT * obs[:, :, 3]
        obs[:, 3] = O.EMPTY
    assert freed >= 1 and alive.mean() > 0.5


def test_a_plan_does_not_depend_on_the_batch_around_it(ctx, orc):
    T, R, n_sub = 40, 128, 4
    s = _scene(orc, "t", 300, T)
    want = _want(orc, "t", 48, T, R, n_sub)
    pick = int(np.nonzero((want["best_idx"] != want["free_idx"]) & ~want["all_blocked"])[0][0])     # an ego that takes a detour
    s48 = _scene(orc, "t", 48, T)
    ego, ego_obs = s48["x0"][pick], s48["obs"][pick]
    _install(ctx, s, grid=False)
    ctx.stmpc_set_collision(False, n_sub)
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    ref0 = O.oracle_ref(orc, ego[None], s["wp"], T)
    first = None
    for E in (1, 63, 300):
        x0 = s["x0"][:E].copy(); x0[0] = ego
        obs = s["obs"][:E].copy(); obs[0] = ego_obs
        stmpc_set_obstacles(ctx, obs)
        got = _plan(ctx, x0, np.concatenate([ref0, s["ref"][1:E]]), cfg, None)
        one = {k: got[k][0] for k in KEYS + ("warm",)}
        if first is None:
            first = one
            assert one["best_idx"] >= 0
        for k in one:
            np.testing.assert_array_equal(one[k], first[k], err_msg=f"{k} E={E}")


def test_a_borrowed_device_array_equals_the_copied_one(ctx, orc):
    """f1p_stmpc_set_obstacles_dev: the same plan, and the array rewritten in place is the next plan's"""
    E, T, R, n_sub = 48, 40, 128, 2
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    ctx.stmpc_set_collision(False, n_sub)
    moved = s["obs"].copy(); moved[:, :, 0] += 0.3 * moved[:, :, 2]; moved[:, :, 1] += 0.3 * moved[:, :, 3]; moved[:, 3] = O.EMPTY
    want = []
    for obs in (s["obs"], moved):
        stmpc_set_obstacles(ctx, obs)
        want.append(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)))
    assert (want[0]["best_idx"] != want[1]["best_idx"]).any()
    d_obs = ctx.to_device(s["obs"])
    stmpc_set_obstacles_dev(ctx, d_obs, E, s["obs"].shape[1])
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), want[0])
    d_obs.upload(moved)                                                 # in place, no second set
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T)), want[1])
    _same(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T), streamed=True), want[1], keys=KEYS)
    with pytest.raises(ValueError, match="E and M"):
        stmpc_set_obstacles_dev(ctx, d_obs)
    stmpc_set_obstacles_dev(ctx, None)
    d_obs.free()
    off = _plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(E, T))
    assert (off["best_idx"] >= 0).all()


@pytest.mark.parametrize("case", O.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_on_the_device(ctx, case):
    """zero controls, so every rollout is the straight line p_t = (0.125 t, 0): blocked means best_idx -1, free means rollout 0 -- through
    the generated plan (sigma 0, no warm start) and through the streamed entry point, each in both modes"""
    _, x0, T, n_sub, obs, blocked = case
    R = 4
    cfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R, dt=O.HAND_DT)
    x0 = np.array([x0], np.float64); ref = np.zeros((1, 7, T + 1))
    ctx.stmpc_set_collision(False, n_sub)
    stmpc_set_obstacles(ctx, np.array([obs], np.float64))
    want = -1 if blocked else 0
    zero = dict(sigma_steer_v=0.0, sigma_accel=0.0, sigma_steer=0.0)
    for mixed in (True, False):
        got = _plan(ctx, x0, ref, cfg, None, mixed=mixed, sig=zero)
        assert got["best_idx"][0] == want, f"generated, mixed={mixed}"
        assert (got["speed"][0] == 0.0) == blocked and (got["best_cost"][0] == np.inf) == blocked
        ctx.stmpc_set_mode(mixed)
        try:
            got = ctx.stmpc_shoot(x0, ref, np.zeros((1, T, 2, R), np.float32), cfg)
        finally:
            ctx.stmpc_set_mode(True)
        assert got["best_idx"][0] == want, f"streamed, mixed={mixed}"


def test_the_two_obstacle_states_do_not_reach_each_other(ctx, orc):
    """f1p_stmpc_set_obstacles leaves f1p_kmpc_plan_batch as it is, and f1p_kmpc_set_obstacles leaves f1p_stmpc_plan_batch (its kinematic
    branch runs the kmpc kernel) and f1p_stmpc_plan_dev as they are"""
    E, T, R = 48, 40, 128
    s = O.scene_mixed()
    dcfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=TK, n_rollouts=R)
    _install(ctx, s, grid=False)
    ksmp = _abi.kmpc_sampler(seed=SEED, call=CALL, use_warm=False, sigma_accel=1.5, sigma_steer=0.15)
    xk = O.xy4(s["x0"])
    ctx.stmpc_warm_reset()
    off = _batch(ctx, s["x0"], dcfg, kcfg, SEED, CALL)
    koff = ctx.kmpc_plan(xk, kcfg, ksmp)
    kobs = O.KO.traffic(xk, TK)
    kmpc_set_obstacles(ctx, kobs)                                        # the kmpc state alone
    kon = ctx.kmpc_plan(xk, kcfg, ksmp)
    assert (kon["best_idx"] != koff["best_idx"]).any()
    ctx.stmpc_warm_reset()
    _same(_batch(ctx, s["x0"], dcfg, kcfg, SEED, CALL), off, keys=KEYS[:4] + ("branch", "warm", "tag"), msg="kmpc obstacles, stmpc plan")
    kmpc_set_obstacles(ctx, None)
    stmpc_set_obstacles(ctx, s["obs"])                                   # the stmpc state alone
    ctx.stmpc_warm_reset()
    son = _batch(ctx, s["x0"], dcfg, kcfg, SEED, CALL)
    kin = off["branch"] == 0
    assert (son["best_idx"][kin] != off["best_idx"][kin]).any() and (son["best_idx"][~kin] != off["best_idx"][~kin]).any()
    _same(ctx.kmpc_plan(xk, kcfg, ksmp), koff, keys=KEYS, msg="stmpc obstacles, kmpc plan")


def test_clearing_one_obstacle_state_leaves_the_other_in_force(ctx, orc):
    """the two states are set and cleared by one function: kmpc discs for (E 2, M 1), OTHER discs for the dynamic MPC with (E 3, M 2), the
    kmpc ones cleared -- the stmpc plan is the expected one with its own discs and its own shape, the kmpc plan the unobstructed one"""
    T, R, n_sub = 4, 64, 2
    s = dict(_scene(orc, "t", 3, 40))                                    # (the traffic scene needs a longer horizon; only its egos and course are used)
    s["ref"] = O.oracle_ref(orc, s["x0"], s["wp"], T)
    cfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    ksmp = _abi.kmpc_sampler(seed=SEED, call=CALL, use_warm=False, sigma_accel=1.5, sigma_steer=0.15)
    _install(ctx, s, grid=False)
    ctx.stmpc_set_collision(False, n_sub)
    xk = O.xy4(s["x0"][:2])
    obs = np.empty((3, 2, 5)); obs[:] = O.EMPTY
    obs[0, 1] = (s["x0"][0, 0], s["x0"][0, 1], 0.0, 0.0, 0.5)            # parked on ego 0: every rollout of it is blocked
    obs[2, 0] = (s["x0"][2, 0] + 50.0, s["x0"][2, 1], 0.0, 0.0, 0.3)     # out of ego 2's reach
    kobs = np.array([[(xk[0, 0], xk[0, 1], 0.0, 0.0, 0.5)], [O.EMPTY]])  # [2, 1, 5]: parked on the kinematic ego 0
    koff = ctx.kmpc_plan(xk, kcfg, ksmp)
    kmpc_set_obstacles(ctx, kobs)
    kon = ctx.kmpc_plan(xk, kcfg, ksmp)
    assert kon["best_idx"][0] == -1 and koff["best_idx"][0] >= 0
    stmpc_set_obstacles(ctx, obs)
    kmpc_set_obstacles(ctx, None)
    want = O.expected(orc, s["x0"], s["ref"], cfg, obs, n_sub, SEED, CALL, warm=O.warm_start(3, T))
    assert want["all_blocked"][0] and not want["all_blocked"][1:].any()
    _check_against(_plan(ctx, s["x0"], s["ref"], cfg, O.warm_start(3, T)), want)
    _same(ctx.kmpc_plan(xk, kcfg, ksmp), koff, keys=KEYS, msg="kmpc obstacles cleared")


def test_the_rejections(ctx, orc):
    """each returns its error code and a text, launches nothing, leaves the outputs untouched and the warm-start tags as they were"""
    from f1tenth_planning_amd.runtime import F1PError
    E, T, R = 8, 40, 64
    cfg, kcfg = _abi.stmpc_cfg(horizon=T, n_rollouts=R), _abi.kmpc_cfg(horizon=TK, n_rollouts=R)
    s = _scene(orc, "t", E, T)
    _install(ctx, s, grid=False)
    obs = s["obs"]
    tags = np.array([2, 1, 0, 2, 2, 1, 0, 2], np.int32)
    warm = O.warm_start(E, T)

    def rejected(code, text, E_, dev=True, batch=True):
        ctx.stmpc_warm_set(warm, tags, T, TK)
        d_x0, d_ref = ctx.to_device(s["x0"][:E_]), ctx.to_device(s["ref"][:E_])
        sizes = (8 * E_, 8 * E_, 4 * E_, 8 * E_, 16 * E_ * T)
        d_ctrl = ctx.to_device(synth.make_controls(E_, T, R))
        for streamed in (False, True) if dev else ():
            d = [ctx.alloc(n) for n in sizes]
            for b, n in zip(d, sizes):
                b.upload(np.full(n, 0x5A, np.uint8))
            with pytest.raises(F1PError, match=text) as ei:
                if streamed:
                    ctx.stmpc_shoot_dev(d_x0, d_ref, d_ctrl, E_, cfg, *d)
                else:
                    ctx.stmpc_plan_dev(d_x0, d_ref, E_, cfg, _sampler(1, 0), *d)
            assert ei.value.code == code
            ctx.sync()
            for b, n in zip(d, sizes):
                assert (b.download(np.uint8, (n,)) == 0x5A).all()
                b.free()
        if batch:
            with pytest.raises(F1PError, match=text) as ei:
                ctx.stmpc_plan(s["x0"][:E_], cfg, kcfg, _sampler(1, 0))
            assert ei.value.code == code
        if dev:
            with pytest.raises(F1PError, match=text):
                ctx.stmpc_shoot(s["x0"][:E_], s["ref"][:E_], synth.make_controls(E_, T, R), cfg)
        w, t = ctx.stmpc_warm_get(E, T, TK)
        np.testing.assert_array_equal(t, tags); np.testing.assert_array_equal(w, warm)
        for b in (d_x0, d_ref, d_ctrl):
            b.free()

    for bad in (17, -1, 100):                                           # 1. M outside [1, 16]: nothing changes
        big = np.zeros((E, max(bad, 1), 5))
        assert ctx.lib.f1p_stmpc_set_obstacles(ctx.h, big.ctypes.data, E, bad) == _abi.F1P_EINVAL
        assert b"M must be in [1, 16]" in ctx.lib.f1p_last_error(ctx.h)
        d_big = ctx.to_device(big)
        assert ctx.lib.f1p_stmpc_set_obstacles_dev(ctx.h, d_big.ptr, E, bad) == _abi.F1P_EINVAL
        d_big.free()
    with pytest.raises(ValueError, match="M must be"):
        stmpc_set_obstacles(ctx, np.zeros((E, 17, 5)))
    with pytest.raises(ValueError, match=r"\[E, M, 5\]"):
        stmpc_set_obstacles(ctx, np.zeros((E, 4)))
    stmpc_set_obstacles(ctx, obs)                                        # 2. a plan of another E (plan_batch: the caller's E)
    rejected(_abi.F1P_ESTATE, "obstacles were set for 8 egos", 5)
    ctx.kmpc_set_groups(2)                                              # 3. forced workgroups per ego: plan_batch's kinematic branch
    rejected(_abi.F1P_ESTATE, "f1p_kmpc_set_groups", E, dev=False)
    ctx.kmpc_set_groups(0)
    got = _plan(ctx, s["x0"], s["ref"], cfg, warm, fill=0x5A)             # ... and with everything in order the same call plans
    assert np.isfinite(got["steer"]).all() and (got["best_idx"] >= -1).all() and (got["best_idx"] < R).all() and (got["best_idx"] == -1).any()


def test_planner_class(orc):
    from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
    E, T, R = 48, 40, 128
    s = O.scene_mixed()
    wp, obs = s["wp"], s["obs"]
    course = [wp[:, 0].copy(), wp[:, 1].copy(), wp[:, 3].copy(), wp[:, 2].copy()]
    conf = mpc_config(T=T, N_ROLLOUTS=R, SEED=5, COLLISION_SUBSTEPS=2, COLLISION_SUBSTEPS_K=2)

    def planner(obstacles=None):
        pl = STMPCPlanner(waypoints=[c.copy() for c in course], config=conf)
        assert pl.obstacles is None
        pl.obstacles = obstacles
        return pl

    free = planner().plan_batch(s["x0"])
    pl = planner(obs)
    with_obs = pl.plan_batch(s["x0"])
    assert pl.obstacles is None                                         # the obstacles are one call's: it takes them
    blocked = with_obs["best_idx"] == -1
    for b in (1, 0):
        assert blocked[with_obs["branch"] == b].any()
    assert (free["best_idx"] >= 0).all() and (with_obs["best_idx"] != free["best_idx"]).mean() >= 0.25
    assert (with_obs["steer"][blocked] == 0).all() and (with_obs["speed"][blocked] == 0).all() and np.isinf(with_obs["best_cost"][blocked]).all()
    np.testing.assert_array_equal(with_obs["branch"], free["branch"])
    pl.reset()                                                          # reset(): the call counter and the warm start; no obstacles are left
    again = pl.plan_batch(s["x0"])
    for k in KEYS[:4] + ("u",):
        np.testing.assert_array_equal(again[k], free[k], err_msg=k)
    pl.obstacles = obs                                                  # ... and a planner that has planned without takes them as well
    pl.reset()
    once_more = pl.plan_batch(s["x0"])
    for k in KEYS[:4] + ("u",):
        np.testing.assert_array_equal(once_more[k], with_obs[k], err_msg=k)
    # plan(): both branches; the warning and (0, 0) on all-blocked; an open road otherwise, also right after (no leftovers in either state)
    for b in (1, 0):
        e = int(np.nonzero(blocked & (with_obs["branch"] == b))[0][0])
        pl3 = planner(obs[e])
        with pytest.warns(RuntimeWarning, match="blocked"):
            assert pl3.plan(s["x0"][e]) == (0.0, 0.0)
        assert pl3.obstacles is None and (pl3.oa == 0).all() and (pl3.odelta_v == 0).all()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            st, sp = pl3.plan(s["x0"][e])
        assert not [w for w in rec if "blocked" in str(w.message)]
        assert abs(st) <= 0.4189 + 1e-12 and sp > 0.0
        quiet = int(np.nonzero((np.arange(E) % 5 == 4) & (with_obs["branch"] == b))[0][0])      # an ego without a live slot
        pl3.obstacles = obs[quiet]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            st, sp = pl3.plan(s["x0"][quiet])
        assert not [w for w in rec if "blocked" in str(w.message)]
        assert abs(st) <= 0.4189 + 1e-12 and sp > 0.0
