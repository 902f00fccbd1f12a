"""The f32 filter's FREE verdict where it is final: f1p_kmpc_plan_dev with best_cost == NULL emits a single survivor on the filter's word
(csrc/k_kmpc.hip, `n_eff == 1 && !best_cost`).  The scenes of tests/shoot_graze_ref.py put one tested point of the would-be winner within
1e-8 m .. twice the filter's allowance of a disc's rim (or a cell's edge), inside or outside it; tests/test_shoot_graze_host.py holds the
scenes' own conditions.

Per batch: the control run without obstacles reaches n_refined == 1 on at least 90 % of the egos (measured on the MI355X: 48 of 48 egos,
share 1.000, in all six batches and in both batches of the dynamic planner's kinematic branch); with
the obstacles, mixed mode gives the expected winner on every decisive ego, equals plain fp64 bit for bit on every ego, and the call without
best_cost equals the call with it."""
import numpy as np
import pytest

import shoot_graze_ref as G
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.runtime import kmpc_set_obstacles

pytestmark = pytest.mark.gpu

KEYS = ("steer", "speed", "best_idx", "best_seq", "warm")


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c
        kmpc_set_obstacles(c, None)
        c.kmpc_set_collision(False)


@pytest.fixture(autouse=True)
def _clean(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        kmpc_set_obstacles(c, None)
        c.kmpc_set_collision(False, 1)
        c.kmpc_set_mode(True)


def _plan(ctx, b, mixed=True, want_cost=True):
    """f1p_kmpc_plan_dev on the batch's egos, reference and warm start -> outputs, the warm start it left, n_refined"""
    cfg = b["cfg"]
    E, T = b["x0"].shape[0], cfg.horizon
    smp = _abi.kmpc_sampler(seed=G.SEED, call=G.CALL, use_warm=True, sigma_accel=G.SIGMA[0], sigma_steer=G.SIGMA[1])
    ctx.kmpc_warm_set(b["warm"])
    d_x0, d_ref = ctx.to_device(b["x0"]), ctx.to_device(b["ref"])
    sizes = dict(steer=8 * E, speed=8 * E, best_idx=4 * E, best_cost=8 * E, best_seq=16 * E * T)
    d = {k: ctx.alloc(v) for k, v in sizes.items()}
    for k in d:
        d[k].upload(np.full(sizes[k], 0x5A, np.uint8))
    d_nref = ctx.alloc(4 * E)
    d_nref.upload(np.full(E, -99, np.int32))
    ctx.kmpc_set_mode(mixed, None, d_nref)
    try:
        ctx.kmpc_plan_dev(d_x0, d_ref, E, cfg, smp, d["steer"], d["speed"], d["best_idx"], d["best_cost"] if want_cost else None, d["best_seq"])
        ctx.sync()
    finally:
        ctx.kmpc_set_mode(True)
    out = dict(steer=d["steer"].download(np.float64, (E,)), speed=d["speed"].download(np.float64, (E,)),
               best_idx=d["best_idx"].download(np.int32, (E,)), best_cost=d["best_cost"].download(np.float64, (E,)),
               best_seq=d["best_seq"].download(np.float64, (E, T, 2)), n_refined=d_nref.download(np.int32, (E,)),
               warm=ctx.kmpc_warm_get(E, T))
    if not want_cost:                                                   # the buffer was not passed: nothing wrote to it
        assert (d["best_cost"].download(np.uint8, (8 * E,)) == 0x5A).all()
    for buf in list(d.values()) + [d_x0, d_ref, d_nref]:
        buf.free()
    return out


def _install(ctx, b, grid=None):
    ctx.set_waypoints(b["wp"], cols=(0, 1, 2, 3))
    if grid is None:
        ctx.set_grid(None, 0, (0, 0), 0)
    else:
        img, res, ox, oy, occ = grid
        ctx.set_grid(img, res, (ox, oy), occ)


def _three_assertions(ctx, b, win, decisive, what):
    """the expected winner on the decisive egos; mixed == plain fp64 on every ego; without best_cost == with it"""
    bare = _plan(ctx, b, want_cost=False)
    full = _plan(ctx, b)
    plain = _plan(ctx, b, mixed=False)
    wrong = decisive & (bare["best_idx"] != win)
    by_rung = [int((wrong & (b["rung"] == k)).sum()) for k in range(G.N_RUNGS)]
    print(f"{what}: n_refined == 1 on {int((bare['n_refined'] == 1).sum())} egos, wrong winners per rung {by_rung} "
          f"(inside {int((wrong & b['inside']).sum())}, outside {int((wrong & ~b['inside']).sum())})")
    assert not wrong.any(), (what, by_rung, np.nonzero(wrong)[0].tolist())
    np.testing.assert_array_equal(plain["best_idx"][decisive], win[decisive])
    assert (plain["n_refined"] == -1).all() and (bare["n_refined"] != -99).all()
    for k in KEYS:
        np.testing.assert_array_equal(bare[k], plain[k], err_msg=f"{what}: mixed without best_cost vs plain fp64: {k}")
        np.testing.assert_array_equal(full[k], plain[k], err_msg=f"{what}: mixed vs plain fp64: {k}")
    np.testing.assert_array_equal(full["best_cost"], plain["best_cost"])
    return bare


@pytest.mark.parametrize("name,T,n_sub", G.BATCHES)
def test_control_run_reaches_the_single_survivor(ctx, orc, name, T, n_sub):
    """no obstacle: the filter keeps one survivor, rollout 0, and best_cost == NULL emits it unrefined"""
    b = G.build(orc, name, T, n_sub)
    _install(ctx, b)
    got = _plan(ctx, b, want_cost=False)
    share = float((got["n_refined"] == 1).mean())
    print(f"control {name} T={T}: n_refined == 1 on {share:.3f} of the egos")
    assert share >= 0.9
    clear = b["gap0"] >= 10.0                                            # the long-double winner leads by 10 margins: every ego of these scenes
    assert clear.mean() >= 0.9 and (got["n_refined"][clear] == 1).mean() >= 0.9
    np.testing.assert_array_equal(got["best_idx"][clear], b["free_win"][clear])
    assert (got["best_idx"][b["decisive"]] == 0).all()
    plain = _plan(ctx, b, mixed=False)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)


@pytest.mark.parametrize("name,T,n_sub", G.BATCHES)
def test_a_disc_grazing_the_winner(ctx, orc, name, T, n_sub):
    b = G.build(orc, name, T, n_sub)
    _install(ctx, b)
    ctx.kmpc_set_collision(False, n_sub)
    kmpc_set_obstacles(ctx, b["obs"])
    bare = _three_assertions(ctx, b, b["win"], b["decisive"], f"disc {name} T={T} n_sub={n_sub}")
    # the outside egos beyond the allowance are FREE and final: the path under test is reached with the obstacle in place
    far = b["decisive"] & ~b["inside"] & (b["delta"] > 1.5 * b["allow"])
    assert far.any() and (bare["n_refined"][far] == 1).all()


@pytest.mark.parametrize("name,T,n_sub", G.BATCHES)
def test_a_disc_grazing_the_winner_with_the_occupancy_test_on(ctx, orc, name, T, n_sub):
    """the scene's image without an occupied cell and f1p_kmpc_set_collision on: the discs' proof beside the clearance look-ups"""
    b = G.build(orc, name, T, n_sub)
    _install(ctx, b, grid=b["grid"])
    ctx.kmpc_set_collision(True, n_sub)
    kmpc_set_obstacles(ctx, b["obs"])
    _three_assertions(ctx, b, b["win"], b["decisive_grid"], f"disc + open grid {name} T={T} n_sub={n_sub}")


@pytest.mark.parametrize("name,T", G.GRID_BATCHES)
def test_a_single_cell_under_an_interior_sub_point(ctx, orc, name, T):
    """one occupied cell per ego, delta inside or outside one of its edges, the neighbouring tested points more than four cells away:
    the grid alone, then with a bystander disc per ego (the discs' kernel with the bitmap)"""
    b = G.build_grid(orc, name, T)
    _install(ctx, b, grid=b["grid"])
    ctx.kmpc_set_collision(True, b["n_sub"])
    _three_assertions(ctx, b, b["win"], b["decisive"], f"cell {name} T={T}")
    kmpc_set_obstacles(ctx, b["obs"])
    _three_assertions(ctx, b, b["win"], b["decisive_both"], f"cell + bystander disc {name} T={T}")


def _stmpc_plan(ctx, b, dcfg, mixed=True, want_cost=True):
    """Context.stmpc_plan with every ego in the kinematic branch -> outputs, the warm start it left, the kinematic kernels' n_refined"""
    kcfg = b["cfg"]
    E, T, TK = b["x0"].shape[0], dcfg.horizon, kcfg.horizon
    W = max(T, TK)
    warm = np.zeros((E, W, 2), np.float32); warm[:, :TK] = b["warm"]
    ctx.stmpc_warm_set(warm, np.full(E, 1), T, TK)
    smp = _abi.stmpc_sampler(seed=G.SEED, call=G.CALL, use_warm=True, sigma_accel=G.SIGMA[0], sigma_steer=G.SIGMA[1])
    d_nref = ctx.alloc(4 * E)
    d_nref.upload(np.full(E, -99, np.int32))
    ctx.kmpc_set_mode(mixed, None, d_nref)                              # the kinematic branch runs f1p_kmpc_plan_*'s schedule under f1p_kmpc_set_mode
    try:
        out = ctx.stmpc_plan(b["x7"], dcfg, kcfg, smp, v_ks=G.STMPC_V_KS, want_cost=want_cost)
        ctx.sync()
    finally:
        ctx.kmpc_set_mode(True)
    out["n_refined"] = d_nref.download(np.int32, (E,))
    d_nref.free()
    w, tag = ctx.stmpc_warm_get(E, T, TK)
    out["warm"] = w[:, :TK]
    out["best_seq"] = out["best_seq"][:, :TK]
    assert (out["branch"] == 0).all() and (tag == 1).all()
    return out


@pytest.mark.parametrize("name,T,n_sub", G.STMPC_BATCHES)
def test_a_disc_grazing_the_winner_in_stmpc_plans_kinematic_branch(ctx, orc, name, T, n_sub):
    """k_kmpc_plan_gen_idx_obs emits on the filter's word as well: stmpc_plan(want_cost=False), every ego at or below v_ks"""
    from f1tenth_planning_amd.runtime import stmpc_set_obstacles
    b = G.build(orc, name, T, n_sub, stmpc=True)
    dcfg = _abi.stmpc_cfg(horizon=8, n_rollouts=G.R)
    _install(ctx, b)
    ctx.stmpc_set_collision(False, 1, n_sub)
    try:
        stmpc_set_obstacles(ctx, None)
        free = _stmpc_plan(ctx, b, dcfg, want_cost=False)
        clear = b["gap0"] >= 10.0
        print(f"stmpc control {name} T={T}: n_refined == 1 on {float((free['n_refined'] == 1).mean()):.3f} of the egos")
        assert (free["n_refined"][clear] == 1).mean() >= 0.9
        np.testing.assert_array_equal(free["best_idx"][clear], b["free_win"][clear])
        stmpc_set_obstacles(ctx, b["obs"])
        bare = _stmpc_plan(ctx, b, dcfg, want_cost=False)
        full = _stmpc_plan(ctx, b, dcfg)
        plain = _stmpc_plan(ctx, b, dcfg, mixed=False)
    finally:
        stmpc_set_obstacles(ctx, None)
        ctx.stmpc_set_collision(False)
    d = b["decisive"]
    wrong = d & (bare["best_idx"] != b["win"])
    print(f"stmpc disc {name} T={T}: n_refined == 1 on {int((bare['n_refined'] == 1).sum())} egos, wrong winners {np.nonzero(wrong)[0].tolist()}")
    assert not wrong.any()
    np.testing.assert_array_equal(plain["best_idx"][d], b["win"][d])
    for k in KEYS:
        np.testing.assert_array_equal(bare[k], plain[k], err_msg=f"mixed without best_cost vs plain fp64: {k}")
        np.testing.assert_array_equal(full[k], plain[k], err_msg=f"mixed vs plain fp64: {k}")
    np.testing.assert_array_equal(full["best_cost"], plain["best_cost"])
