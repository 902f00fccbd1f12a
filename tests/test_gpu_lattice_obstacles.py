"""f1p_lattice_set_obstacles: the lattice planner's candidates tested against moving discs -- against the expected results composed from the
oracle and the numpy disc rule (tests/lattice_obstacle_ref.py), the mixed schedule against the all-fp64 kernel bit for bit (every mode, with a
previous path, with and without a map, cfg.check_collision off, cfg.prune, the audit), every plan shape, the edge cases of the rule, the closed
loop, the pipeline, and the errors of the C-ABI and the class."""
import ctypes as C

import numpy as np
import pytest

import lattice_obstacle_ref as O
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.runtime import F1PError, lattice_set_obstacles, lattice_set_obstacles_dev
from lattice_helpers import compare

pytestmark = pytest.mark.gpu
KEYS = ("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj")


def _copy_cfg(cfg, **fields):
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


@pytest.fixture(scope="module")
def scenes(orc):
    out = {}

    def get(E=96, generator="clothoid"):
        key = (E, generator)
        if key not in out:
            s = O.make_scene(orc, E=E, generator=generator)
            s["want"] = O.expected(orc, s["poses"], s["rl"], s["cfg"], s["obs"], s["pace"], grid=s["grid"], base=s["base"])
            out[key] = s
        return out[key]
    return get


@pytest.fixture()
def ctx_of():
    from f1tenth_planning_amd.runtime import Context
    made = []

    def make(s, grid=True, mode=1, waypoints=True):
        c = Context(0)
        made.append(c)
        if waypoints:
            c.set_waypoints(s["rl"])
        if grid:
            c.set_grid(s["img"], O.RES, s["origin"], O.OCC_BELOW)
        c.lattice_set_mode(mode)
        return c
    yield make
    for c in made:
        c.close()


def _same(a, b, keys=KEYS, what=""):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")     # (NaN == NaN: assert_array_equal's rule)


def _sub(d, m, keys=KEYS):
    return {k: d[k][m] for k in keys}


def _keep(d, keys=KEYS):
    return {k: np.array(d[k], copy=True) for k in keys if k in d}


# ---- against the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,E", [(0, 96), (1, 96), (2, 96), (3, 96), (1, 97), (2, 97)])
def test_scene_against_the_reference(scenes, ctx_of, mode, E):
    s = scenes(E)
    w = s["want"]
    ctx = ctx_of(s, mode=mode)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = ctx.lattice_plan(s["poses"], s["cfg"])
    m = ~w["fragile"] & ~w["all_blocked"]
    assert m.mean() >= 0.98
    compare(_sub(got, m), _sub(w, m))
    assert (got["best_idx"] != s["base"]["best_idx"]).mean() > 0.9     # the discs do change the plans


# ---- bit-identity across the schedules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "prev", "no_map", "no_check", "prev+no_map"])
def test_mixed_schedules_equal_the_all_fp64_kernel_bit_for_bit(scenes, ctx_of, variant):
    s = scenes(97)
    E, S = s["E"], s["cfg"].n_stations
    prev = np.random.default_rng(11).normal(0, 0.15, (E, S)) if "prev" in variant else None
    cfg = _copy_cfg(s["cfg"], check_collision=0) if variant == "no_check" else s["cfg"]
    ctx = ctx_of(s, grid="no_map" not in variant, mode=0)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    ref = _keep(ctx.lattice_plan(s["poses"], cfg, prev_theta=prev))
    free = _keep(ctx_of(s, grid="no_map" not in variant, mode=0).lattice_plan(s["poses"], cfg, prev_theta=prev))
    assert (ref["best_idx"] != free["best_idx"]).mean() > 0.5           # (the discs matter in this variant too)
    for mode in (1, 2, 3):
        ctx.lattice_set_mode(mode)
        _same(ctx.lattice_plan(s["poses"], cfg, prev_theta=prev), ref, what=f"{variant} mode {mode}")


def test_prune_on_equals_off_and_the_audit_reads_no_mismatch(scenes, ctx_of):
    s = scenes(97)
    ctx = ctx_of(s, mode=0)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    ref = _keep(ctx.lattice_plan(s["poses"], s["cfg"]))
    pruned = _copy_cfg(s["cfg"], prune=1)
    for mode in (0, 1):
        ctx.lattice_set_mode(mode)
        _same(ctx.lattice_plan(s["poses"], pruned), ref, what=f"prune, mode {mode}")
    ctx.lattice_set_mode(1)
    ctx.lattice_set_audit(1, 64)
    ctx.lattice_audit_read(reset=True)
    for _ in range(3):                                                  # three windows of 64 of the 97 egos
        _same(ctx.lattice_plan(s["poses"], s["cfg"]), ref, what="audited plan")
    assert ctx.lattice_audit_read() == dict(plans=3, egos=192, mismatching_egos=0)
    ctx.lattice_set_audit(0, 0)


# ---- plan shapes -------------------------------------------------------------------------------------------------------------------------
def _modes_0_and_1(ctx, plan):
    ctx.lattice_set_mode(0)
    a = _keep(plan(), KEYS + ("all_cost", "all_traj"))
    ctx.lattice_set_mode(1)
    b = plan()
    _same(b, a, keys=[k for k in a], what="mode 1 against mode 0")
    return a


def _against(got, w):
    m = ~w["fragile"] & ~w["all_blocked"]
    assert m.mean() >= 0.9
    compare(_sub(got, m), _sub(w, m))


def test_shape_host_goals(orc, scenes, ctx_of):
    s = scenes(96)
    g = O.host_goals(orc, s["poses"], s["rl"], s["cfg"])
    ctx = ctx_of(s)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan(s["poses"], s["cfg"], goals=g))
    _against(got, s["want"])                                            # (host goals from orc.lattice_goals: the device goals' plan)


def test_shape_cubic(scenes, ctx_of):
    s = scenes(96, "cubic")
    ctx = ctx_of(s)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan(s["poses"], s["cfg"]))
    _against(got, s["want"])
    assert s["want"]["blocked"].sum(axis=1).mean() > 3.0


def test_shape_oriented_footprint(orc, scenes, ctx_of):
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    s = scenes(96)
    offsets, radius = LatticePlanner(waypoints=s["rl"]).set_footprint(length=0.58, width=0.31, n_discs=3, center_offset=0.145)
    assert len(offsets) == 3
    grid_img = orc.inflate_image(s["img"], O.RES, O.OCC_BELOW, radius, nthreads=8)
    orc.set_footprint(offsets)
    try:
        w = O.expected(orc, s["poses"], s["rl"], s["cfg"], s["obs"], s["pace"], grid=(grid_img, O.RES, s["origin"][0], s["origin"][1], O.OCC_BELOW),
                       foot=offsets)
    finally:
        orc.set_footprint(())
    ctx = ctx_of(s)
    ctx.set_footprint(offsets, radius)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan(s["poses"], s["cfg"]))
    _against(got, w)
    assert (w["blocked"].sum(axis=1) > s["want"]["blocked"].sum(axis=1)).any()   # the disc centres reach further than the station points


def test_shape_track_set_with_a_bad_id(orc, scenes, ctx_of):
    s = scenes(96)
    rl = s["rl"]
    lane = rl.copy()
    lane[:, 0] -= 0.3 * np.sin(rl[:, 3]); lane[:, 1] += 0.3 * np.cos(rl[:, 3]); lane[:, 2] = rl[:, 2] * 1.03
    tracks = [rl, np.ascontiguousarray(lane)]
    ids = (np.arange(s["E"]) % 2).astype(np.int32)
    ids[5] = 7
    ctx = ctx_of(s, waypoints=False)
    ctx.set_tracks(tracks)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan_tracks(s["poses"], ids, s["cfg"]))
    for k in (0, 1):
        sel = ids == k
        w = O.expected(orc, s["poses"][sel], tracks[k], s["cfg"], s["obs"][sel], s["pace"][sel], grid=s["grid"])
        _against(_sub(got, sel), w)
    assert got["status"][5] == _abi.ST_BAD_TRACK and np.isnan(got["steer"][5]) and got["best_idx"][5] == -1
    st = ctx.lattice_step_tracks(s["poses"], ids, s["cfg"], keep_traj=True)     # the step: the same plan (no previous path yet)
    np.testing.assert_array_equal(st["steer"], got["steer"]); np.testing.assert_array_equal(st["status"], got["status"])
    np.testing.assert_array_equal(ctx.lattice_fetch_traj(s["E"], s["cfg"].n_stations), got["best_traj"])


def test_shape_f32_rows(scenes, ctx_of):
    s = scenes(96)
    ctx = ctx_of(s)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan(s["poses"], s["cfg"], traj_dtype=np.float32))
    assert got["best_traj"].dtype == np.float32
    ref = ctx.lattice_plan(s["poses"], s["cfg"])
    _same(got, ref, keys=KEYS[:-1])
    np.testing.assert_array_equal(got["best_traj"], ref["best_traj"].astype(np.float32))
    _against(dict(ref), s["want"])


def test_shape_all_cost_and_all_traj(scenes, ctx_of):
    s = scenes(96)
    w = s["want"]
    ctx = ctx_of(s)
    free = _keep(ctx.lattice_plan(s["poses"], s["cfg"], want_all=True), KEYS + ("all_cost", "all_traj"))
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    got = _modes_0_and_1(ctx, lambda: ctx.lattice_plan(s["poses"], s["cfg"], want_all=True))
    _against(got, w)
    sure = ~(np.abs(w["pen"]) <= O.DISC_EPS)                            # candidates whose disc verdict does not hang on 1e-9 m
    np.testing.assert_array_equal(np.isposinf(got["all_cost"])[sure], np.isposinf(w["all_cost"])[sure])
    keep = np.isfinite(got["all_cost"])
    np.testing.assert_array_equal(got["all_cost"][keep], free["all_cost"][keep])          # an unblocked candidate keeps its cost,
    np.testing.assert_array_equal(got["all_traj"], free["all_traj"])                      # ... and every candidate its rows
    assert (np.isposinf(got["all_cost"]) & np.isfinite(free["all_cost"])).sum() == w["blocked"].sum()


# ---- edge cases --------------------------------------------------------------------------------------------------------------------------
def test_disc_over_the_ego_empty_slots_far_discs_and_a_nan_pace(scenes, ctx_of):
    s = scenes(96)
    E = s["E"]
    ctx = ctx_of(s)
    free = _keep(ctx.lattice_plan(s["poses"], s["cfg"]))
    q_free = ctx.lattice_debug_queue(E).copy()
    # a disc over the ego itself: everything blocked; an ego whose slots are all empty: the plan without obstacles
    obs = np.full((E, 3, 5), np.nan); obs[:, :, 4] = -1.0
    obs[0, 1] = (s["poses"][0, 0], s["poses"][0, 1], 0.0, 0.0, 0.5)
    for mode in (0, 1):
        ctx.lattice_set_mode(mode)
        lattice_set_obstacles(ctx, obs, s["pace"])
        got = ctx.lattice_plan(s["poses"], s["cfg"])
        assert got["status"][0] == _abi.ST_ALL_BLOCKED and got["steer"][0] == 0.0 and got["speed"][0] == 0.0 and np.isposinf(got["best_cost"][0])
        _same(_sub(got, slice(1, None)), _sub(free, slice(1, None)), what=f"empty slots, mode {mode}")
    # discs 100 m away: the same bits, and the filter has not sent the batch to fp64
    far = s["obs"].copy()
    far[:, :, 0] += 100.0
    ctx.lattice_set_mode(1)
    lattice_set_obstacles(ctx, far, s["pace"])
    _same(ctx.lattice_plan(s["poses"], s["cfg"]), free, what="far discs")
    np.testing.assert_array_equal(ctx.lattice_debug_queue(E), q_free)
    # a NaN pace blocks that ego only
    pace = s["pace"].copy(); pace[3] = np.nan
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    ref = _keep(ctx.lattice_plan(s["poses"], s["cfg"]))
    for mode in (0, 1):
        ctx.lattice_set_mode(mode)
        lattice_set_obstacles(ctx, s["obs"], pace)
        got = ctx.lattice_plan(s["poses"], s["cfg"])
        assert got["status"][3] == _abi.ST_ALL_BLOCKED and np.isposinf(got["best_cost"][3])
        m = np.arange(E) != 3
        _same(_sub(got, m), _sub(ref, m), what=f"NaN pace, mode {mode}")


# ---- closed loop, device arrays, pipeline ------------------------------------------------------------------------------------------------
def test_three_steps_equal_the_chain_of_three_plans(scenes, ctx_of):
    s = scenes(96)
    E, S = s["E"], s["cfg"].n_stations
    cfg = _copy_cfg(s["cfg"], w_similarity=0.4)
    a, b = ctx_of(s), ctx_of(s)
    b.lattice_set_closed_loop(True)
    winners = []
    for k in range(3):
        obs = s["obs"].copy()
        obs[:, :, 0] += obs[:, :, 2] * 0.1 * k; obs[:, :, 1] += obs[:, :, 3] * 0.1 * k      # the caller advances the discs between steps
        lattice_set_obstacles(a, obs, s["pace"]); lattice_set_obstacles(b, obs, s["pace"])
        st = a.lattice_step(s["poses"], cfg, keep_traj=True)
        pl = b.lattice_plan(s["poses"], cfg)
        for key in ("steer", "speed", "status"):
            np.testing.assert_array_equal(st[key], pl[key], err_msg=f"step {k} {key}")
        np.testing.assert_array_equal(a.lattice_fetch_traj(E, S), pl["best_traj"])
        winners.append(pl["best_idx"].copy())
    assert (winners[0] != winners[2]).any()                             # the chain does move


def test_borrowed_device_arrays_rewritten_in_place_equal_the_copies(scenes, ctx_of):
    s = scenes(96)
    E, M = s["obs"].shape[:2]
    a, b = ctx_of(s), ctx_of(s)
    d_obs, d_pace = a.alloc(s["obs"].nbytes), a.alloc(s["pace"].nbytes)
    d_obs.upload(s["obs"]); d_pace.upload(s["pace"])
    lattice_set_obstacles_dev(a, d_obs, d_pace, E, M)
    for k in range(2):
        obs = s["obs"].copy()
        obs[:, :, 0] += 0.25 * k
        d_obs.upload(obs)                                               # in place, between plans
        lattice_set_obstacles(b, obs, s["pace"])
        _same(a.lattice_plan(s["poses"], s["cfg"]), b.lattice_plan(s["poses"], s["cfg"]), what=f"plan {k}")
    lattice_set_obstacles_dev(a, None)
    d_obs.free(); d_pace.free()


def test_pipelined_plan_equals_the_unpipelined_one(scenes, ctx_of):
    s = scenes(97)
    ctx = ctx_of(s)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    ref = _keep(ctx.lattice_plan(s["poses"], s["cfg"]))
    ctx.lattice_set_pipeline(3)
    _same(ctx.lattice_plan(s["poses"], s["cfg"]), ref, what="three chunks")
    ctx.lattice_set_pipeline(0)


# ---- errors and contract -----------------------------------------------------------------------------------------------------------------
def test_errors_launch_nothing_and_change_nothing(scenes, ctx_of):
    s = scenes(96)
    E = s["E"]
    ctx = ctx_of(s)
    lattice_set_obstacles(ctx, s["obs"], s["pace"])
    ref = _keep(ctx.lattice_plan(s["poses"], s["cfg"]))
    with pytest.raises(ValueError):                                      # M = 17: F1P_EINVAL
        lattice_set_obstacles(ctx, np.zeros((E, 17, 5)), s["pace"])
    rc = ctx.lib.f1p_lattice_set_obstacles(ctx.h, s["obs"].ctypes.data_as(C.c_void_p), None, E, 4)
    assert rc == _abi.F1P_EINVAL                                         # no pace
    with pytest.raises(F1PError) as ei:                                  # another batch size
        ctx.lattice_plan(s["poses"][:50], s["cfg"])
    assert ei.value.code == _abi.F1P_ESTATE
    with pytest.raises(F1PError) as ei:                                  # a candidate shard
        ctx.lattice_plan(s["poses"], _copy_cfg(s["cfg"], cand_begin=0, cand_count=40), want_traj=False)
    assert ei.value.code == _abi.F1P_ESTATE
    with pytest.raises(F1PError) as ei:
        ctx.lattice_set_split(2)
    assert ei.value.code == _abi.F1P_ESTATE
    d_pose = ctx.to_device(s["poses"]); d_idx = ctx.to_device(ref["best_idx"]); d_cost = ctx.to_device(ref["best_cost"])
    d_steer, d_speed = ctx.alloc(8 * E), ctx.alloc(8 * E)
    d_steer.upload(np.full(E, 7.0))
    with pytest.raises(F1PError) as ei:
        ctx.lattice_emit_dev(d_pose, E, s["cfg"], d_idx, d_cost, d_steer, d_speed)
    assert ei.value.code == _abi.F1P_ESTATE
    np.testing.assert_array_equal(d_steer.download(np.float64, (E,)), 7.0)   # nothing was launched
    for bffr in (d_pose, d_idx, d_cost, d_steer, d_speed):
        bffr.free()
    _same(ctx.lattice_plan(s["poses"], s["cfg"]), ref, what="after the refused calls")   # the discs are still in force, the split is not
    lattice_set_obstacles(ctx, s["obs"][:, :0], s["pace"])               # M = 0 clears
    free = ctx_of(s).lattice_plan(s["poses"], s["cfg"])
    _same(ctx.lattice_plan(s["poses"], s["cfg"]), free, what="cleared")
    ctx.lattice_set_split(2); ctx.lattice_set_split(0)                   # ... and a split may be forced again
    ctx.lattice_set_split(2)
    with pytest.raises(F1PError) as ei:                                  # setting discs while a split is forced
        lattice_set_obstacles(ctx, s["obs"], s["pace"])
    assert ei.value.code == _abi.F1P_ESTATE
    ctx.lattice_set_split(0)


def test_class_takes_the_obstacles_and_the_next_plan_has_none(scenes):
    from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner
    s = scenes(96)

    def planner():
        p = LatticePlanner(waypoints=s["rl"], device=0)
        p.set_map(s["img"], O.RES, s["origin"], occupied_thresh=1.0 - (O.OCC_BELOW - 0.5) / 255.0)     # occupied below 206
        p.configure(lookahead_distances=np.linspace(0.6, 3.0, 16), widths=np.linspace(-1.0, 1.0, 5), weights=(0.25, 0.25, 0.25, 0.25), num_stations=20)
        return p
    p, fresh = planner(), planner()
    assert p._map[3] == O.OCC_BELOW
    free = _keep(fresh.plan_batch(s["poses"]))
    assert p.obstacle_min_speed == 0.5
    p.obstacles = s["obs"]
    got = p.plan_batch(s["poses"])
    assert p.obstacles is None
    m = ~s["want"]["fragile"]
    compare(_sub(got, m), _sub(s["want"], m))                            # pace = 1 / max(|v|, 0.5) from the velocity column
    _same(p.plan_batch(s["poses"]), free, what="the plan after one with obstacles")
    p.obstacles = s["obs"]
    st = p.step_batch(s["poses"])
    assert p.obstacles is None
    np.testing.assert_array_equal(st["steer"], got["steer"])
    e = 4
    p.obstacles = s["obs"][e]
    steer, speed, traj = p.plan(*s["poses"][e])
    assert p.obstacles is None and steer == got["steer"][e] and speed == got["speed"][e]
    np.testing.assert_array_equal(traj, got["best_traj"][e])
    steer2, _, _ = p.plan(*s["poses"][e])                                # a plan() without obstacles after one with: none are in force
    f = planner()
    f.prev_traj = traj                                                   # (plan() carries the previous winner: like with like)
    assert steer2 == f.plan(*s["poses"][e])[0] and p.obstacles is None
