"""f1p_lattice_set_obstacles on the CPU: the disc rule's hand cases, the public surface (header, _abi, runtime, class), and the scene of the
GPU tests -- the reference (tests/lattice_obstacle_ref.py, oracle calls and numpy only) must meet the scene's conditions and the cap on
"fragile" egos, so that tests/test_gpu_lattice_obstacles.py compares something that means something."""
import os
import re

import numpy as np
import pytest

import lattice_obstacle_ref as O
from f1tenth_planning_amd import _abi, runtime
from f1tenth_planning_amd.planning.lattice_planner.lattice_planner import LatticePlanner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS9 = ("steer", "speed", "best_idx", "best_cost", "status", "near_idx", "best_traj", "all_cost", "all_traj")


@pytest.fixture(scope="module")
def scene(orc):
    s = O.make_scene(orc)
    s["want"] = O.expected(orc, s["poses"], s["rl"], s["cfg"], s["obs"], s["pace"], grid=s["grid"], base=s["base"])
    return s


# ---- the public surface ------------------------------------------------------------------------------------------------------------------
def test_header_abi_runtime_and_class_agree():
    hdr = open(os.path.join(ROOT, "include", "f1p.h")).read()
    assert re.search(r"#define\s+F1P_LATTICE_MAX_OBS\s+16", hdr)
    assert re.search(r"int\s+f1p_lattice_set_obstacles\(f1p_ctx\*\s*ctx,\s*const\s+double\*\s*obs,\s*const\s+double\*\s*pace,\s*int32_t\s+E,\s*int32_t\s+M\);", hdr)
    assert re.search(r"int\s+f1p_lattice_set_obstacles_dev\(f1p_ctx\*\s*ctx,\s*const\s+double\*\s*d_obs,\s*const\s+double\*\s*d_pace,\s*int32_t\s+E,\s*int32_t\s+M\);", hdr)
    for words in ("blocked when !(d2 > rr)", "ax = ct*dx0 + st*dy0; ay = ct*dy0 - st*dx0", "tau_j = s_j * pace[e]", "a slot with !(r >= 0) is empty"):
        assert words in hdr, words
    for name in ("f1p_lattice_set_obstacles", "f1p_lattice_set_obstacles_dev"):
        assert len(_abi.PROTOTYPES[name][1]) == 5
    assert callable(runtime.lattice_set_obstacles) and callable(runtime.lattice_set_obstacles_dev)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5l" in design and "f1p_lattice_set_obstacles" in design
    p = LatticePlanner.__new__(LatticePlanner)
    LatticePlanner.__init__(p, device=0)
    assert p.obstacles is None and p.obstacle_min_speed == 0.5


def test_runtime_rejects_bad_shapes_before_the_library():
    with pytest.raises(ValueError):
        runtime.Context._lattice_set_obstacles(None, np.zeros((3, 5)), np.ones(3))
    with pytest.raises(ValueError):
        runtime.Context._lattice_set_obstacles(None, np.zeros((3, 2, 5)), None)
    with pytest.raises(ValueError):
        runtime.Context._lattice_set_obstacles(None, np.zeros((3, 2, 5)), np.ones(4))
    with pytest.raises(ValueError):
        runtime.Context._lattice_set_obstacles_dev(None, object(), None, 3, 2)


def test_class_takes_the_attribute_and_checks_the_shape():
    p = LatticePlanner(device=0)
    p.obstacles = np.zeros((2, 17, 5))
    with pytest.raises(ValueError, match="at most 16"):
        p.plan_batch(np.zeros((2, 4)))
    assert p.obstacles is None                                  # taken, also when the call raises
    p.obstacles = np.zeros((3, 2, 5))
    with pytest.raises(ValueError, match=r"\[E=2, M, 5\]"):
        p.plan_batch(np.zeros((2, 4)))
    assert p.obstacles is None
    p.obstacles = np.zeros((2, 5, 5))
    with pytest.raises(ValueError, match=r"\[M, 5\]"):
        p.plan(0.0, 0.0, 0.0, 1.0)
    assert p.obstacles is None
    p.obstacles = np.zeros((2, 2, 5))
    with pytest.raises(ValueError, match="multi-GPU"):
        p.plan_batch(np.zeros((2, 4)), devices=[0, 1])
    assert p.obstacles is None
    p.obstacles = np.zeros((3, 2, 5))
    with pytest.raises(ValueError, match=r"\[E=2, M, 5\]"):
        p.step_batch(np.zeros((2, 4)))
    assert p.obstacles is None


# ---- hand cases of the rule --------------------------------------------------------------------------------------------------------------
POSE0 = np.array([0.0, 0.0, 0.0, 1.0])


def test_touching_blocks_and_just_outside_does_not():
    live = O.slot_transform(POSE0, [[1.0, 0.0, 0.0, 0.0, 0.5]])
    assert O.point_blocked(live, 0.5, 0.0, 0.0)                 # d2 == rr: touching blocks
    assert O.point_blocked(live, 0.75, 0.0, 0.0)
    assert not O.point_blocked(live, 0.5 - 1e-9, 0.0, 0.0)
    live0 = O.slot_transform(POSE0, [[1.0, 0.0, 0.0, 0.0, 0.0]])
    assert O.point_blocked(live0, 1.0, 0.0, 0.0) and not O.point_blocked(live0, 1.0, 1e-100, 1.0)   # r = 0: only the centre itself


def test_nan_blocks_and_empty_slots_do_not():
    for bad in ([np.nan, 0.0, 0.0, 0.0, 0.1], [50.0, np.nan, 0.0, 0.0, 0.1], [50.0, 0.0, np.nan, 0.0, 0.1], [50.0, 0.0, 0.0, np.inf, 0.1]):
        live = O.slot_transform(POSE0, [bad])
        assert len(live) == 1 and O.point_blocked(live, 0.0, 0.0, 0.0), bad        # (inf velocity at tau = 0: 0 * inf = NaN)
    assert len(O.slot_transform(POSE0, [[0.0, 0.0, 0.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.0, np.nan], [0.0, 0.0, 0.0, 0.0, -0.0]])) == 1   # -0.0 >= 0: live
    live = O.slot_transform(POSE0, [[50.0, 0.0, 0.0, 0.0, 0.1]])
    assert O.point_blocked(live, 0.0, 0.0, np.nan)              # a NaN pace: tau is NaN, every point of the ego is blocked
    assert not O.point_blocked(np.zeros((0, 5)), 0.0, 0.0, np.nan)   # ... unless the ego has no live slot
    assert O.point_blocked(O.slot_transform(POSE0, [[50.0, 0.0, 0.0, 0.0, np.inf]]), 0.0, 0.0, 0.0)


def test_pace_zero_parks_every_disc_and_time_orders_the_meeting():
    rows = np.zeros((5, 4)); rows[:, 0] = np.arange(5) * 1.0    # a straight candidate, stations 1 m apart
    slot = [[2.0, -2.0, 0.0, 1.0, 0.25]]                        # crosses the path at x = 2 at t = 2 s
    live = O.slot_transform(POSE0, slot)
    for pace, want in ((1.0, True), (0.0, False), (0.5, False), (2.0, False)):
        tau = O.station_times(rows, 4.0, pace, cubic=False)
        got = any(O.point_blocked(live, rows[j, 0], rows[j, 1], tau[j]) for j in range(5))
        assert got == want, pace
    np.testing.assert_array_equal(O.station_times(rows, 4.0, 0.25, cubic=True), np.arange(5) * 0.25)   # chord sums of this path = its abscissae


def test_slot_transform_is_the_ego_frame():
    pose = np.array([1.0, 2.0, np.pi / 2, 1.0])
    live = O.slot_transform(pose, [[1.0, 5.0, 0.0, -1.0, 0.5]])     # 3 m ahead, coming towards the ego
    np.testing.assert_allclose(live[0], [3.0, 0.0, -1.0, 0.0, 0.25], atol=1e-15)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
def test_host_goals_reproduce_device_goals_bit_for_bit(orc, scene):
    s = scene
    g = O.host_goals(orc, s["poses"], s["rl"], s["cfg"])
    a = s["base"]
    b = orc.lattice_plan_batch(s["poses"], s["rl"], s["cfg"], grid=s["grid"], goals=g, want_all=True)
    for k in KEYS9:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_masking_goals_yields_the_argmin_of_the_masked_costs(scene):
    w = scene["want"]
    ok = ~w["all_blocked"]
    np.testing.assert_array_equal(w["best_idx"][ok], w["argmin"][ok])
    np.testing.assert_array_equal(w["best_cost"][ok], w["all_cost"][ok, w["argmin"][ok]])


def test_scene_meets_its_conditions(scene):
    s, w = scene, scene["want"]
    E = s["E"]
    newly = w["blocked"].sum(axis=1)
    changed = int((w["best_idx"] != s["base"]["best_idx"]).sum())
    print(f"fragile {int(w['fragile'].sum())} of {E}; winners changed {changed}; distinct winners {len(set(w['best_idx'].tolist()))}; "
          f"newly blocked per ego {newly.mean():.1f}; all-blocked egos {int(w['all_blocked'].sum())}")
    assert w["fragile"].sum() <= 0.02 * E
    assert not w["all_blocked"].any()
    assert changed >= 0.9 * E                                   # slot 0 sits on the obstacle-free winner
    assert len(set(w["best_idx"].tolist())) >= 8
    assert newly.mean() >= 5.0
    assert (np.isfinite(s["base"]["all_cost"]) & ~w["blocked"]).any(axis=1).all()
    assert np.isnan(s["obs"][:, 2, 0]).all() and (s["obs"][:, 2, 4] == -1.0).all()
