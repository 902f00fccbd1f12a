"""The shooting MPC's moving-obstacle test on the host: the class's argument checks, the symbols in header and prototypes, the disc
rule's hand cases on the numpy restatement, and scene "traffic" -- the helper alone (tests/kmpc_obstacle_ref.py, oracle calls and numpy
only) must meet the scene conditions and the cap on "fragile" egos, so that the GPU test compares decisions the test really decides."""
import os
import re

import numpy as np
import pytest

import kmpc_obstacle_ref as O
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(48, 8, 128, 1), (48, 8, 128, 4), (16, 30, 512, 2), (1, 8, 64, 1)]          # (E, T, R, n_sub)


def _planner(**kw):
    s = O.scene_traffic(4, 8)
    wp = s["wp"]
    return KMPCPlanner(waypoints=[wp[:, 0], wp[:, 1], wp[:, 3], wp[:, 2]], config=mpc_config(**kw)), s


def _state7(x):
    return np.array([x[0], x[1], 0.0, x[2], x[3], 0.0, 0.0])


def test_obstacles_with_the_qp_solver_are_a_value_error():
    pl, s = _planner(SOLVER="qp")
    with pytest.raises(ValueError, match="obstacles"):
        pl.obstacles = s["obs"]
        pl.plan_batch(s["x0"])
    with pytest.raises(ValueError, match="obstacles"):
        pl.obstacles = s["obs"][0]
        pl.plan(_state7(s["x0"][0]))
    assert pl._ctx is None                                              # nothing touched the GPU


@pytest.mark.parametrize("shape", [(4, 4), (3, 4, 5), (4, 4, 4), (4, 0, 5), (4, 2, 5, 1)])
def test_a_wrong_shape_is_a_value_error(shape):
    pl, s = _planner()
    with pytest.raises(ValueError, match="obstacles"):
        pl.obstacles = np.zeros(shape)
        pl.plan_batch(s["x0"])
    assert pl._ctx is None


@pytest.mark.parametrize("shape", [(5,), (2, 4), (1, 2, 5)])
def test_plan_takes_m_by_5(shape):
    pl, s = _planner()
    with pytest.raises(ValueError, match="obstacles"):
        pl.obstacles = np.zeros(shape)
        pl.plan(_state7(s["x0"][0]))
    assert pl._ctx is None


def test_more_than_16_obstacles_are_a_value_error():
    pl, s = _planner()
    with pytest.raises(ValueError, match="16"):
        pl.obstacles = np.zeros((4, 17, 5))
        pl.plan_batch(s["x0"])
    with pytest.raises(ValueError, match="16"):
        pl.obstacles = np.zeros((17, 5))
        pl.plan(_state7(s["x0"][0]))
    assert pl._ctx is None


@pytest.mark.parametrize("n_sub", [0, 17, -1])
def test_substeps_outside_1_16_with_obstacles_is_a_value_error(n_sub):
    """COLLISION off: the number still serves the obstacles"""
    pl, s = _planner()
    pl.config = mpc_config(COLLISION_SUBSTEPS=n_sub)
    with pytest.raises(ValueError, match="COLLISION_SUBSTEPS"):
        pl.obstacles = s["obs"]
        pl.plan_batch(s["x0"])
    with pytest.raises(ValueError, match="COLLISION_SUBSTEPS"):
        pl.obstacles = s["obs"][0]
        pl.plan(_state7(s["x0"][0]))
    assert pl._ctx is None


def test_symbols_in_header_and_prototypes():
    hdr = open(os.path.join(ROOT, "include", "f1p.h")).read()
    assert re.search(r"int\s+f1p_kmpc_set_obstacles\(f1p_ctx\*\s*ctx,\s*const\s+double\*\s*obs,\s*int32_t\s+E,\s*int32_t\s+M\);", hdr)
    assert re.search(r"int\s+f1p_kmpc_set_obstacles_dev\(f1p_ctx\*\s*ctx,\s*const\s+double\*\s*d_obs,\s*int32_t\s+E,\s*int32_t\s+M\);", hdr)
    assert re.search(r"#define\s+F1P_KMPC_MAX_OBS\s+16\b", hdr) and O.MAX_OBS == 16
    for name in ("f1p_kmpc_set_obstacles", "f1p_kmpc_set_obstacles_dev"):
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == 4
    from f1tenth_planning_amd import runtime
    assert callable(runtime.kmpc_set_obstacles) and callable(runtime.kmpc_set_obstacles_dev)
    assert KMPCPlanner(config=mpc_config()).obstacles is None
    with pytest.raises(ValueError, match="E and M"):                    # a borrowed array needs its shape (raised before the library is touched)
        runtime.Context._kmpc_set_obstacles_dev(None, object())
    # no field was added to the structs the oracle mirrors
    assert [f[0] for f in _abi.KmpcSampler._fields_] == ["seed", "call", "use_warm", "sigma_accel", "sigma_steer"]


@pytest.mark.parametrize("E,T,R,n_sub", SHAPES)
def test_scene_traffic_meets_its_conditions(orc, E, T, R, n_sub):
    """conditions, not measurements: the unconstrained winner is blocked in >= 25 % of the egos, nothing changes in >= 25 %, at least one ego
    is all-blocked, one takes a detour, fragile egos are <= 2 % of the batch (a one-ego batch can only be checked for the cap)"""
    s = O.scene_traffic(E, T)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    ref = O.oracle_ref(orc, s["x0"], s["wp"], T)
    w = O.expected(orc, s["x0"], ref, cfg, s["obs"], n_sub, seed=11, call=3, warm=O.warm_start(E, T))
    assert w["fragile"].mean() <= 0.02
    if E > 1:
        assert (w["best_idx"] != w["free_idx"]).mean() >= 0.25
        assert (w["best_idx"] == w["free_idx"]).mean() >= 0.25
        assert w["all_blocked"].sum() >= 1
        assert ((w["best_idx"] != w["free_idx"]) & ~w["all_blocked"]).sum() >= 1
        quiet = np.zeros(E, bool); quiet[4::5] = True                   # egos without a live slot: the plan without obstacles
        parked = np.zeros(E, bool); parked[3::8] = True                 # the parked disc on the first station
        assert w["all_blocked"][parked & ~quiet].all()
        np.testing.assert_array_equal(w["best_idx"][quiet], w["free_idx"][quiet])
    ab = w["all_blocked"]
    assert (w["best_idx"][ab] == -1).all() and np.isinf(w["best_cost"][ab]).all() and (w["best_seq"][ab] == 0).all() and (w["warm"][ab] == 0).all()


def test_a_rejected_call_has_taken_the_obstacles():
    """the attribute is per call: a call takes it, also one that raises"""
    pl, s = _planner(SOLVER="qp")
    pl.obstacles = s["obs"]
    with pytest.raises(ValueError, match="obstacles"):
        pl.plan_batch(s["x0"])
    assert pl.obstacles is None and pl._ctx is None


@pytest.mark.parametrize("E,T,R,n_sub", [(48, 8, 128, 4), (16, 30, 512, 2)])
def test_sixteen_live_discs_meet_the_conditions(orc, E, T, R, n_sub):
    s = O.scene_traffic(E, T)
    obs = O.crowd16(s["x0"], T)
    assert obs.shape == (E, 16, 5) and (obs[:, :, 4] >= 0).all()
    reach = np.maximum(s["x0"][:, 2], 6.0) * T * 0.1                     # every one of them within the horizon's reach: none is dropped
    d = np.hypot(obs[:, :, 0] - s["x0"][:, None, 0], obs[:, :, 1] - s["x0"][:, None, 1])
    assert (d - obs[:, :, 4] - np.hypot(obs[:, :, 2], obs[:, :, 3]) * T * 0.1 <= reach[:, None]).all()
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    w = O.expected(orc, s["x0"], O.oracle_ref(orc, s["x0"], s["wp"], T), cfg, obs, n_sub, seed=11, call=3, warm=O.warm_start(E, T))
    assert w["fragile"].mean() <= 0.02
    assert (w["best_idx"] != w["free_idx"]).mean() >= 0.25 and (~w["all_blocked"]).mean() >= 0.25 and w["all_blocked"].any()


def test_without_a_live_slot_the_helper_is_the_oracles_plan(orc):
    E, T, R = 16, 8, 64
    s = O.scene_traffic(E, T)
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=R)
    ref = O.oracle_ref(orc, s["x0"], s["wp"], T)
    obs = np.empty((E, 3, 5)); obs[:] = O.EMPTY; obs[:, 1, 4] = np.nan; obs[:, 2, :4] = np.nan
    w = O.expected(orc, s["x0"], ref, cfg, obs, 4, seed=11, call=3, warm=O.warm_start(E, T))
    want = orc.kmpc_plan_batch(s["x0"], ref, cfg, 11, 3, 1.5, 0.15, warm=O.warm_start(E, T), nthreads=8)
    np.testing.assert_array_equal(w["best_idx"], want["best_idx"])
    np.testing.assert_array_equal(w["warm"], want["warm"])
    assert (w["n_tested"] == 1).all() and not w["fragile"].any()


# ---- the disc rule's hand cases (tests/test_gpu_kmpc_obstacles.py runs the same ones on the device) ----------------------------------------
@pytest.mark.parametrize("case", O.hand_cases(), ids=lambda c: c[0])
def test_hand_cases_on_the_rule(orc, case):
    _, x0, T, n_sub, obs, blocked = case
    cfg = _abi.kmpc_cfg(horizon=T, n_rollouts=2)
    path = orc.predict_motion_kinematic(np.array(x0), np.zeros(T), np.zeros(T), cfg)
    if np.isfinite(x0).all():
        np.testing.assert_array_equal(path[0], 0.25 * np.arange(T + 1)); np.testing.assert_array_equal(path[1], 0.0)
    else:
        assert np.isnan(path[:2, 1:]).any(axis=0).all()                 # every tested point has a NaN coordinate
    pts = O.tested_points(path, n_sub)
    hit, _, _ = O.disc_blocked(pts, O.point_times(T, n_sub, cfg.dt), np.array(obs, np.float64))
    assert hit == blocked


def test_point_times_follow_the_formula():
    tau = O.point_times(3, 4, 0.1)
    assert tau.shape == (12,)
    assert tau[0] == (0.0 + 1.0 / 4.0) * 0.1 and tau[3] == (0.0 + 1.0) * 0.1 and tau[4] == (1.0 + 1.0 / 4.0) * 0.1 and tau[11] == 3.0 * 0.1
    np.testing.assert_array_equal(O.point_times(5, 1, 0.1), (np.arange(5) + 1.0) * 0.1)
