"""Wall rows of the dynamic QP on the host: the march against a brute-force scan on the GPU tests' scenes; the scenes hold the
families they claim, the yardstick certifies every ego of every shape (the long shapes from the golden record g24, on the problems rebuilt
here) and none is edge-sensitive; the closed loop emulated with the yardstick alone; the class's checks raise before the library is reached
and its switch reaches f1p_stmpc_qp_set_walls (on the stub library of tools/record_runtime_calls.py); the header's names.  No GPU."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import kmpc_qp_ref as KQ
import stmpc_qp_ref as SQ
import stmpc_qp_walls_ref as W
import stmpc_qp_walls_scenes as SC
import tracker_ref as TR
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._planner import qp_walls
from f1tenth_planning_amd.control.dynamic_mpc import dynamic_mpc as DM
from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import mpc_config as kin_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. scenes, record, yardstick ---------------------------------------------------------------------------------------------------------
def test_shapes_take_both_launch_paths_and_end_at_the_cap():
    B = SC.B()
    lds = lambda T: int(_abi.load_library().f1p_stmpc_qp_avoid_lds_bytes(T))       # noqa: E731
    assert lds(B - 1) <= 64 * 1024 < lds(B) and lds(SC.CAP) <= 160 * 1024
    assert SC.shapes() == ((2, 0), (10, 0), (10, 4), (24, 4), (B, 0), (40, 16)) and SC.CAP == 40
    assert {SC.family_of(e) for e in range(SC.n_egos(SC.CAP))} == set(SC.FAMILIES)      # the 16 egos of the cap's batch cover every family


@pytest.mark.parametrize("T,M", SC.shapes())
def test_march_equals_the_brute_force_scan(T, M):
    """every step of every ego's linearisation path, both sides, at the scenes' reach and one past it"""
    x0, ref, oa, odv, obs, fam = SC.scene(T, M)
    p, grid = SQ.default_params(T), SC.grid_of()
    hits = set()
    for e in range(SC.n_egos(T)):
        if e in fam["nan_state"]:
            continue
        path = SQ.predict_motion(x0[e], oa[e], odv[e], p)
        for t in range(1, T + 1):
            hd = W.heading(path, t)
            for sg in (1.0, -1.0):
                lx, ly = -sg * math.sin(hd), sg * math.cos(hd)
                for n in (SC.N_SAMPLES, SC.N_SAMPLES + 1):
                    k = W.march(grid, path[0, t], path[1, t], lx, ly, n)[0]
                    assert k == W.brute_first_hit(grid, path[0, t], path[1, t], lx, ly, n), (e, t, sg, n)
                    hits.add(k)
    assert {0, 1, SC.N_SAMPLES, SC.N_SAMPLES + 1} <= hits


@pytest.mark.parametrize("T,M", SC.shapes())
def test_scenes_hold_their_families_and_certify(T, M):
    """what tests/test_gpu_stmpc_qp_walls.py asserts from the yardstick's output: every family, a certified exact optimum for every feasible
    ego of every shape, none edge-sensitive; the egos are above V_KS and the previous solution is not zero"""
    x0, ref, oa, odv, obs, fam = SC.scene(T, M)
    ok = np.setdiff1d(np.arange(len(x0)), fam["v0_out"] + fam["nan_state"])
    assert (x0[ok, 3] > 2.0).all() and np.abs(oa).max() > 0 and np.abs(odv).max() > 0
    sols = SC.solutions(T, M)
    SC.assert_families(T, M, sols)
    assert sum(s is not None for s in sols) == len(ok)
    assert SC.uncertified(sols) == 0 and SC.edge_sensitive(sols) == []
    feas = [s for s in sols if s is not None]
    assert sum((s["avoid_lam"][:-1] > 1e-6).any() for s in feas) >= 2                    # the rows bind somewhere
    assert sum(s["eps"] > 1e-4 for s in feas) >= 1 and sum(abs(s["eps"]) <= 1e-9 for s in feas) >= 3


@pytest.mark.parametrize("T,M", [(2, 0), (10, 4)])
def test_golden_record_is_the_helpers_output(T, M):
    """the previous solutions of the short horizons computed again here (the long ones: tools/gen_golden_stmpc_qp_walls.py)"""
    oa, odv = SC.compute_prev(T)
    assert np.abs(oa - SC.scene(T, M)[2]).max() <= 1e-9 and np.abs(odv - SC.scene(T, M)[3]).max() <= 1e-9


def test_recorded_active_sets_are_the_optima():
    """T = 24 solved outright against the record's active set (the cap's shape takes a minute: the generator asserts it)"""
    T, M = 24, 4
    for rec, now in zip(SC.solutions(T, M), SC.solve_scene(T, M)):
        assert (rec is None) == (now is None)
        if rec is not None:
            assert np.abs(rec["w"] - now["w"]).max() <= 1e-9 and np.abs(rec["lam"] - now["lam"]).max() <= 1e-6 * (1.0 + np.abs(now["lam"]).max())


def test_no_candidate_is_the_plain_qp():
    T = 10
    x0, ref, oa, odv, obs, fam = SC.scene(T, 0)
    p = SQ.default_params(T)
    for e in fam["no_wall"]:
        s = SC.solutions(T, 0)[e]
        s0 = SQ.solve_case(x0[e], ref[e], oa[e], odv[e], p)
        assert len(s["build"]["rows"]) == 0 and abs(s["eps"]) <= 1e-12 and np.abs(s["u"] - s0["u"]).max() <= 1e-9


def test_closed_loop_emulated_with_the_yardstick_alone():
    """the GPU test's closed loop with the yardstick as the planner: at least 95 % of the plans certified and not edge-sensitive, every plan in
    the dynamic branch, and the raceline does lead into the inflated band"""
    L = SC.LOOP
    T = L["T"]
    img, res, origin, (cx, cy, cyaw, sp) = SC.band_track()
    grid = SC.band_grid_inflated()
    p = SQ.default_params(T)
    s = SC.loop_start()
    prev = [None, None]
    good = plans = inside = 0
    for step in range(L["steps"]):
        for e in range(len(s)):
            assert s[e, 3] > 2.0
            ref = TR.stmpc_ref_ref(KQ.nearest_index(s[e, 0], s[e, 1], cx, cy), s[e, [0, 1, 3, 4]], cx, cy, cyaw, sp, T)
            sol = SC.loop_check(s[e], ref, prev[e], grid, True, T)
            plans += 1
            good += bool(sol["certified"] and not sol["edge"])
            inside += W.occupied(grid, s[e, 0], s[e, 1])
            prev[e] = (sol["u"][:, 1].copy(), sol["u"][:, 0].copy())
            s[e] = SQ.plant(s[e], sol["steer"], sol["speed"], p)
    assert good >= 0.95 * plans, (good, plans)
    assert W.occupied(grid, cx[40], cy[40]) and not W.occupied(grid, cx[-1], cy[-1])


# ---- 2. the class's checks, before the library is reached ------------------------------------------------------------------------------
def _stub():
    spec = importlib.util.spec_from_file_location("record_runtime_calls", os.path.join(ROOT, "tools", "record_runtime_calls.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.stub_context()


WP = np.zeros((4, 10))


def test_config_defaults_and_repr():
    c = mpc_config()
    assert (c.QP_WALLS_ST, c.QP_WALL_REACH, c.QP_WALL_MARGIN, c.QP_WALLS) == (False, 1.5, 0.0, False)
    assert "QP_WALL" not in repr(c) and "QP_WALL" not in repr(mpc_config(QP_WALLS_ST=True))
    assert not hasattr(kin_config(), "QP_WALLS_ST")
    assert qp_walls(c, 0.1) is None
    w = qp_walls(mpc_config(QP_WALLS_ST=True, QP_WALL_REACH=1.0, QP_WALL_MARGIN=0.05), 0.1)
    assert (w.on, w.n_samples, w.margin) == (1, 20, 0.05)


def test_the_old_field_still_raises_its_old_text():
    for kw in (dict(), dict(SOLVER="qp"), dict(SOLVER="qp", QP_WALLS_ST=True)):
        with pytest.raises(ValueError) as ei:
            STMPCPlanner(config=mpc_config(QP_WALLS=True, **kw))
        assert str(ei.value) == "QP_WALLS: KMPCPlanner only"


def test_qp_walls_st_needs_the_qp_solver_and_a_map():
    with pytest.raises(ValueError, match="QP_WALLS_ST adds wall rows to the QP"):
        STMPCPlanner(config=mpc_config(QP_WALLS_ST=True))
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True))
    with pytest.raises(ValueError, match="QP_WALLS_ST needs an occupancy grid"):
        pl.plan_batch(np.zeros((2, 7)), waypoints=WP)
    with pytest.raises(ValueError, match="QP_WALLS_ST needs an occupancy grid"):
        pl.plan(np.zeros(7), waypoints=WP)
    assert pl._ctx is None
    kc = kin_config(SOLVER="qp")
    kc.QP_WALLS_ST = True                                        # a field the kinematic planner's config does not have
    with pytest.raises(ValueError, match="QP_WALLS_ST: STMPCPlanner only"):
        KMPCPlanner(config=kc)


@pytest.mark.parametrize("field,value", [("QP_WALL_REACH", 0.0), ("QP_WALL_REACH", -1.0), ("QP_WALL_REACH", math.nan), ("QP_WALL_REACH", math.inf),
                                         ("QP_WALL_MARGIN", math.nan), ("QP_WALL_MARGIN", math.inf), ("T", 41), ("TK", 32)])
def test_bad_wall_numbers_raise_before_the_library(field, value):
    base = dict(T=40) if field == "TK" else {}
    with pytest.raises(ValueError):
        STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True, **base, **{field: value}))
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True, **base))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN)
    setattr(pl.config, field, value)
    pl._ctx.lib.log.clear()
    with pytest.raises(ValueError):
        pl.plan_batch(np.zeros((1, 7)), waypoints=WP)
    assert pl._ctx.lib.log == []
    STMPCPlanner(config=mpc_config(SOLVER="qp", **base, **{field: value}))      # off: the numbers are not read, the plain QP's caps hold


def test_reach_past_256_samples_names_reach_and_resolution():
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True, QP_WALL_REACH=12.81))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN)
    pl._ctx.lib.log.clear()
    with pytest.raises(ValueError, match=r"12\.81.*0\.1"):
        pl.plan_batch(np.zeros((1, 7)), waypoints=WP)
    assert pl._ctx.lib.log == []
    pl.config.QP_WALL_REACH = 12.8
    pl.plan_batch(np.zeros((1, 7)), waypoints=WP)                # 256 samples: the most


def test_switch_reaches_the_library(monkeypatch):
    """plan_batch with QP_WALLS_ST: f1p_stmpc_qp_set_walls(on, n_samples, margin) before the plan; off again after a plan without it;
    QP_AVOID's switch beside it untouched; plan, tracks, obstacles and rivals take it"""
    from f1tenth_planning_amd._rivals import Rivals
    seen = []
    real = DM.stmpc_qp_set_walls
    monkeypatch.setattr(DM, "stmpc_qp_set_walls", lambda ctx, w: (seen.append(None if w is None else (w.on, w.n_samples, w.margin)), real(ctx, w))[1])
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS_ST=True, QP_WALL_REACH=1.0, QP_WALL_MARGIN=0.05))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN, inflate=0.2)
    log = pl._ctx.lib.log
    assert [c[0] for c in log] == ["f1p_set_grid", "f1p_inflate_grid"]
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), waypoints=WP)
    names = [c[0] for c in log]
    assert seen == [(1, 20, 0.05)] and "f1p_stmpc_qp_set_avoid" not in names and "f1p_kmpc_qp_set_walls" not in names
    assert names.index("f1p_stmpc_qp_set_walls") < names.index("f1p_stmpc_qp_plan_batch")
    assert ["f1p_stmpc_qp_set_walls", ["ptr", "byref:KmpcQpWalls"]] in log
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), tracks=[WP, WP], track_ids=[0, 1])
    names = [c[0] for c in log]
    assert names.index("f1p_stmpc_qp_set_walls") < names.index("f1p_stmpc_qp_plan_tracks_batch")
    pl.config.QP_WALLS_ST = False
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), waypoints=WP)
    assert seen[-1] is None and ["f1p_stmpc_qp_set_walls", ["ptr", None]] in log
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), waypoints=WP)                # off after a plan with it off: nothing to switch
    assert "f1p_stmpc_qp_set_walls" not in [c[0] for c in log]
    # obstacles and rivals with it
    pl.config.QP_WALLS_ST = pl.config.QP_AVOID = True
    pl.obstacles = np.zeros((2, 1, 5))
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), waypoints=WP)
    names = [c[0] for c in log]
    assert {"f1p_stmpc_qp_set_walls", "f1p_stmpc_qp_set_avoid", "f1p_stmpc_set_obstacles", "f1p_stmpc_qp_plan_batch"} <= set(names)
    pl.rivals = Rivals(count=1, radius=0.3)
    log.clear()
    pl.plan_batch(np.zeros((2, 7)), waypoints=WP)
    names = [c[0] for c in log]
    assert names.index("f1p_stmpc_qp_set_walls") < names.index("f1p_stmpc_qp_plan_batch") and "f1p_stmpc_set_obstacles_dev" in names
    pl.rivals = None
    # the single-vehicle call
    pl.config.QP_AVOID = False
    log.clear()
    try:
        pl.plan(np.array([0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0]), waypoints=WP)
    except RuntimeError:
        pass                                                     # (whatever the stub's zeroed outputs make of the status)
    names = [c[0] for c in log]
    assert names.index("f1p_stmpc_qp_set_walls") < names.index("f1p_stmpc_qp_plan_batch")


def test_runtime_module_functions_on_the_stub():
    from f1tenth_planning_amd.runtime import stmpc_qp_set_walls, stmpc_qp_walls
    ctx = _stub()
    cfg = _abi.stmpc_cfg(horizon=3)
    out = stmpc_qp_walls(ctx, np.zeros((2, 7)), np.zeros((2, 7, 4)), None, cfg, want_planes=True, want_avoid_duals=True, want_duals=True)
    assert out["planes"].shape == (2, 3, 2, 4) and out["avoid_duals"].shape == (2, 7) and out["eps"].shape == (2,) and out["duals"].shape == (2, 28)
    name, args = ctx.lib.log[-1]
    assert name == "f1p_stmpc_qp_walls_batch" and len(args) == len(_abi.PROTOTYPES[name][1]) == 23
    assert args[8] is None and args[9] == ["i", 0] and args[10] is None and args[11] is None               # obs, M, avoid, walls
    stmpc_qp_walls(ctx, np.zeros((2, 7)), np.zeros((2, 7, 4)), np.zeros((2, 3, 5)), cfg, avoid=_abi.kmpc_qp_avoid(), walls=_abi.kmpc_qp_walls(n_samples=7))
    args = ctx.lib.log[-1][1]
    assert args[8:12] == ["ptr", ["i", 3], "byref:KmpcQpAvoid", "byref:KmpcQpWalls"]
    with pytest.raises(ValueError, match="obstacles must be"):
        stmpc_qp_walls(ctx, np.zeros((2, 7)), np.zeros((2, 7, 4)), np.zeros((3, 1, 5)), cfg)
    stmpc_qp_set_walls(ctx, None)
    assert ctx.lib.log[-1] == ["f1p_stmpc_qp_set_walls", ["ptr", None]]


# ---- 3. the header ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_new_names():
    """include/f1p.h declares the three entry points (tests/test_abi.py then demands them of the library), with f1p_kmpc_qp_walls reused"""
    hdr = open(os.path.join(ROOT, "include", "f1p.h")).read()
    for name in ("f1p_stmpc_qp_walls_batch", "f1p_stmpc_qp_walls_dev", "f1p_stmpc_qp_set_walls"):
        m = re.search(r"^int " + name + r"\(f1p_ctx\* ctx,[^;]*;", hdr, re.M)
        assert m and "const f1p_kmpc_qp_walls* walls" in m.group(0), name
        assert name in _abi.PROTOTYPES and hasattr(_abi.load_library(), name)
    assert len(_abi.PROTOTYPES["f1p_stmpc_qp_walls_batch"][1]) == len(_abi.PROTOTYPES["f1p_stmpc_qp_avoid_batch"][1]) + 1
