"""Wall rows of the kinematic QP on the host: the yardstick's march against a brute-force scan of the hand-made grid; the
yardstick certifies its own optima on the GPU tests' scenes, which hold the families they claim and no edge-sensitive ego; mpc_config.QP_WALLS'
checks raise before the library is reached and its switch reaches f1p_kmpc_qp_set_walls (on the stub library of tools/record_runtime_calls.py);
n_samples from reach and resolution; the f1p_kmpc_qp_walls layout.  No GPU."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kmpc_qp_ref as Q
import kmpc_qp_walls_ref as W
import kmpc_qp_walls_scenes as SC
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._planner import qp_wall_samples
from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner
from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import mpc_config as dyn_config
from f1tenth_planning_amd.control.kinematic_mpc import kinematic_mpc as KM
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the march ----------------------------------------------------------------------------------------------------------------------
def test_march_agrees_with_a_brute_force_scan():
    """random origins in and around the image, random and axis-aligned directions, every reach up to 64 samples"""
    grid = SC.grid_of()
    rng = np.random.default_rng(3)
    hits = set()
    for i in range(600):
        px = SC.ORIGIN[0] + rng.uniform(-1.0, SC.GW * SC.RES + 1.0)
        py = SC.ORIGIN[1] + rng.uniform(-1.0, SC.GH * SC.RES + 1.0)
        psi = [rng.uniform(-math.pi, math.pi), 0.0, math.pi / 2, math.pi, -math.pi / 2][i % 5 if i % 10 < 5 else 0]
        n = int(rng.integers(1, 65))
        lx, ly = -math.sin(psi), math.cos(psi)
        k, _ = W.march(grid, px, py, lx, ly, n)
        assert k == W.brute_first_hit(grid, px, py, lx, ly, n), (px, py, psi, n)
        hits.add(0 if k == 0 else 1 if k == 1 else 2)
    assert hits == {0, 1, 2}
    assert W.march(grid, math.nan, 1.0, 0.0, 1.0, 5)[0] == 1 and W.march(grid, 1.0, math.inf, 0.0, 1.0, 5)[0] == 1     # not finite: occupied


def test_cell_rule_and_image_order():
    """row 0 of the image is the TOP row; a cell is floor((p - origin) * (1 / res)); outside the image: occupied"""
    grid = SC.grid_of()
    assert not W.occupied(grid, SC.wx(4) + 0.01, SC.wy(24) + 0.01) and W.occupied(grid, SC.wx(4) - 0.01, SC.wy(24) + 0.01)
    assert W.occupied(grid, SC.wx(4) + 0.01, SC.wy(24) - 0.01) and not W.occupied(grid, SC.wx(30), SC.wy(43) + 0.05)
    assert not W.occupied(grid, SC.wx(96) - 0.01, SC.wy(0) + 0.01) and W.occupied(grid, SC.wx(96) + 0.01, SC.wy(0) + 0.01)
    assert W.occupied(grid, SC.wx(70), SC.wy(0) - 0.01) and W.occupied(grid, SC.wx(70), SC.wy(64) + 0.01)
    img = SC.grid_image()
    assert img.shape == (SC.GH, SC.GW) and img[SC.GH - 1 - 30, 10] == 255 and img[0, 70] == 255 and img[0, 10] == 0


def test_selection_among_discs_and_walls():
    """the two smallest clearances of {discs, left wall, right wall}, ties to the lower slot: discs before walls, left before right"""
    p = Q.default_params(2)
    grid = SC.grid_of()
    x0 = np.array([SC.wx(10), SC.wy(30), 1.0, 0.0])            # the corridor's centre line, heading exactly +x: both walls 0.6 m away
    ref = np.zeros((4, 3))
    oa = od = np.zeros(2)
    d = Q.qp_data(x0, ref, oa, od, p)
    c = Q.condense(d, 2)
    pl, _, _ = W.planes(d, c, None, grid, p, 20)
    assert pl[:, :, 3].tolist() == [[16.0, 17.0], [16.0, 17.0]]                      # a tie: left first
    assert pl[0, 0, :2].tolist() == [0.0, -1.0] and pl[0, 1, :2].tolist() == [-0.0, 1.0]
    path = d["path"]
    clear = 11 * 0.05                                            # k* = 12: the sample at 0.60 m is the first in the wall's cell
    assert W.march(grid, path[0, 1], path[1, 1], 0.0, 1.0, 20)[0] == 12
    obs = np.array([[path[0, 1], path[1, 1] + clear + 0.3, 0.0, 0.0, 0.3],        # a disc with the walls' clearance: before both
                    [path[0, 1], path[1, 1] - 2.0, 0.0, 0.0, 0.3]])
    pl, _, _ = W.planes(d, c, obs, grid, p, 20)
    assert pl[0, :, 3].tolist() == [0.0, 16.0]
    pl, _, _ = W.planes(d, c, obs, grid, p, 11)                  # the walls out of reach: the discs, whatever their distance
    assert pl[0, :, 3].tolist() == [0.0, 1.0]
    pl, _, _ = W.planes(d, c, None, grid, p, 11)
    assert (pl[:, :, 3] == -1).all() and (pl[:, :, :3] == 0).all()


# ---- 2. the scenes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", SC.SHAPES)
def test_scenes_certify_and_hold_their_families(T, M):
    """a condition on the scenes, checked here so that the GPU test's skips cannot hide a failure: the yardstick fails to certify at most 5 %
    of the egos, and at most 2 % are edge-sensitive (expected: none).  T = 31: the recorded points (golden g23) on the problems rebuilt here."""
    sols = SC.solutions(T, M)
    SC.assert_families(T, M, sols)
    feas = [s for s in sols if s is not None]
    fam = SC.scene(T, M)[5]
    assert len(feas) == SC.E - len(fam["v0_out"]) - len(fam["nan_state"]) == 54
    assert sum(not W.cert_ok(s["cert"]) for s in feas) <= 0.05 * SC.E
    assert sum(s["edge"] for s in feas) <= 0.02 * SC.E
    assert sum(s["edge"] for s in feas) == 0
    assert sum((s["avoid_lam"][:-1] > 1e-6).any() for s in feas) >= 5            # the rows bind somewhere
    assert sum(s["eps"] > 1e-3 for s in feas) >= 2 and sum(abs(s["eps"]) <= 1e-9 for s in feas) >= 5


def test_no_candidate_is_the_plain_qp():
    x0, ref, oa, od, obs, fam = SC.scene(8, 0)
    p = Q.default_params(8)
    for e in fam["no_wall"]:
        s = SC.solutions(8, 0)[e]
        s0 = Q.solve_case(x0[e], ref[e], oa[e], od[e], p)
        assert len(s["build"]["rows"]) == 0 and abs(s["eps"]) <= 1e-12 and np.abs(s["u"] - s0["u"]).max() <= 1e-9


# ---- 3. the class's checks, before the library is reached ------------------------------------------------------------------------------
def _stub():
    spec = importlib.util.spec_from_file_location("record_runtime_calls", os.path.join(ROOT, "tools", "record_runtime_calls.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.stub_context()


WP = np.zeros((4, 10))


def test_config_defaults_and_repr():
    c = mpc_config()
    assert (c.QP_WALLS, c.QP_WALL_REACH, c.QP_WALL_MARGIN) == (False, 1.5, 0.0)
    assert "QP_WALL" not in repr(c)
    assert dyn_config().QP_WALLS is False and "QP_WALLS" not in repr(dyn_config())


def test_qp_walls_needs_the_qp_solver_and_a_map():
    with pytest.raises(ValueError, match="QP_WALLS"):
        KMPCPlanner(config=mpc_config(QP_WALLS=True))
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS=True))
    with pytest.raises(ValueError, match="QP_WALLS needs an occupancy grid"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=WP)
    with pytest.raises(ValueError, match="QP_WALLS needs an occupancy grid"):
        pl.plan(np.zeros(7), waypoints=WP)
    assert pl._ctx is None
    with pytest.raises(ValueError) as ei:
        STMPCPlanner(config=dyn_config(QP_WALLS=True))
    assert str(ei.value) == "QP_WALLS: KMPCPlanner only"
    with pytest.raises(ValueError) as ei:
        STMPCPlanner(config=dyn_config(SOLVER="qp", QP_WALLS=True))
    assert str(ei.value) == "QP_WALLS: KMPCPlanner only"


@pytest.mark.parametrize("field,value", [("QP_WALL_REACH", 0.0), ("QP_WALL_REACH", -1.0), ("QP_WALL_REACH", math.nan), ("QP_WALL_REACH", math.inf),
                                         ("QP_WALL_MARGIN", math.nan), ("QP_WALL_MARGIN", math.inf), ("TK", 32)])
def test_bad_wall_numbers_raise_before_the_library(field, value):
    with pytest.raises(ValueError):
        KMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS=True, **{field: value}))
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS=True))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN)
    setattr(pl.config, field, value)
    pl._ctx.lib.log.clear()
    with pytest.raises(ValueError):
        pl.plan_batch(np.zeros((1, 4)), waypoints=WP)
    assert pl._ctx.lib.log == []
    KMPCPlanner(config=mpc_config(SOLVER="qp", **{field: value} if field != "TK" else {}))      # off: the numbers are not read


def test_reach_past_256_samples_names_reach_and_resolution():
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS=True, QP_WALL_REACH=12.81))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN)
    pl._ctx.lib.log.clear()
    with pytest.raises(ValueError, match=r"12\.81.*0\.1"):
        pl.plan_batch(np.zeros((1, 4)), waypoints=WP)
    assert pl._ctx.lib.log == []
    pl.config.QP_WALL_REACH = 12.8
    pl.plan_batch(np.zeros((1, 4)), waypoints=WP)                # 256 samples: the most


def test_samples_from_reach_and_resolution():
    assert qp_wall_samples(1.5, 0.1) == 30 and qp_wall_samples(1.5, 0.058) == math.ceil(1.5 / 0.029) == 52
    assert qp_wall_samples(2.4, 0.1) == 48 and qp_wall_samples(2.41, 0.1) == 49 and qp_wall_samples(0.01, 0.1) == 1
    assert qp_wall_samples(12.8, 0.1) == 256
    with pytest.raises(ValueError):
        qp_wall_samples(12.85, 0.1)


def test_switch_reaches_the_library(monkeypatch):
    """plan_batch with QP_WALLS: f1p_kmpc_qp_set_walls(on, n_samples, margin) before the plan; off again after a plan without it; QP_AVOID's
    switch beside it untouched"""
    seen = []
    real = KM.kmpc_qp_set_walls
    monkeypatch.setattr(KM, "kmpc_qp_set_walls", lambda ctx, w: (seen.append(None if w is None else (w.on, w.n_samples, w.margin)), real(ctx, w))[1])
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_WALLS=True, QP_WALL_REACH=1.0, QP_WALL_MARGIN=0.05))
    pl._ctx = _stub()
    pl.set_map(SC.grid_image(), SC.RES, SC.ORIGIN, inflate=0.2)
    log = pl._ctx.lib.log
    assert [c[0] for c in log] == ["f1p_set_grid", "f1p_inflate_grid"]
    log.clear()
    pl.plan_batch(np.zeros((2, 4)), waypoints=WP)
    names = [c[0] for c in log]
    assert seen == [(1, 20, 0.05)] and "f1p_kmpc_qp_set_avoid" not in names
    assert names.index("f1p_kmpc_qp_set_walls") < names.index("f1p_kmpc_qp_plan_batch")
    assert ["f1p_kmpc_qp_set_walls", ["ptr", "byref:KmpcQpWalls"]] in log
    pl.config.QP_WALLS = False
    log.clear()
    pl.plan_batch(np.zeros((2, 4)), waypoints=WP)
    assert seen[-1] is None and ["f1p_kmpc_qp_set_walls", ["ptr", None]] in log
    log.clear()
    pl.plan_batch(np.zeros((2, 4)), waypoints=WP)                # off after a plan with it off: nothing to switch
    assert "f1p_kmpc_qp_set_walls" not in [c[0] for c in log]
    # tracks and obstacles with it
    pl.config.QP_WALLS = pl.config.QP_AVOID = True
    pl.obstacles = np.zeros((2, 1, 5))
    log.clear()
    pl.plan_batch(np.zeros((2, 4)), tracks=[WP, WP], track_ids=[0, 1])
    names = [c[0] for c in log]
    assert {"f1p_kmpc_qp_set_walls", "f1p_kmpc_qp_set_avoid", "f1p_kmpc_set_obstacles", "f1p_kmpc_qp_dev"} <= set(names)
    assert names.index("f1p_kmpc_qp_set_walls") < names.index("f1p_kmpc_qp_dev")


def test_runtime_module_functions_on_the_stub():
    from f1tenth_planning_amd.runtime import kmpc_qp_set_walls, kmpc_qp_walls
    ctx = _stub()
    cfg = _abi.kmpc_cfg(horizon=3)
    out = kmpc_qp_walls(ctx, np.zeros((2, 4)), np.zeros((2, 4, 4)), None, cfg, want_planes=True, want_avoid_duals=True)
    assert out["planes"].shape == (2, 3, 2, 4) and out["avoid_duals"].shape == (2, 7) and out["eps"].shape == (2,)
    name, args = ctx.lib.log[-1]
    assert name == "f1p_kmpc_qp_walls_batch" and len(args) == len(_abi.PROTOTYPES[name][1]) == 23
    assert args[8] is None and args[9] == ["i", 0] and args[10] is None and args[11] is None               # obs, M, avoid, walls
    kmpc_qp_walls(ctx, np.zeros((2, 4)), np.zeros((2, 4, 4)), np.zeros((2, 3, 5)), cfg, avoid=_abi.kmpc_qp_avoid(), walls=_abi.kmpc_qp_walls(n_samples=7))
    args = ctx.lib.log[-1][1]
    assert args[8:12] == ["ptr", ["i", 3], "byref:KmpcQpAvoid", "byref:KmpcQpWalls"]
    with pytest.raises(ValueError, match="obstacles must be"):
        kmpc_qp_walls(ctx, np.zeros((2, 4)), np.zeros((2, 4, 4)), np.zeros((3, 1, 5)), cfg)
    kmpc_qp_set_walls(ctx, None)
    assert ctx.lib.log[-1] == ["f1p_kmpc_qp_set_walls", ["ptr", None]]


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------------------------
def test_qp_walls_layout_matches_gcc():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f1p.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n", ' \
          'sizeof(f1p_kmpc_qp_walls), offsetof(f1p_kmpc_qp_walls, on), offsetof(f1p_kmpc_qp_walls, n_samples), ' \
          'offsetof(f1p_kmpc_qp_walls, margin), F1P_KMPC_QP_WALL_MAX_SAMPLES);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.c"), "-o", os.path.join(d, "l")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    S = _abi.KmpcQpWalls
    assert got == [C.sizeof(S), S.on.offset, S.n_samples.offset, S.margin.offset, _abi.KMPC_QP_WALL_MAX_SAMPLES] == [16, 0, 4, 8, 256]
    w = _abi.kmpc_qp_walls()
    assert (w.on, w.n_samples, w.margin) == (1, 48, 0.0)


def test_qp_walls_default_and_symbols():
    lib = _abi.load_library()
    w = _abi.KmpcQpWalls(on=7, n_samples=7, margin=7.0)
    lib.f1p_kmpc_qp_walls_default(C.byref(w))
    assert (w.on, w.n_samples, w.margin) == (0, 48, 0.0)
    for name in ("f1p_kmpc_qp_walls_batch", "f1p_kmpc_qp_walls_dev", "f1p_kmpc_qp_set_walls"):
        assert hasattr(lib, name)
