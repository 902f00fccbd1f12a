"""Moving-disc avoidance rows of the dynamic QP on the host: the GPU tests' scenes hold the families they claim and their
recorded optima (golden g22) certify on the problems rebuilt here; the yardstick's shifted slack is the same problem; the ABI; the class's
switches raise before the library is reached (on the stub library of tools/record_runtime_calls.py).  No GPU."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import stmpc_qp_avoid_ref as A
import stmpc_qp_avoid_scenes as SC
import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._rivals import SINGLE_EGO, Rivals
from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. scenes, record, yardstick ---------------------------------------------------------------------------------------------------------
def test_horizons_straddle_the_opt_in_boundary_and_end_at_the_cap():
    a, b = SC.HORIZONS[2], SC.HORIZONS[3]
    assert b == a + 1 and SC.lds_bytes(a) <= 64 * 1024 < SC.lds_bytes(b)
    assert SC.HORIZONS[0] == 2 and SC.HORIZONS[-1] == SC.CAP == 40
    assert SC.lds_bytes(SC.CAP) <= 160 * 1024 and SC.lds_bytes(1) == -1
    assert {f for e in range(16) for f in [SC.family(e)[0]]} == set(SC.FAMILIES)        # the 16 egos of the cap's batch cover every family


@pytest.mark.parametrize("T,M,margin", SC.SHAPES)
def test_exact_scenes_hold_their_families(T, M, margin):
    """what tests/test_gpu_stmpc_qp_avoid.py asserts from the yardstick's output; at most 1 ego in 16 may fail to certify (the GPU test skips
    only the distance check there).  The recorded points (golden g22) are certified on the problems rebuilt here."""
    x0, ref, oa, odv, obs, fam = SC.exact_scene(T, M)
    assert (x0[np.setdiff1d(np.arange(len(x0)), fam["v0_out"]), 3] > 2.0).all() and np.abs(oa).max() > 0 and np.abs(odv).max() > 0
    sols = SC.exact_solutions(T, M, margin)
    SC.assert_families(T, M, margin, obs, sols, fam)
    feas = [s for s in sols if s is not None]
    assert len(feas) == SC.n_egos(T) - len(fam["nan_live"]) - len(fam["v0_out"])
    assert 16 * SC.uncertified(sols) <= len(sols)


@pytest.mark.parametrize("T,M,margin", [(2, 1, 0.0), (2, 16, 0.0), (10, 4, 0.0), (10, 4, 0.015)])
def test_golden_record_is_the_helpers_output(T, M, margin):
    """the short horizons solved again here (the long ones take minutes: tools/gen_golden_stmpc_qp_avoid.py)"""
    for rec, now in zip(SC.exact_solutions(T, M, margin), SC.solve_scene(T, M, margin)):
        assert (rec is None) == (now is None)
        if rec is not None:
            assert np.abs(rec["w"] - now["w"]).max() <= 1e-10 and np.abs(rec["lam"] - now["lam"]).max() <= 1e-7 * (1.0 + np.abs(now["lam"]).max())
            assert rec["degenerate"] == now["degenerate"]
    oa, odv = SC.compute_prev(T)
    assert np.abs(oa - SC.exact_scene(T, M)[2]).max() <= 1e-9 and np.abs(odv - SC.exact_scene(T, M)[3]).max() <= 1e-9


def test_shifted_slack_is_the_same_problem():
    """solve()'s eps shift and scale: the returned point satisfies build()'s unshifted rows with the unscaled multipliers, and an ego without
    a live slot has the plain QP's u"""
    T, M = 10, 4
    x0, ref, oa, odv, obs, fam = SC.exact_scene(T, M)
    p = SQ.default_params(T)
    e = fam["no_live"][0]
    s = A.solve(x0[e], ref[e], oa[e], odv[e], obs[e], p)
    s0 = SQ.solve_case(x0[e], ref[e], oa[e], odv[e], p)
    assert len(s["build"]["rows"]) == 0 and s["eps"] == pytest.approx(0.0, abs=1e-12)
    assert np.abs(s["u"] - s0["u"]).max() <= 1e-9 and abs(s["obj"] - s0["obj"]) <= 1e-9 * (1.0 + abs(s0["obj"]))
    e = fam["inside"][0]
    s = A.solve(x0[e], ref[e], oa[e], odv[e], obs[e], p)
    b = s["build"]
    assert (b["G"] @ s["w"] <= b["h"] + 1e-9).all() and s["certified"] and s["eps"] > 5e-3
    cs, D, w0 = A.scaled(b)
    ws = (s["w"] - w0) / D
    assert (cs["G"] @ np.zeros(len(ws)) <= cs["h"]).all()                      # the shifted origin is feasible
    f = lambda H, g, w: 0.5 * w @ H @ w + g @ w                                 # noqa: E731
    other = ws + np.random.default_rng(0).normal(0.0, 0.1, len(ws))
    assert (f(cs["H"], cs["g"], other) - f(cs["H"], cs["g"], ws)) == pytest.approx(
        f(b["H"], b["g"], D * other + w0) - f(b["H"], b["g"], s["w"]), rel=1e-9, abs=1e-9)


# ---- 2. ABI --------------------------------------------------------------------------------------------------------------------------------
def test_symbols_prototypes_and_the_cap():
    """fails on the parent: the symbols do not exist"""
    lib = _abi.load_library()
    for name in ("f1p_stmpc_qp_avoid_batch", "f1p_stmpc_qp_avoid_dev", "f1p_stmpc_qp_set_avoid", "f1p_stmpc_qp_avoid_lds_bytes"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
    assert len(_abi.PROTOTYPES["f1p_stmpc_qp_avoid_batch"][1]) == len(_abi.PROTOTYPES["f1p_stmpc_qp_batch"][1]) + 6
    assert _abi.PROTOTYPES["f1p_stmpc_qp_avoid_batch"][1] == _abi.PROTOTYPES["f1p_stmpc_qp_avoid_dev"][1]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f1p.h"\nint main(void){printf("%d %d %zu %zu\\n", F1P_STMPC_QP_AVOID_MAX_T, ' \
          'F1P_STMPC_QP_MAX_T, sizeof(f1p_kmpc_qp_avoid), offsetof(f1p_kmpc_qp_avoid, lin));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.c"), "-o", os.path.join(d, "l")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    assert got == [_abi.STMPC_QP_AVOID_MAX_T, 44, C.sizeof(_abi.KmpcQpAvoid), _abi.KmpcQpAvoid.lin.offset] == [40, 44, 32, 24]
    # the cap is the layout's: the longest horizon that leaves a KiB of the CU's 160 KiB
    assert lib.f1p_stmpc_qp_avoid_lds_bytes(40) <= 160 * 1024 - 1024 < lib.f1p_stmpc_qp_avoid_lds_bytes(41)
    from f1tenth_planning_amd import runtime
    assert callable(runtime.stmpc_qp_avoid) and callable(runtime.stmpc_qp_set_avoid)
    assert not hasattr(runtime.Context, "stmpc_qp_avoid") and not hasattr(runtime.Context, "stmpc_qp_set_avoid")


# ---- 3. the class, on the stub library: rejections before the library is reached --------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("record_runtime_calls", os.path.join(ROOT, "tools", "record_runtime_calls.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


WP = np.random.default_rng(2).normal(size=(6, 5))
COURSE = [WP[:, 0], WP[:, 1], WP[:, 3], WP[:, 2]]


def _planner(tool, **cfg):
    p = STMPCPlanner(config=mpc_config(**cfg))
    p._ctx = tool.stub_context()
    return p


def _rejected(p, call, match):
    with pytest.raises(ValueError, match=match):
        call()
    assert p._ctx.lib.log == [], "the library was reached before the rejection"


def test_qp_avoid_needs_the_qp_solver(tool):
    with pytest.raises(ValueError, match="QP_AVOID adds avoidance rows to the QP"):
        STMPCPlanner(config=mpc_config(QP_AVOID=True))
    c = mpc_config()
    assert (c.QP_AVOID, c.QP_AVOID_MARGIN, c.QP_AVOID_RHO, c.QP_AVOID_LIN) == (False, 0.0, 1e4, 10.0)
    assert "QP_AVOID" not in repr(c)
    p = _planner(tool, SOLVER="qp", QP_AVOID=True)
    p.config.SOLVER = "shooting"
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "QP_AVOID")


@pytest.mark.parametrize("field,value", [("QP_AVOID_RHO", 0.0), ("QP_AVOID_RHO", -1.0), ("QP_AVOID_RHO", math.nan), ("QP_AVOID_RHO", math.inf),
                                         ("QP_AVOID_LIN", -1e-3), ("QP_AVOID_LIN", math.nan), ("QP_AVOID_MARGIN", math.nan),
                                         ("QP_AVOID_MARGIN", math.inf), ("T", _abi.STMPC_QP_AVOID_MAX_T + 1), ("TK", 32)])
def test_bad_avoid_numbers_raise_before_the_gpu(tool, field, value):
    with pytest.raises(ValueError, match=field if field.startswith("QP") else f"QP_AVOID needs {field} <="):
        STMPCPlanner(config=mpc_config(SOLVER="qp", QP_AVOID=True, **{field: value}))
    p = _planner(tool, SOLVER="qp", QP_AVOID=True)
    setattr(p.config, field, value)
    p.obstacles = np.zeros((1, 1, 5))
    _rejected(p, lambda: p.plan_batch(np.zeros((1, 7)), waypoints=COURSE), "QP_AVOID")
    p.obstacles = np.zeros((1, 5))
    _rejected(p, lambda: p.plan(np.zeros(7), waypoints=COURSE), "QP_AVOID")
    if field not in ("T", "TK"):
        STMPCPlanner(config=mpc_config(SOLVER="qp", **{field: value}))           # off: the numbers are not read
    else:                                                                          # off: the plain caps (44, and TK <= T) are what they were
        STMPCPlanner(config=mpc_config(SOLVER="qp", T=41, TK=32))


def test_unchanged_rejections_with_qp_avoid_off(tool):
    p = _planner(tool, SOLVER="qp")
    p.obstacles = np.zeros((2, 1, 5))
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "obstacles are tested on the shooting solver's rollouts; SOLVER='qp' takes none")
    p.obstacles = np.zeros((1, 5))
    _rejected(p, lambda: p.plan(np.zeros(7), waypoints=COURSE), "obstacles are tested on the shooting solver's rollouts; SOLVER='qp' takes none")
    p.rivals = Rivals(count=2, radius=0.45)
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "rivals are tested on the shooting solver's rollouts; SOLVER='qp' takes none")
    p.rivals = None
    with pytest.raises(ValueError, match="COLLISION tests the shooting solver's rollouts"):
        STMPCPlanner(config=mpc_config(SOLVER="qp", COLLISION=True))
    with pytest.raises(ValueError, match="SOLVER='qp' needs TK <= T"):
        STMPCPlanner(config=mpc_config(SOLVER="qp", T=4, TK=8))
    q = _planner(tool)
    _rejected(q, lambda: q.plan_batch(np.zeros((2, 7)), tracks=[COURSE], track_ids=[0, 0]), "plan_batch with tracks needs SOLVER='qp'")
    # off, the QP plan makes the calls it made: no switch, no obstacles
    p.plan_batch(np.zeros((2, 7)), waypoints=COURSE)
    names = [c[0] for c in p._ctx.lib.log]
    assert "f1p_stmpc_qp_plan_batch" in names and not any("avoid" in n or "obstacles" in n for n in names), names


def test_qp_avoid_on_keeps_the_shape_and_single_ego_checks(tool):
    p = _planner(tool, SOLVER="qp", QP_AVOID=True)
    p.obstacles = np.zeros((2, 17, 5))
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "at most 16 obstacles")
    p.obstacles = np.zeros((3, 1, 5))
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "obstacles must be")
    p.rivals = Rivals(count=2, radius=0.45)
    with pytest.raises(ValueError) as ei:
        p.plan(np.zeros(7), waypoints=COURSE)
    assert str(ei.value) == SINGLE_EGO
    p.obstacles = np.zeros((2, 1, 5))
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "planner.rivals and planner.obstacles in one call")
    p.rivals = Rivals(count=17, radius=0.45)
    _rejected(p, lambda: p.plan_batch(np.zeros((2, 7)), waypoints=COURSE), "Rivals.count")


def test_accepted_calls_switch_then_set_obstacles_then_plan(tool):
    """QP_AVOID on: the switch, the discs in the caller's order, the plan -- with and without tracks; the attribute is taken; a later plan
    without discs clears them; QP_AVOID off again turns the switch off once"""
    p = _planner(tool, SOLVER="qp", QP_AVOID=True)
    p.obstacles = np.zeros((2, 3, 5))
    p.plan_batch(np.zeros((2, 7)), waypoints=COURSE)
    names = [c[0] for c in p._ctx.lib.log]
    assert p.obstacles is None
    assert [n for n in names if "avoid" in n or "obstacles" in n or "plan" in n] == \
        ["f1p_stmpc_qp_set_avoid", "f1p_stmpc_set_obstacles", "f1p_stmpc_qp_plan_batch"], names
    del p._ctx.lib.log[:]
    p.obstacles = np.zeros((2, 3, 5))
    p.plan_batch(np.zeros((2, 7)), tracks=[COURSE, COURSE], track_ids=[0, 1])
    names = [c[0] for c in p._ctx.lib.log]
    assert [n for n in names if "avoid" in n or "obstacles" in n or "plan" in n] == \
        ["f1p_stmpc_qp_set_avoid", "f1p_stmpc_set_obstacles", "f1p_stmpc_qp_plan_tracks_batch"], names
    del p._ctx.lib.log[:]
    p.plan_batch(np.zeros((2, 7)), waypoints=COURSE)                              # none this time: the held ones are cleared
    names = [c[0] for c in p._ctx.lib.log]
    assert "f1p_stmpc_set_obstacles" in names
    del p._ctx.lib.log[:]
    p.config.QP_AVOID = False
    p.plan_batch(np.zeros((2, 7)), waypoints=COURSE)
    p.plan_batch(np.zeros((2, 7)), waypoints=COURSE)
    names = [c[0] for c in p._ctx.lib.log]
    assert names.count("f1p_stmpc_qp_set_avoid") == 1 and names.count("f1p_stmpc_qp_plan_batch") == 2
