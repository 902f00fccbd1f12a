"""Moving-disc avoidance rows of the kinematic QP on the host: the yardstick (tests/kmpc_qp_avoid_ref.py) certifies itself on the
two levine scenes and avoids the parked disc the plain QP drives through; the class's switches raise before a device is opened; the
f1p_kmpc_qp_avoid layout; the GPU tests' scenes hold the families they claim.  No GPU."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kmpc_qp_avoid_ref as A
import kmpc_qp_avoid_scenes as SC
import kmpc_qp_ref as Q
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd._rivals import SINGLE_EGO, Rivals
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the reference certifies itself -------------------------------------------------------------------------------------------------
def test_parked_scene_reference_certifies_and_avoids(tracks):
    """every one of the 400 steps: the exact solution passes _cert_ok's bars; the ego keeps >= 0.30 m from the disc's centre where the plain
    QP passes within 0.10 m (measured: 0.348 and 0.040, rows active on the 91 steps 94..184, eps <= 0.071)"""
    plain = SC.run_scene(tracks["levine"], "parked", 400, avoid=False)
    assert plain["dmin"] < 0.10, plain["dmin"]
    r = SC.run_scene(tracks["levine"], "parked", 400)
    assert r["uncertified"] == [], r["uncertified"]
    assert r["degenerate"] == []
    assert r["dmin"] >= 0.30, r["dmin"]
    assert len(r["active"]) >= 50, len(r["active"])
    assert 0.0 < r["eps_max"] < 0.2


def test_moving_scene_reference_certifies(tracks):
    """a disc that starts on waypoint 60 and moves at 1.5 m/s along the course heading there, 500 steps"""
    r = SC.run_scene(tracks["levine"], "moving", 500)
    assert r["uncertified"] == [], r["uncertified"]
    assert r["degenerate"] == []
    assert len(r["active"]) >= 1 and r["dmin"] >= 0.45, (len(r["active"]), r["dmin"])      # the rows bind and the ego stays outside r = 0.45


def test_shifted_slack_is_the_same_problem():
    """solve()'s eps shift: the returned point satisfies build()'s unshifted rows, and an ego without a live slot has the plain QP's u"""
    x0, ref, oa, od, obs, _ = SC.exact_scene(8, 4)
    p = Q.default_params(8)
    e = SC.FAMILY_EGO["no_live"]
    s = A.solve(x0[e], ref[e], oa[e], od[e], obs[e], p)
    s0 = Q.solve_case(x0[e], ref[e], oa[e], od[e], p)
    assert len(s["build"]["rows"]) == 0 and s["eps"] == pytest.approx(0.0, abs=1e-12)
    assert np.abs(s["u"] - s0["u"]).max() <= 1e-9
    e = SC.FAMILY_EGO["inside"]
    s = A.solve(x0[e], ref[e], oa[e], od[e], obs[e], p)
    b = s["build"]
    assert (b["G"] @ s["w"] <= b["h"] + 1e-9).all() and A.cert_ok(s["cert"])


@pytest.mark.parametrize("T,M", SC.SHAPES)
def test_exact_scenes_hold_their_families(T, M):
    """what tests/test_gpu_kmpc_qp_avoid.py asserts from the reference's output; at most 5 % of the egos may fail to certify (the GPU test
    skips the distance check there).  The recorded points (golden g20) are certified on the problems rebuilt here."""
    x0, ref, oa, od, obs, fam = SC.exact_scene(T, M)
    sols = SC.exact_solutions(T, M)
    SC.assert_families(T, M, obs, sols, fam)
    feas = [s for s in sols if s is not None]
    assert len(feas) == SC.E - len(fam["nan_live"]) - len(fam["v0_out"])
    assert sum(not A.cert_ok(s["cert"]) for s in feas) <= 0.05 * len(sols)


@pytest.mark.parametrize("T,M", [(2, 1), (2, 16), (8, 4)])
def test_golden_record_is_the_helpers_output(T, M):
    """the short horizons solved again here (a T = 31 batch takes a minute: tools/gen_golden_kmpc_qp_avoid.py)"""
    for rec, now in zip(SC.exact_solutions(T, M), SC.solve_scene(T, M)):
        assert (rec is None) == (now is None)
        if rec is not None:
            assert np.abs(rec["w"] - now["w"]).max() <= 1e-10 and np.abs(rec["lam"] - now["lam"]).max() <= 1e-7 * (1.0 + np.abs(now["lam"]).max())
            assert rec["degenerate"] == now["degenerate"]


# ---- 2. host rejections, before a device is opened -------------------------------------------------------------------------------------
def test_qp_avoid_needs_the_qp_solver():
    with pytest.raises(ValueError, match="QP_AVOID"):
        KMPCPlanner(config=mpc_config(QP_AVOID=True))
    c = mpc_config()
    assert (c.QP_AVOID, c.QP_AVOID_MARGIN, c.QP_AVOID_RHO, c.QP_AVOID_LIN) == (False, 0.0, 1e4, 10.0)
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_AVOID=True))
    assert pl._ctx is None


@pytest.mark.parametrize("field,value", [("QP_AVOID_RHO", 0.0), ("QP_AVOID_RHO", -1.0), ("QP_AVOID_RHO", math.nan), ("QP_AVOID_RHO", math.inf),
                                         ("QP_AVOID_LIN", -1e-3), ("QP_AVOID_LIN", math.nan), ("QP_AVOID_MARGIN", math.nan),
                                         ("QP_AVOID_MARGIN", math.inf), ("TK", 32)])
def test_bad_avoid_numbers_raise_before_the_gpu(field, value):
    with pytest.raises(ValueError):
        KMPCPlanner(config=mpc_config(SOLVER="qp", QP_AVOID=True, **{field: value}))
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_AVOID=True))
    setattr(pl.config, field, value)
    pl.obstacles = np.zeros((1, 1, 5))
    with pytest.raises(ValueError):
        pl.plan_batch(np.zeros((1, 4)), waypoints=np.zeros((4, 10)))
    assert pl._ctx is None
    KMPCPlanner(config=mpc_config(SOLVER="qp", **{field: value} if field != "TK" else {}))      # off: the numbers are not read


def test_unchanged_rejections_with_qp_avoid_off():
    wp = np.zeros((4, 10))
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp"))
    pl.obstacles = np.zeros((2, 1, 5))
    with pytest.raises(ValueError, match="obstacles are tested on the shooting solver's rollouts; SOLVER='qp' takes none"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    pl.obstacles = np.zeros((1, 5))
    with pytest.raises(ValueError, match="obstacles are tested on the shooting solver's rollouts; SOLVER='qp' takes none"):
        pl.plan(np.zeros(7), waypoints=wp)
    pl.rivals = Rivals(count=2, radius=0.45)
    with pytest.raises(ValueError, match="rivals are tested on the shooting solver's rollouts; SOLVER='qp' takes none"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    with pytest.raises(ValueError, match="COLLISION tests the shooting solver's rollouts"):
        KMPCPlanner(config=mpc_config(SOLVER="qp", COLLISION=True))
    assert pl._ctx is None


def test_qp_avoid_on_keeps_the_shape_and_single_ego_checks():
    wp = np.zeros((4, 10))
    pl = KMPCPlanner(config=mpc_config(SOLVER="qp", QP_AVOID=True))
    pl.obstacles = np.zeros((2, 17, 5))
    with pytest.raises(ValueError, match="at most 16 obstacles"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    pl.obstacles = np.zeros((3, 1, 5))
    with pytest.raises(ValueError, match="obstacles must be"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    pl.rivals = Rivals(count=2, radius=0.45)
    with pytest.raises(ValueError, match="plan_batch"):
        pl.plan(np.zeros(7), waypoints=wp)
    with pytest.raises(ValueError) as ei:
        pl.plan(np.zeros(7), waypoints=wp)
    assert str(ei.value) == SINGLE_EGO
    pl.obstacles = np.zeros((2, 1, 5))
    with pytest.raises(ValueError, match="planner.rivals and planner.obstacles in one call"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    pl.rivals = Rivals(count=17, radius=0.45)
    with pytest.raises(ValueError, match="Rivals.count"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    pl.rivals = None
    pl.config.QP_AVOID = False
    pl.config.SOLVER = "shooting"
    pl.config.QP_AVOID = True
    with pytest.raises(ValueError, match="QP_AVOID"):
        pl.plan_batch(np.zeros((2, 4)), waypoints=wp)
    assert pl._ctx is None


# ---- 3. ABI ----------------------------------------------------------------------------------------------------------------------------
def test_qp_avoid_layout_matches_gcc():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f1p.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", ' \
          'sizeof(f1p_kmpc_qp_avoid), offsetof(f1p_kmpc_qp_avoid, on), offsetof(f1p_kmpc_qp_avoid, pad), offsetof(f1p_kmpc_qp_avoid, margin), ' \
          'offsetof(f1p_kmpc_qp_avoid, rho), offsetof(f1p_kmpc_qp_avoid, lin));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.c"), "-o", os.path.join(d, "l")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    S = _abi.KmpcQpAvoid
    assert got == [C.sizeof(S), S.on.offset, S.pad.offset, S.margin.offset, S.rho.offset, S.lin.offset] == [32, 0, 4, 8, 16, 24]
    a = _abi.kmpc_qp_avoid()
    assert (a.on, a.margin, a.rho, a.lin) == (1, 0.0, 1e4, 10.0)


def test_qp_avoid_default_and_symbols():
    lib = _abi.load_library()
    a = _abi.KmpcQpAvoid(on=7, pad=7, margin=7.0, rho=7.0, lin=7.0)
    lib.f1p_kmpc_qp_avoid_default(C.byref(a))
    assert (a.on, a.pad, a.margin, a.rho, a.lin) == (0, 0, 0.0, 1e4, 10.0)
    for name in ("f1p_kmpc_qp_avoid_batch", "f1p_kmpc_qp_avoid_dev", "f1p_kmpc_qp_set_avoid"):
        assert hasattr(lib, name)
