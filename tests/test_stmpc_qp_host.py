"""The linearised dynamic-MPC QP on the host: the yardstick (tests/stmpc_qp_ref.py) against the reference's own problem data (golden G17,
recorded from the reference's code by tools/gen_golden_stmpc_qp.py) for both of STMPCPlanner's branches, its exact solver against the
KKT certificate, the class's solver switch, and the C struct layouts.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kmpc_qp_ref as KQ
import stmpc_qp_ref as SQ
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.control.dynamic_mpc.dynamic_mpc import STMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g17_cases(golden):
    g = golden("g17_stmpc_qp.npz")

    def dense(p, m):
        A = np.zeros(tuple(g[p + m + "_shape"]))
        A[g[p + m + "_rows"], g[p + m + "_cols"]] = g[p + m + "_vals"]
        return A
    out = []
    for k in range(int(g["n_cases"])):
        p = f"c{k:02d}_"
        rec = {m: dense(p, m) for m in ("P", "Aeq", "G")}
        rec.update({v: g[p + v] for v in ("q", "beq", "h")})
        rec["r"] = float(g[p + "r"])
        out.append(dict(branch=str(g[p + "branch"]), T=int(g[p + "T"]), kind=str(g[p + "kind"]), track=str(g[p + "track"]), x0=g[p + "x0"],
                        ref=g[p + "ref"], oa=g[p + "oa"], od=g[p + "od"], warm=bool(g[p + "warm"]), rec=rec))
    return out


def helper_data(c):
    if c["branch"] == "dyn":
        return SQ.qp_data(c["x0"], c["ref"], c["oa"], c["od"], SQ.default_params(c["T"]))
    return KQ.qp_data(c["x0"], c["ref"], c["oa"], c["od"], SQ.kin_params(c["T"]))


def test_g17_covers_the_cases(golden):
    cases = g17_cases(golden)
    dyn = [c for c in cases if c["branch"] == "dyn"]
    kin = [c for c in cases if c["branch"] == "kin"]
    assert sum(c["T"] == 40 for c in dyn) >= 24 and sum(c["T"] == 10 for c in dyn) >= 16 and len(kin) >= 8
    kinds = {"zero", "warm", "vks", "fast", "steer_max", "sharp", "yawrate", "wrap"}
    for T in (40, 10):
        for track in ("levine", "spielberg"):
            assert {c["kind"] for c in dyn if c["T"] == T and c["track"] == track} == kinds, (T, track)
    assert any(2.05 <= c["x0"][3] <= 2.5 for c in dyn) and any(c["x0"][3] >= 5.8 for c in dyn)
    assert any(abs(c["x0"][2]) == 0.4189 for c in dyn)
    assert any(abs(c["x0"][5]) > 0.5 for c in dyn) and any(abs(c["x0"][4]) > np.pi for c in dyn)
    assert any(c["warm"] for c in dyn) and any(not c["warm"] for c in dyn)
    assert all(c["x0"][2] <= 2.0 for c in kin) and any(c["warm"] for c in kin) and any(not c["warm"] for c in kin)


def test_helper_qp_data_equals_the_references(golden):
    """pins the dense Jacobian, the previous acceleration in it, the unshifted warm start, the t = 0 objective term, the row order
    and the column-major ordering -- exactly"""
    for k, c in enumerate(g17_cases(golden)):
        d = helper_data(c)
        for m in ("P", "Aeq", "G", "q", "beq", "h"):
            a, b = c["rec"][m], d[m]
            assert a.shape == b.shape, (k, m)
            assert np.array_equal(a, b), (k, m, np.abs(a - b).max())
        assert c["rec"]["r"] == d["r"], k


def test_helper_exact_solutions_pass_the_certificate(golden):
    n_exact = 0
    for k, c in enumerate(g17_cases(golden)):
        if c["branch"] == "dyn":
            s = SQ.solve_case(c["x0"], c["ref"], c["oa"], c["od"], SQ.default_params(c["T"]))
            z = np.concatenate([s["x"].T.ravel(), s["u"].ravel()])
            rows = SQ.gpu_rows(c["T"])
        else:
            s = KQ.solve_case(c["x0"], c["ref"], c["oa"], c["od"], SQ.kin_params(c["T"]))
            z = np.concatenate([s["xk"].T.ravel(), s["u"].ravel()])
            rows = KQ.gpu_rows(c["T"])
        r = c["rec"]
        lam = np.zeros(len(r["h"]))
        lam[rows] = s["lam"]
        cert = SQ.certificate(r["P"], r["q"], r["Aeq"], r["beq"], r["G"], r["h"], z, lam)
        if s["degenerate"]:
            continue                      # the GPU test's certificate decides those
        n_exact += 1
        assert cert["primal"] <= 1e-9 and cert["dual"] >= -1e-10 and cert["comp"] <= 1e-7 and cert["stat"] <= 1e-8, (k, cert)
    assert n_exact >= 30


def test_default_solver_is_shooting():
    assert mpc_config().SOLVER == "shooting"
    assert mpc_config().QP_TOL == 1e-10 and mpc_config().QP_MAX_ITER == 50


def test_bad_solver_and_off_diagonal_weights_raise_before_the_gpu():
    c = mpc_config()
    c.SOLVER = "osqp"
    with pytest.raises(ValueError):
        STMPCPlanner(config=c)
    c = mpc_config(SOLVER="qp")
    c.Rd = np.array([[0.3, 0.01], [0.01, 0.01]])
    with pytest.raises(ValueError):
        STMPCPlanner(config=c)
    pl = STMPCPlanner(config=mpc_config(SOLVER="qp"))
    pl.config.Q = np.ones((7, 7))
    with pytest.raises(ValueError):
        pl.plan(np.array([0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0]), waypoints=np.zeros((4, 10)))
    with pytest.raises(ValueError):
        pl.plan_batch(np.zeros((1, 7)), waypoints=np.zeros((4, 10)))
    assert pl._ctx is None                                   # nothing touched the GPU


def test_struct_layouts_match_gcc():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f1p.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", ' \
          'sizeof(f1p_stmpc_cfg), offsetof(f1p_stmpc_cfg, dt), offsetof(f1p_stmpc_cfg, q), offsetof(f1p_stmpc_cfg, r), ' \
          'offsetof(f1p_stmpc_cfg, params), sizeof(f1p_kmpc_qp_opts), offsetof(f1p_kmpc_qp_opts, tol), F1P_STMPC_QP_MAX_T);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.c"), "-o", os.path.join(d, "l")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    S, O = _abi.StmpcCfg, _abi.KmpcQpOpts
    assert got[:7] == [C.sizeof(S), S.dt.offset, S.q.offset, S.r.offset, S.params.offset, C.sizeof(O), O.tol.offset]
    assert got[7] >= 40
