"""The linearised kinematic-MPC QP on the host: the yardstick (tests/kmpc_qp_ref.py) against the reference's own problem data (golden G16,
recorded from the reference's code by tools/gen_golden_kmpc_qp.py), its exact solver against the KKT certificate, the class's solver
switch, and the f1p_kmpc_qp_opts layout.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kmpc_qp_ref as Q
from f1tenth_planning_amd import _abi
from f1tenth_planning_amd.control.kinematic_mpc.kinematic_mpc import KMPCPlanner, mpc_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g16_cases(golden):
    g = golden("g16_kmpc_qp.npz")

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
        out.append(dict(T=int(g[p + "T"]), kind=str(g[p + "kind"]), x0=g[p + "x0"], ref=g[p + "ref"], oa=g[p + "oa"], od=g[p + "od"],
                        warm=bool(g[p + "warm"]), rec=rec))
    return out


def test_g16_covers_the_cases(golden):
    cases = g16_cases(golden)
    assert len(cases) == 40 and sum(c["T"] == 8 for c in cases) == 32 and sum(c["T"] == 30 for c in cases) == 8
    assert {c["kind"] for c in cases} == {"zero", "warm", "fast", "sharp", "wrap"}
    assert any(c["warm"] for c in cases) and any(not c["warm"] for c in cases)
    assert any(c["x0"][2] >= 5.9 for c in cases)
    assert any(abs(c["x0"][3]) > np.pi for c in cases)


def test_helper_qp_data_equals_the_references(golden):
    """pins delta_bar = 0, the unshifted warm start, the t = 0 objective term and the column-major ordering"""
    for k, c in enumerate(g16_cases(golden)):
        d = Q.qp_data(c["x0"], c["ref"], c["oa"], c["od"], Q.default_params(c["T"]))
        for m in ("P", "Aeq", "G", "q", "beq", "h"):
            a, b = c["rec"][m], d[m]
            assert a.shape == b.shape, (k, m)
            assert np.abs(a - b).max() <= 1e-12 * (1.0 + np.abs(a).max()), (k, m)
        assert abs(c["rec"]["r"] - d["r"]) <= 1e-12 * (1.0 + abs(d["r"])), k


def test_helper_exact_solutions_pass_the_certificate(golden):
    n_exact = 0
    for k, c in enumerate(g16_cases(golden)):
        p = Q.default_params(c["T"])
        s = Q.solve_case(c["x0"], c["ref"], c["oa"], c["od"], p)
        r = c["rec"]
        lam = np.zeros(len(r["h"]))
        lam[Q.gpu_rows(c["T"])] = s["lam"]
        z = np.concatenate([s["xk"].T.ravel(), s["u"].ravel()])
        cert = Q.certificate(r["P"], r["q"], r["Aeq"], r["beq"], r["G"], r["h"], z, lam)
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
        KMPCPlanner(config=c)
    c = mpc_config(SOLVER="qp")
    c.Rdk = np.array([[0.01, 0.001], [0.001, 100.0]])
    with pytest.raises(ValueError):
        KMPCPlanner(config=c)
    ok = mpc_config(SOLVER="qp")
    pl = KMPCPlanner(config=ok)
    pl.config.Qk = np.ones((4, 4))
    with pytest.raises(ValueError):
        pl.plan_batch(np.zeros((1, 4)), waypoints=np.zeros((4, 10)))
    assert pl._ctx is None                                   # nothing touched the GPU


def test_qp_opts_layout_matches_gcc():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "f1p.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(f1p_kmpc_qp_opts), ' \
          'offsetof(f1p_kmpc_qp_opts, max_iter), offsetof(f1p_kmpc_qp_opts, pad), offsetof(f1p_kmpc_qp_opts, tol));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "l.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "l.c"), "-o", os.path.join(d, "l")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "l")]).split()]
    O = _abi.KmpcQpOpts
    assert got == [C.sizeof(O), O.max_iter.offset, O.pad.offset, O.tol.offset]
    o = _abi.kmpc_qp_opts()
    assert (o.max_iter, o.tol) == (50, 1e-10)
