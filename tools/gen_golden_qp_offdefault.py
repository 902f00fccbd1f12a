#!/usr/bin/env python3
"""Generate tests/golden/g18_qp_offdefault.npz: the reference's own kinematic and dynamic MPC QPs OFF the defaults of its mpc_config.

Runs ONLY where the reference is mounted.  The recording cvxpy stand-ins are imported from gen_golden_kmpc_qp.py (dense, the kinematic
planner) and gen_golden_stmpc_qp.py (sparse, the dynamic planner); no reference source is copied.  Every case has its own mpc_config,
drawn by tests/qp_cases.py (kmpc_spec / stmpc_spec: time step, wheelbase, bounds, Q != Qf, R != Rd, zero weights, vehicle mass and
friction), at the short horizons TK in {2, 3, 9} and T in {2, 5}; its state and previous solution come from qp_cases' input generators,
its reference trajectory from the reference's own calc_ref_trajectory* on qp_cases.track().  The fixture holds the reference's PROBLEM
(P, q, r, Aeq, beq, G, h; matrices as COO triplets) with x0 / ref / oa / od, the spec's seed and the config numbers that were used.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import gen_golden  # noqa: E402
import gen_golden_kmpc_qp as GK  # noqa: E402
import gen_golden_stmpc_qp as GS  # noqa: E402
import qp_cases as QC  # noqa: E402

REF = gen_golden.REF
OUT = os.path.join(ROOT, "tests", "golden", "g18_qp_offdefault.npz")
KIN = [(T, seed) for T in (2, 3, 9) for seed in (3, 5, 8, 10)]         # seed 3: zero weights, seed 5: Rdk = 0
DYN = [(T, seed) for T in (2, 5) for seed in (0, 1, 2, 3)]


def _course():
    rl = QC.track()
    return tuple(np.array(rl[:, k]) for k in (0, 1, 3, 2))               # cx, cy, cyaw, sp


def _forget_planning():
    """the next `import f1tenth_planning...` must find the reference's package, not this repository's of the same name"""
    for m in [m for m in sys.modules if m == "f1tenth_planning" or m.startswith("f1tenth_planning.")]:
        del sys.modules[m]


def _apply(cfg, fields):
    for k, v in fields.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def _store_spec(g, p, seed, spec):
    g[p + "seed"] = np.int64(seed)
    for k, v in spec.items():
        g[p + "cfg_" + k] = np.asarray(v, dtype=np.float64)


def _kin_cases(g, k):
    sys.modules["cvxpy"] = GK._cvxpy_module()
    _forget_planning()
    from f1tenth_planning.control.kinematic_mpc import kinematic_mpc as K
    cx, cy, cyaw, sp = _course()
    for T, seed in KIN:
        spec = QC.kmpc_spec(seed, T)
        GK._Reg.variables, GK._Reg.records = [], []
        planner = K.KMPCPlanner(config=_apply(K.mpc_config(), QC.kmpc_config_fields(spec)))

        def ref_fn(x4, T_, dt):
            s = x4[0]
            return planner.calc_ref_trajectory_kinematic(K.State(x=s[0], y=s[1], v=s[2], yaw=s[3]), cx, cy, cyaw.copy(), sp)[None]
        x0, ref, oa, od = (a[0] for a in QC.kmpc_inputs(seed, QC.kmpc_params(spec), 1, ref_fn))
        with contextlib.redirect_stdout(io.StringIO()):
            planner.linear_mpc_control_kinematic(ref, list(x0), list(oa), list(od))
        p = f"c{k:02d}_"
        g[p + "branch"] = np.array("kin"); g[p + "T"] = np.int64(T)
        g[p + "x0"] = x0; g[p + "ref"] = ref; g[p + "oa"] = oa; g[p + "od"] = od
        _store_spec(g, p, seed, spec)
        GS._store(g, p, GK._Reg.records[-1], 0, GK._Reg.nz())
        k += 1
    return k


def _dyn_cases(g, k):
    sys.modules.update(GS._cvxpy_modules())
    _forget_planning()
    from f1tenth_planning.control.dynamic_mpc import dynamic_mpc as D
    cx, cy, cyaw, sp = _course()
    for T, seed in DYN:
        spec = QC.stmpc_spec(seed, T)
        GS._Reg.variables, GS._Reg.records = [], []
        planner = D.STMPCPlanner(config=_apply(D.mpc_config(), QC.stmpc_config_fields(spec)), params=np.array(spec["vp"]))
        nzk = GS._Reg.nz()                                               # the kinematic problem's variables come first

        def ref_fn(x4, T_, dt):
            s = x4[0]
            return planner.calc_ref_trajectory(D.State(x=s[0], y=s[1], v=s[2], yaw=s[3]), cx, cy, cyaw.copy(), sp)[None]
        x0, ref, oa, od = (a[0] for a in QC.stmpc_inputs(seed, QC.stmpc_params(spec), 1, ref_fn))
        with contextlib.redirect_stdout(io.StringIO()):
            planner.linear_mpc_control(ref, list(x0), oa, od, planner.vehicle_params)
        p = f"c{k:02d}_"
        g[p + "branch"] = np.array("dyn"); g[p + "T"] = np.int64(T)
        g[p + "x0"] = x0; g[p + "ref"] = ref; g[p + "oa"] = oa; g[p + "od"] = od
        _store_spec(g, p, seed, spec)
        GS._store(g, p, GS._Reg.records[-1], nzk, GS._Reg.nz())
        k += 1
    return k


def main():
    gen_golden._install_stubs()
    QC.track()                                  # built by this repository's synth; then the repository leaves the path: its own
    sys.path.remove(ROOT)                       # f1tenth_planning package would shadow the reference's (a namespace package)
    sys.path.insert(0, REF)
    g = {}
    k = _kin_cases(g, 0)
    k = _dyn_cases(g, k)
    g["n_cases"] = np.int64(k)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {k} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
