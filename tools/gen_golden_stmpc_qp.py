#!/usr/bin/env python3
"""Generate tests/golden/g17_stmpc_qp.npz: the reference's own dynamic-MPC QPs (both branches of STMPCPlanner), as its code builds them.

Runs ONLY where the reference is mounted (like gen_golden_kmpc_qp.py, whose track loader it uses, and gen_golden.py, whose stand-ins for
numba / matplotlib / pyclothoids it reuses).  cvxpy is replaced by a RECORDING stand-in with SPARSE coefficients: the reference's
dynamic problem scatters its model matrices through `Indexer @ Annz` (control/dynamic_mpc/dynamic_mpc.py:648-669), and a stand-in that
lifts every constant to a dense [*shape, n_vars] array (G16's) would need hundreds of GiB there.  Each affine expression evaluates to
(C: scipy.sparse [size, n_vars], rows in C order of its shape; c: its constant), and Problem.solve records

    1/2 z'Pz + q'z + r,   Aeq z = beq,   G z <= h

instead of solving.  STMPCPlanner.__init__ builds the kinematic problem first (:712-833), so its variables come first; a record is
sliced to the variables of the problem that was solved: z = [vec(x); vec(u)] (dynamic) or [vec(xk); vec(uk)] (kinematic).
The reference's real STMPCPlanner.linear_mpc_control / linear_mpc_control_kinematic is called per case on a FRESH planner (mpc_prob_init
then runs on that case's own linearisation point: see DESIGN.md 5c on the reference's init_flag).  OSQP is absent, so the fixture
holds the reference's PROBLEM, not an answer (tests/stmpc_qp_ref.py solves it).  No reference source is copied.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_kmpc_qp import _tracks  # noqa: E402

REF = gen_golden.REF
OUT = os.path.join(HERE, "..", "tests", "golden", "g17_stmpc_qp.npz")


# ---- the recording cvxpy stand-in (sparse) -------------------------------------------------------------------------------------------
class _Reg:
    variables = []
    records = []

    @classmethod
    def nz(cls):
        return sum(v.size for v in cls.variables)


def _dense(m):
    return m.toarray() if hasattr(m, "toarray") else np.asarray(m, dtype=np.float64)


def _zero(size):
    return sp.csr_matrix((size, _Reg.nz()))


class Expr:
    """an affine expression: ev() -> (C [size, nz] sparse, c [*shape]), evaluated when the problem is solved"""
    __array_priority__ = 1000
    __hash__ = object.__hash__

    def __init__(self, ev, shape):
        self.ev, self.shape = ev, tuple(shape)

    @property
    def size(self):
        return int(np.prod(self.shape)) if self.shape else 1

    @staticmethod
    def lift(x):
        if isinstance(x, Expr):
            return x
        a = _dense(x)
        return Expr(lambda: (_zero(a.size), a), a.shape)

    def _bin(self, other, sgn, rev=False):
        o = Expr.lift(other)
        a, b = (o, self) if rev else (self, o)
        shape = np.broadcast_shapes(a.shape, b.shape)

        def bc(e, C):
            idx = np.broadcast_to(np.arange(e.size).reshape(e.shape), shape).ravel()
            return C[idx]

        def ev():
            Ca, ca = a.ev()
            Cb, cb = b.ev()
            return bc(a, Ca) + sgn * bc(b, Cb), ca + sgn * cb
        return Expr(ev, shape)

    def __add__(self, o):
        return self._bin(o, 1.0)

    def __radd__(self, o):
        return self._bin(o, 1.0, rev=True)

    def __sub__(self, o):
        return self._bin(o, -1.0)

    def __rsub__(self, o):
        return self._bin(o, -1.0, rev=True)

    def __neg__(self):
        return Expr(lambda: tuple(-x for x in self.ev()), self.shape)

    def __matmul__(self, o):            # (parameter-valued matrix) @ affine vector
        o = Expr.lift(o)

        def ev():
            Cm, M = self.ev()
            assert Cm.nnz == 0, "only constant-by-affine products occur at :575-710"
            Co, co = o.ev()
            return sp.csr_matrix(M) @ Co, M @ co
        return Expr(ev, (self.shape[0],) + o.shape[1:])

    def __rmatmul__(self, m):           # scipy.sparse / numpy @ expression: the constant matrix is never lifted
        def ev():
            Co, co = self.ev()
            return sp.csr_matrix(m @ Co), np.asarray(m @ co).reshape(-1)
        return Expr(ev, (m.shape[0],) + self.shape[1:])

    def __getitem__(self, key):
        idx = np.arange(self.size).reshape(self.shape)[key]

        def ev():
            C, c = self.ev()
            return C[idx.ravel()], c[key]
        return Expr(ev, idx.shape)

    def __le__(self, o):
        return Constraint("ineq", self - o)

    def __ge__(self, o):
        return Constraint("ineq", Expr.lift(o) - self)

    def __eq__(self, o):
        return Constraint("eq", self - o)


# plain Expr objects, not subclasses (see gen_golden_kmpc_qp.py: a subclass would flip the sign of `x[:, 0] == x0`)
def Variable(shape):
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    off = _Reg.nz()
    n = int(np.prod(shape))
    pos = np.arange(n).reshape(shape[::-1]).T.ravel()           # column-major: element (i, j) is z[off + i + j * rows]

    def ev():
        return sp.csr_matrix((np.ones(n), (np.arange(n), off + pos)), shape=(n, _Reg.nz())), np.zeros(shape)
    v = Expr(ev, shape)
    v.value = None
    _Reg.variables.append(v)
    return v


def Parameter(shape):
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    p = Expr(None, shape)
    p.value = None
    p.ev = lambda: (_zero(int(np.prod(shape))), np.asarray(p.value, dtype=np.float64).reshape(shape))
    return p


class Constraint:
    def __init__(self, kind, e):
        self.kind, self.e = kind, e


class _Abs:
    def __init__(self, e):
        self.e = e

    def __le__(self, c):                # |e| <= c  ->  e <= c, -e <= c (the upper rows first)
        return (Constraint("ineq", self.e - c), Constraint("ineq", -self.e - c))


class Quad:
    """sum of quad_form terms: (C z + c)' W (C z + c)"""

    def __init__(self, terms):
        self.terms = terms

    def __add__(self, o):
        if isinstance(o, Quad):
            return Quad(self.terms + o.terms)
        return self if np.isscalar(o) and o == 0 else NotImplemented

    __radd__ = __add__

    def data(self):
        nz = _Reg.nz()
        P, q, r = np.zeros((nz, nz)), np.zeros(nz), 0.0
        for e, W in self.terms:
            C, c = e.ev()
            C = C.toarray()
            c = c.reshape(-1)
            P += 2.0 * C.T @ W @ C
            q += 2.0 * C.T @ (W @ c)
            r += float(c @ W @ c)
        return P, q, r


def vec(X):
    idx = np.arange(X.size).reshape(X.shape).ravel(order="F")

    def ev():
        C, c = X.ev()
        return C[idx], c.reshape(-1, order="F")
    return Expr(ev, (X.size,))


def reshape(X, shape, order="C"):
    assert order == "C"

    def ev():
        C, c = X.ev()
        return C, c.reshape(shape)
    return Expr(ev, shape)


def diff(X, k=1, axis=0):
    assert k == 1
    if len(X.shape) == 1:
        return X[1:] - X[:-1]
    return X[:, 1:] - X[:, :-1] if axis == 1 else X[1:, :] - X[:-1, :]


def quad_form(x, P):
    return Quad([(x, _dense(P))])


def psd_wrap(P):
    return P


class Minimize:
    def __init__(self, obj):
        self.obj = obj


class Problem:
    def __init__(self, objective, constraints):
        self.objective, self.constraints = objective, constraints
        self.status = None

    def solve(self, **kw):
        P, q, r = self.objective.obj.data()
        eq, ineq = [], []
        flat = [c for con in self.constraints for c in (con if isinstance(con, tuple) else (con,))]
        for con in flat:
            C, c = con.e.ev()
            (eq if con.kind == "eq" else ineq).append((C.toarray(), c.reshape(-1)))
        Aeq = np.vstack([a for a, _ in eq]); beq = -np.concatenate([b for _, b in eq])
        G = np.vstack([a for a, _ in ineq]); h = -np.concatenate([b for _, b in ineq])
        _Reg.records.append(dict(P=P, q=q, r=r, Aeq=Aeq, beq=beq, G=G, h=h))
        self.status = "recorded"          # neither OPTIMAL nor OPTIMAL_INACCURATE: the reference returns Nones, which is all we need
        return None


def _cvxpy_modules():
    m = types.ModuleType("cvxpy")
    for name, obj in dict(Variable=Variable, Parameter=Parameter, vec=vec, reshape=reshape, diff=diff, quad_form=quad_form,
                          Minimize=Minimize, Problem=Problem, abs=_Abs).items():
        setattr(m, name, obj)
    m.OSQP, m.OPTIMAL, m.OPTIMAL_INACCURATE = "OSQP", "optimal", "optimal_inaccurate"
    atoms, affine, wraps = (types.ModuleType(n) for n in ("cvxpy.atoms", "cvxpy.atoms.affine", "cvxpy.atoms.affine.wraps"))
    wraps.psd_wrap = psd_wrap
    m.atoms, atoms.affine, affine.wraps = atoms, affine, wraps
    return {"cvxpy": m, "cvxpy.atoms": atoms, "cvxpy.atoms.affine": affine, "cvxpy.atoms.affine.wraps": wraps}


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
DYN_KINDS = ["zero", "warm", "vks", "fast", "steer_max", "sharp", "yawrate", "wrap"]
KIN_KINDS = ["zero", "warm", "sharp", "wrap"]


def _pose(rng, tr, name, kind):
    cx, cy, cyaw, sp_, kap = tr[name]
    if kind == "sharp":
        i = int(rng.choice(np.argsort(-np.abs(kap))[:40]))
    elif kind == "wrap":
        i = int(rng.choice(np.argsort(np.abs(np.abs(cyaw) - np.pi))[:40]))
    else:
        i = int(rng.integers(0, len(cx) - 1))
    yaw = cyaw[i] + rng.normal(0, 0.1)
    if kind == "sharp":
        yaw += rng.choice([-1, 1]) * rng.uniform(0.4, 0.9)             # heading error large enough to bind the rate / steering rows
    if kind == "wrap":
        yaw = yaw - 2 * np.pi if yaw > 0 else yaw + 2 * np.pi          # the same heading across the seam: the fold of :227-228 acts
    return cx[i] + rng.normal(0, 0.2), cy[i] + rng.normal(0, 0.2), float(yaw)


def _dyn_case(rng, tr, name, kind, T):
    x, y, yaw = _pose(rng, tr, name, kind)
    v = {"vks": rng.uniform(2.05, 2.5), "fast": rng.choice([6.0, 5.95, 5.8]), "sharp": rng.uniform(3.0, 6.0)}.get(kind, rng.uniform(2.5, 5.5))
    delta = {"steer_max": rng.choice([-0.4189, 0.4189])}.get(kind, rng.uniform(-0.2, 0.2))
    yr, beta = (rng.uniform(-1.5, 1.5), rng.uniform(-0.1, 0.1)) if kind == "yawrate" else (rng.normal(0, 0.1), rng.normal(0, 0.01))
    x0 = np.array([x, y, float(delta), float(v), yaw, float(yr), float(beta)])
    if kind in ("warm", "fast", "sharp", "yawrate") or rng.random() < 0.3:
        oa = rng.normal(0.3, 1.2, T).clip(-3, 3); odv = rng.normal(0, 1.2, T).clip(-3.2, 3.2)
    else:
        oa = odv = None
    return x0, oa, odv


def _kin_case(rng, tr, name, kind, TK):
    x, y, yaw = _pose(rng, tr, name, kind)
    x0 = np.array([x, y, float(rng.uniform(0.3, 2.0)), yaw])
    if kind in ("warm", "sharp"):
        oa = rng.normal(0, 1.5, TK).clip(-3, 3); od = rng.normal(0, 0.25, TK).clip(-0.4189, 0.4189)
    else:
        oa = od = None
    return x0, oa, od


def _store(g, p, rec, lo, hi):
    for m in ("P", "Aeq", "G"):
        A = rec[m][:, lo:hi] if m != "P" else rec[m][lo:hi, lo:hi]
        r_, c_ = np.nonzero(A)
        g[p + m + "_rows"] = r_.astype(np.int32); g[p + m + "_cols"] = c_.astype(np.int32); g[p + m + "_vals"] = A[r_, c_]
        g[p + m + "_shape"] = np.array(A.shape, np.int64)
    g[p + "q"] = rec["q"][lo:hi]
    g[p + "beq"] = rec["beq"]; g[p + "h"] = rec["h"]
    g[p + "r"] = np.float64(rec["r"])


def main():
    gen_golden._install_stubs()
    sys.modules.update(_cvxpy_modules())
    sys.path.insert(0, REF)
    from f1tenth_planning.control.dynamic_mpc import dynamic_mpc as D
    tr = _tracks()
    rng = np.random.default_rng(20261016)
    g = {}
    k = 0
    plan = [("dyn", 40, DYN_KINDS * 3), ("dyn", 10, DYN_KINDS * 2), ("kin", 8, KIN_KINDS * 3)]
    for branch, T, kinds in plan:
        for j, kind in enumerate(kinds):
            name = "levine" if (j + j // len(set(kinds))) % 2 == 0 else "spielberg"      # every kind on both tracks
            cx, cy, cyaw, sp_, _ = tr[name]
            while True:
                cfg = D.mpc_config()
                if branch == "dyn":
                    cfg.T = T
                    x0, oa, od = _dyn_case(rng, tr, name, kind, T)
                else:
                    cfg.TK = T
                    x0, oa, od = _kin_case(rng, tr, name, kind, T)
                _Reg.variables, _Reg.records = [], []
                planner = D.STMPCPlanner(config=cfg)                          # mpc_prob_init_kinematic (:712-833)
                nzk = _Reg.nz()
                cyaw_c = np.array(cyaw, dtype=np.float64)                      # folded in place by the reference (:227-228, :271-272)
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        if branch == "dyn":
                            st = D.State(x=x0[0], y=x0[1], delta=x0[2], v=x0[3], yaw=x0[4], yawrate=x0[5], beta=x0[6])
                            ref = planner.calc_ref_trajectory(st, np.array(cx), np.array(cy), cyaw_c, np.array(sp_))
                            planner.linear_mpc_control(ref, list(x0), oa, od, planner.vehicle_params)
                        else:
                            st = D.State(x=x0[0], y=x0[1], v=x0[2], yaw=x0[3])
                            ref = planner.calc_ref_trajectory_kinematic(st, np.array(cx), np.array(cy), cyaw_c, np.array(sp_))
                            planner.linear_mpc_control_kinematic(ref, list(x0), oa, od)
                except ZeroDivisionError:                                      # a warm start that brakes the prediction to v = 0
                    continue
                break
            rec = _Reg.records[-1]
            lo, hi = (nzk, _Reg.nz()) if branch == "dyn" else (0, nzk)
            p = f"c{k:02d}_"
            g[p + "branch"] = np.array(branch); g[p + "T"] = np.int64(T); g[p + "track"] = np.array(name); g[p + "kind"] = np.array(kind)
            g[p + "x0"] = x0; g[p + "ref"] = ref
            g[p + "oa"] = np.zeros(T) if oa is None else np.asarray(oa); g[p + "od"] = np.zeros(T) if od is None else np.asarray(od)
            g[p + "warm"] = np.bool_(oa is not None)
            _store(g, p, rec, lo, hi)
            k += 1
    g["n_cases"] = np.int64(k)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {k} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
