#!/usr/bin/env python3
"""Generate tests/golden/g16_kmpc_qp.npz: the reference's own kinematic-MPC QP, as its code builds it.

Runs ONLY where the reference is mounted (like gen_golden.py, whose stand-ins for numba / matplotlib / pyclothoids it reuses).  cvxpy is
replaced by a RECORDING stand-in: an affine-expression algebra that covers exactly the calls of the reference's
mpc_prob_init_kinematic / mpc_prob_solve_kinematic (control/kinematic_mpc/kinematic_mpc.py:283-450) -- Variable, Parameter (evaluated
lazily: its values are set after the problem is built), vec (column-major), diff, quad_form, reshape(order="C"), @ with scipy.sparse,
slicing, abs(.) <= c, ==, <=, >= -- and a Problem.solve that records the canonical data instead of solving:

    1/2 z'Pz + q'z + r,   Aeq z = beq,   G z <= h,   z = [vec(xk); vec(uk)]

The reference's real KMPCPlanner.linear_mpc_control_kinematic is then called per case (its own linearisation point, model matrices and
parameter updates).  OSQP is absent, so the fixture holds the reference's PROBLEM, not an answer (tests/kmpc_qp_ref.py solves it).
Matrices are stored as COO triplets.  No reference source is copied; the tests never read the reference.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

REF = gen_golden.REF
OUT = os.path.join(HERE, "..", "tests", "golden", "g16_kmpc_qp.npz")


# ---- the recording cvxpy stand-in --------------------------------------------------------------------------------------------------------
class _Reg:
    variables = []
    records = []

    @classmethod
    def nz(cls):
        return sum(v.size for v in cls.variables)


def _dense(m):
    return m.toarray() if hasattr(m, "toarray") else np.asarray(m, dtype=np.float64)


class Expr:
    """an affine expression: ev() -> (C [*shape, nz], c [*shape]), evaluated when the problem is solved"""
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
        return Expr(lambda: (np.zeros(a.shape + (_Reg.nz(),)), a), a.shape)

    def _bin(self, other, sgn, rev=False):
        o = Expr.lift(other)
        a, b = (o, self) if rev else (self, o)

        def ev():
            Ca, ca = a.ev()
            Cb, cb = b.ev()
            c = ca + sgn * cb
            return np.broadcast_to(Ca, c.shape + (Ca.shape[-1],)) + sgn * np.broadcast_to(Cb, c.shape + (Cb.shape[-1],)), c
        return Expr(ev, np.broadcast_shapes(a.shape, b.shape))

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

    def __matmul__(self, o):            # (parameter / constant matrix) @ affine
        o = Expr.lift(o)

        def ev():
            Cm, M = self.ev()
            assert not Cm.any(), "only constant-by-affine products occur at :283-405"
            Co, co = o.ev()
            return np.tensordot(M, Co, axes=(1, 0)), M @ co
        return Expr(ev, (self.shape[0],) + o.shape[1:])

    def __rmatmul__(self, m):           # scipy.sparse / numpy @ expression
        return Expr.lift(m).__matmul__(self)

    def __getitem__(self, key):
        def ev():
            C, c = self.ev()
            return C[key], c[key]
        return Expr(ev, np.zeros(self.shape)[key].shape)

    def __le__(self, o):
        return Constraint("ineq", self - o)

    def __ge__(self, o):
        return Constraint("ineq", Expr.lift(o) - self)

    def __eq__(self, o):
        return Constraint("eq", self - o)


# Variable / Parameter build plain Expr objects, not subclasses: Python tries a right operand's reflected comparison first when its type
# is a subclass of the left one's, which would flip the sign of `xk[:, 0] == x0k` (:385) against the order the reference writes
def Variable(shape):
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    off = _Reg.nz()
    n = int(np.prod(shape))

    def ev():
        C = np.zeros((n, _Reg.nz()))
        C[np.arange(n), off + np.arange(n)] = 1.0             # column-major: element (i, j) is z[off + i + j * rows]
        return C.reshape(shape[::-1] + (_Reg.nz(),)).transpose(tuple(range(len(shape)))[::-1] + (len(shape),)), np.zeros(shape)
    v = Expr(ev, shape)
    v.value = None
    _Reg.variables.append(v)
    return v


def Parameter(shape):
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    p = Expr(None, shape)
    p.value = None
    p.ev = lambda: (np.zeros(shape + (_Reg.nz(),)), np.asarray(p.value, dtype=np.float64).reshape(shape))
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
            P += 2.0 * C.T @ W @ C
            q += 2.0 * C.T @ (W @ c)
            r += float(c @ W @ c)
        return P, q, r


def vec(X):
    def ev():
        C, c = X.ev()
        if c.ndim == 1:
            return C, c
        return C.transpose(1, 0, 2).reshape(-1, C.shape[-1]), c.reshape(-1, order="F")
    return Expr(ev, (X.size,))


def reshape(X, shape, order="C"):
    assert order == "C"

    def ev():
        C, c = X.ev()
        return C.reshape(tuple(shape) + (C.shape[-1],)), c.reshape(shape)
    return Expr(ev, shape)


def diff(X, k=1, axis=0):
    assert k == 1
    if len(X.shape) == 1:
        return X[1:] - X[:-1]
    return X[:, 1:] - X[:, :-1] if axis == 1 else X[1:, :] - X[:-1, :]


def quad_form(x, P):
    return Quad([(x, _dense(P))])


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
            (eq if con.kind == "eq" else ineq).append((C.reshape(-1, C.shape[-1]), c.reshape(-1)))
        Aeq = np.vstack([a for a, _ in eq]); beq = -np.concatenate([b for _, b in eq])
        G = np.vstack([a for a, _ in ineq]); h = -np.concatenate([b for _, b in ineq])
        _Reg.records.append(dict(P=P, q=q, r=r, Aeq=Aeq, beq=beq, G=G, h=h))
        self.status = "recorded"          # neither OPTIMAL nor OPTIMAL_INACCURATE: the reference returns Nones, which is all we need
        return None


def _cvxpy_module():
    m = types.ModuleType("cvxpy")
    for name, obj in dict(Variable=Variable, Parameter=Parameter, vec=vec, reshape=reshape, diff=diff, quad_form=quad_form,
                          Minimize=Minimize, Problem=Problem, abs=_Abs).items():
        setattr(m, name, obj)
    m.OSQP, m.OPTIMAL, m.OPTIMAL_INACCURATE = "OSQP", "optimal", "optimal_inaccurate"
    return m


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _tracks():
    t = np.load(os.path.join(HERE, "..", "tests", "golden", "tracks.npz"))
    lev, spl = t["levine"], t["spielberg"]
    return {"levine": (lev[:, 1], lev[:, 2], lev[:, 3], lev[:, 5], lev[:, 4]),
            "spielberg": (spl[:, 0], spl[:, 1], spl[:, 3], spl[:, 2], spl[:, 4])}


def _cases(rng, T, n):
    """(track, x0, oa, od, kind) spread over the kinds the fixture must hold"""
    tr = _tracks()
    kinds = ["zero", "warm", "fast", "sharp", "wrap"]
    out = []
    for k in range(n):
        kind = kinds[k % len(kinds)]
        name = "levine" if k % 2 == 0 else "spielberg"
        cx, cy, cyaw, sp, kap = tr[name]
        if kind == "sharp":
            i = int(rng.choice(np.argsort(-np.abs(kap))[:40]))
        elif kind == "wrap":
            i = int(rng.choice(np.argsort(np.abs(np.abs(cyaw) - np.pi))[:40]))
        else:
            i = int(rng.integers(0, len(cx) - 1))
        yaw = cyaw[i] + rng.normal(0, 0.1)
        v = {"fast": rng.choice([6.0, 5.95, 5.8]), "sharp": rng.uniform(3.0, 6.0)}.get(kind, rng.uniform(0.5, 5.5))
        if kind == "sharp":
            yaw += rng.choice([-1, 1]) * rng.uniform(0.3, 0.8)               # heading error large enough to bind the steering / rate bounds
        if kind == "wrap":
            yaw = yaw - 2 * np.pi if yaw > 0 else yaw + 2 * np.pi              # the same heading on the other side of the seam: the fold of :198-203 acts
        x0 = np.array([cx[i] + rng.normal(0, 0.2), cy[i] + rng.normal(0, 0.2), float(v), float(yaw)])
        if kind in ("warm", "fast", "sharp") or k % 3 == 1:
            oa = rng.normal(0, 1.5, T).clip(-3, 3); od = rng.normal(0, 0.25, T).clip(-0.4189, 0.4189)
        else:
            oa = od = None
        out.append((name, x0, oa, od, kind))
    return out


def main():
    gen_golden._install_stubs()
    sys.modules["cvxpy"] = _cvxpy_module()
    sys.path.insert(0, REF)
    from f1tenth_planning.control.kinematic_mpc import kinematic_mpc as K
    tr = _tracks()
    rng = np.random.default_rng(20261015)
    g = {}
    k = 0
    for T, n in ((8, 32), (30, 8)):
        for name, x0, oa, od, kind in _cases(rng, T, n):
            cfg = K.mpc_config()
            cfg.TK = T
            _Reg.variables, _Reg.records = [], []
            planner = K.KMPCPlanner(config=cfg)                               # mpc_prob_init_kinematic (:283-405)
            cx, cy, cyaw, sp, _ = tr[name]
            cyaw = np.array(cyaw, dtype=np.float64)                          # folded in place by the reference (:198-203)
            st = K.State(x=x0[0], y=x0[1], v=x0[2], yaw=x0[3])
            ref = planner.calc_ref_trajectory_kinematic(st, np.array(cx), np.array(cy), cyaw, np.array(sp))
            with contextlib.redirect_stdout(io.StringIO()):
                planner.linear_mpc_control_kinematic(ref, list(x0), None if oa is None else list(oa), None if od is None else list(od))
            rec = _Reg.records[-1]
            p = f"c{k:02d}_"
            g[p + "T"] = np.int64(T); g[p + "track"] = np.array(name); g[p + "kind"] = np.array(kind)
            g[p + "x0"] = x0; g[p + "ref"] = ref
            g[p + "oa"] = np.zeros(T) if oa is None else np.asarray(oa); g[p + "od"] = np.zeros(T) if od is None else np.asarray(od)
            g[p + "warm"] = np.bool_(oa is not None)
            for m in ("P", "Aeq", "G"):
                r_, c_ = np.nonzero(rec[m])
                g[p + m + "_rows"] = r_.astype(np.int32); g[p + m + "_cols"] = c_.astype(np.int32); g[p + m + "_vals"] = rec[m][r_, c_]
                g[p + m + "_shape"] = np.array(rec[m].shape, np.int64)
            for v in ("q", "beq", "h"):
                g[p + v] = rec[v]
            g[p + "r"] = np.float64(rec["r"])
            k += 1
    g["n_cases"] = np.int64(k)
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {k} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
