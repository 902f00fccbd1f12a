"""numpy restatement of the wall rows of f1p_stmpc_qp_walls_* (include/f1p.h) on top of tests/kmpc_qp_walls_ref.py (the march, the
candidates, the grid helpers), tests/stmpc_qp_avoid_ref.py and tests/stmpc_qp_ref.py (the dynamic problem, the heading, the certificate and the
scaled solve) -- the yardstick of tests/test_stmpc_qp_walls_host.py and tests/test_gpu_stmpc_qp_walls.py.  A helper module, not a conftest;
pure numpy; nothing here is shared with the library's code.

Per step t = 1..T the walls are looked for left and right of the DIRECTION OF TRAVEL w = psibar_t + betabar_t (stmpc_qp_avoid_ref._heading), from
pbar_t = path[:2, t]; of {the live discs, wall L (slot 16), wall R (slot 17)} the two smallest clearances are the step's rows, ties to the
lower slot.  The rows go to qp_avoid_ref.build, the solve is stmpc_qp_avoid_ref's.
"""
import math

import numpy as np

import qp_avoid_ref as R
import stmpc_qp_avoid_ref as A
import stmpc_qp_ref as SQ
from kmpc_qp_walls_ref import SLOT_L, SLOT_R, brute_first_hit, cell, from_image, march, near_edge, occupied, sample, wall_candidates  # noqa: F401

DEFAULTS = dict(n_samples=48, wall_margin=0.0)
heading = A._heading


def planes(d, c, obs, grid, p, n_samples, margin=0.0, wall_margin=0.0, heading=heading):
    """-> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros: absent), A [2T, 2T]: the rows' u-coefficients, edge).
    heading(path, t): the angle the walls are looked for beside (a test may hand the bare yaw to see that it matters)"""
    T, dt = p["T"], p["DT"]
    path, Z, z0 = d["path"], c["Z"], c["z0"]
    obs = np.zeros((0, 5)) if obs is None else np.asarray(obs, float).reshape(-1, 5)
    pl = np.zeros((T, 2, 4))
    pl[:, :, 3] = -1.0
    Am = np.zeros((2 * T, 2 * T))
    edge = False
    for t in range(1, T + 1):
        tau = float(t) * dt
        px, py, w = path[0, t], path[1, t], heading(path, t)
        cands = []                                               # (clear, slot, centre / contact, normal, what the right-hand side takes off)
        for m, (x, y, vx, vy, r) in enumerate(obs):
            if not r >= 0.0:
                continue
            cx, cy = x + vx * tau, y + vy * tau
            dx, dy = px - cx, py - cy
            dist = math.sqrt(dx * dx + dy * dy)
            n = (-math.cos(A._heading(path, t)), -math.sin(A._heading(path, t))) if dist < 1e-9 else (dx / dist, dy / dist)
            cands.append((dist - r, m, (cx, cy), n, r + margin))
        walls, e = wall_candidates(grid, px, py, w, n_samples)
        edge |= e
        cands += [(cl, slot, cc, n, wall_margin) for cl, slot, cc, n in walls]
        cands.sort(key=lambda q: (q[0], q[1]))
        for k, (cl, slot, (cx, cy), (nx_, ny_), off) in enumerate(cands[:2]):
            rhs = nx_ * (z0[7 * t] - cx) + ny_ * (z0[7 * t + 1] - cy) - off
            pl[t - 1, k] = (nx_, ny_, rhs, slot)
            Am[2 * (t - 1) + k] = -(nx_ * Z[7 * t] + ny_ * Z[7 * t + 1])
    return pl, Am, edge


def build(x0, ref, oa, odv, obs, grid, p, n_samples, margin=0.0, rho=1e4, lin=10.0, wall_margin=0.0, heading=heading):
    """qp_avoid_ref.build on the rows above; the dict gains `edge`"""
    d = SQ.qp_data(x0, ref, oa, odv, p)
    c = SQ.condense(d, p["T"])
    pl, Am, edge = planes(d, c, obs, grid, p, n_samples, margin, wall_margin, heading)
    b = R.build(d, c, pl, Am, p["T"], rho, lin)
    b["edge"] = edge
    return b


cert, cert_ok, lam_full, u_bar, scaled = A.cert, A.cert_ok, A.lam_full, A.u_bar, A.scaled


def result(b, x0, p, w, lam, deg):
    """stmpc_qp_avoid_ref.solve's dict (+ edge) of the point (w, lam) on build()'s problem"""
    T = p["T"]
    n = 2 * T
    al = np.zeros(n + 1)
    al[b["rows"]] = lam[b["m0"]:-1]
    al[n] = lam[-1]
    ct = cert(b, w, lam)
    return dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=bool(deg), planes=b["planes"], cert=ct,
                certified=cert_ok(ct, lam), steer=float(x0[2] + w[0] * p["DT"]), speed=float(x0[3] + w[1] * p["DT"]),
                obj=float(0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"]), build=b, edge=b["edge"])


def try_build(x0, ref, oa, odv, obs, grid, p, n_samples, margin=0.0, rho=1e4, lin=10.0, wall_margin=0.0):
    """build(), or None when the problem is infeasible (delta0 / v0 outside their bounds) or an input or the model is not finite"""
    x0 = np.asarray(x0, float)
    if not np.isfinite(x0).all() or not SQ.feasible(x0, p):
        return None
    with np.errstate(all="ignore"):
        try:
            b = build(x0, ref, oa, odv, obs, grid, p, n_samples, margin, rho, lin, wall_margin)
        except ZeroDivisionError:
            return None
    if not (np.isfinite(b["H"]).all() and np.isfinite(b["g"]).all() and np.isfinite(b["h"]).all()):
        return None
    return b


def solve_built(b, x0, p, lam_hint=None):
    """stmpc_qp_avoid_ref.solve's shift, scale, exact solve and polish, on a built problem"""
    cs, D, w0 = scaled(b)
    ws, lam, deg = SQ.exact(cs, lam_hint)
    ws, lam = A._polish(cs["H"], cs["g"], cs["G"], cs["h"], ws, lam)
    return result(b, np.asarray(x0, float), p, D * ws + w0, lam, deg)


def solve(x0, ref, oa, odv, obs, grid, p, n_samples, margin=0.0, rho=1e4, lin=10.0, wall_margin=0.0):
    """exact optimum of the wall problem: stmpc_qp_avoid_ref.solve's dict (+ edge), or None where try_build gives None"""
    b = try_build(x0, ref, oa, odv, obs, grid, p, n_samples, margin, rho, lin, wall_margin)
    return None if b is None else solve_built(b, x0, p)
