"""What the numpy yardsticks of the two QPs' moving-disc avoidance rows share (tests/kmpc_qp_avoid_ref.py, tests/stmpc_qp_avoid_ref.py): the
half-planes, the QP over w = (u, eps) on top of a model's condensed plain QP, and the multipliers' order.  A model is (nx, dt, heading): the
state width, the time step, and heading(path, t) = the direction of travel at the linearisation path's step t, the fallback normal's.  Pure
numpy; a helper module, not a conftest; nothing here is shared with the library's code.
"""
import math

import numpy as np


def planes(d, c, obs, T, nx, dt, heading, margin):
    """d: the model's qp_data (path), c: its condense (Z, z0) -> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros:
    absent), A [2T, 2T]: the rows' u-coefficients -n.S_xy(t))"""
    path, Z, z0 = d["path"], c["Z"], c["z0"]
    obs = np.asarray(obs, float).reshape(-1, 5)
    pl = np.zeros((T, 2, 4))
    pl[:, :, 3] = -1.0
    A = np.zeros((2 * T, 2 * T))
    for t in range(1, T + 1):
        tau = float(t) * dt
        px, py = path[0, t], path[1, t]
        c0 = c1 = math.inf
        m0 = m1 = -1
        for m, (x, y, vx, vy, r) in enumerate(obs):
            if not r >= 0.0:
                continue
            dx, dy = px - (x + vx * tau), py - (y + vy * tau)
            clear = math.sqrt(dx * dx + dy * dy) - r
            if clear < c0:
                c1, m1, c0, m0 = c0, m0, clear, m
            elif clear < c1:
                c1, m1 = clear, m
        for k, m in enumerate((m0, m1)):
            if m < 0:
                continue
            x, y, vx, vy, r = obs[m]
            cx, cy = x + vx * tau, y + vy * tau
            dx, dy = px - cx, py - cy
            dist = math.sqrt(dx * dx + dy * dy)
            if dist < 1e-9:
                nx_, ny_ = -math.cos(heading(path, t)), -math.sin(heading(path, t))
            else:
                nx_, ny_ = dx / dist, dy / dist
            rhs = nx_ * (z0[nx * t] - cx) + ny_ * (z0[nx * t + 1] - cy) - (r + margin)
            pl[t - 1, k] = (nx_, ny_, rhs, m)
            A[2 * (t - 1) + k] = -(nx_ * Z[nx * t] + ny_ * Z[nx * t + 1])
    return pl, A


def build(d, c, pl, A, T, rho, lin):
    """the avoidance QP over w = (u, eps) from the plain QP's (d, c) and planes()'s (pl, A): dict(H, g, G, h [rows: the plain ones, the 2T
    avoidance rows in step order (absent ones left out: `rows` lists the kept ones' indices into the 2T), then -eps <= 0], planes, data,
    cond, rho, lin)"""
    n = 2 * T
    keep = np.flatnonzero(pl.reshape(-1, 4)[:, 3] >= 0)
    H = np.zeros((n + 1, n + 1)); H[:n, :n] = c["H"]; H[n, n] = 2.0 * rho
    g = np.concatenate([c["g"], [lin]])
    m0 = len(c["h"])
    G = np.zeros((m0 + len(keep) + 1, n + 1))
    G[:m0, :n] = c["G"]
    G[m0:m0 + len(keep), :n] = A[keep]
    G[m0:m0 + len(keep), n] = -1.0
    G[-1, n] = -1.0
    h = np.concatenate([c["h"], pl.reshape(-1, 4)[keep, 2], [0.0]])
    return dict(H=H, g=g, G=G, h=h, planes=pl, rows=keep, m0=m0, data=d, cond=c, rho=rho, lin=lin)


def lam_full(b, duals, avoid_duals):
    """the multipliers of build()'s rows from the GPU's duals (the plain rows) and avoid_duals [2T+1]"""
    return np.concatenate([duals, avoid_duals[:-1][b["rows"]], avoid_duals[-1:]])
