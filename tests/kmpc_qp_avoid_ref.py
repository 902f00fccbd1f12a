"""numpy restatement of the moving-disc avoidance rows of f1p_kmpc_qp_avoid_* (include/f1p.h) on top of tests/kmpc_qp_ref.py --
the yardstick of tests/test_kmpc_qp_avoid_host.py and tests/test_gpu_kmpc_qp_avoid.py.  A helper module, not a conftest.

The condensed QP of kmpc_qp_ref.condense is kept (u, its 8T-2 rows) and gains the slack eps as input 2T (cost rho eps^2 + lin eps, row
-eps <= 0) and at most two half-plane rows per step against the discs nearest to the linearisation path.  exact_solve wants a feasible
origin: eps is shifted (and scaled), eps = sigma eps' + eps0 with eps0 = max(0, -min h_avoid) + 1 and sigma = 1 / sqrt(2 rho).
"""
import math

import numpy as np

import kmpc_qp_ref as Q

DEFAULTS = dict(margin=0.0, rho=1e4, lin=10.0)


def planes(d, c, obs, p, margin):
    """-> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros: absent), A [2T, 2T]: the rows' u-coefficients -n.S_xy(t))"""
    T, DTK = p["T"], p["DTK"]
    path, Z, z0 = d["path"], c["Z"], c["z0"]
    obs = np.asarray(obs, float).reshape(-1, 5)
    pl = np.zeros((T, 2, 4))
    pl[:, :, 3] = -1.0
    A = np.zeros((2 * T, 2 * T))
    for t in range(1, T + 1):
        tau = float(t) * DTK
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
                nx, ny = -math.cos(path[3, t]), -math.sin(path[3, t])
            else:
                nx, ny = dx / dist, dy / dist
            rhs = nx * (z0[4 * t] - cx) + ny * (z0[4 * t + 1] - cy) - (r + margin)
            pl[t - 1, k] = (nx, ny, rhs, m)
            A[2 * (t - 1) + k] = -(nx * Z[4 * t] + ny * Z[4 * t + 1])
    return pl, A


def build(x0, ref, oa, od, obs, p, margin=0.0, rho=1e4, lin=10.0):
    """the avoidance QP over w = (u, eps): dict(H, g, G, h [rows: the plain 8T-2, the 2T avoidance rows in step order (absent ones left
    out: `rows` lists the kept ones' indices into the 2T), then -eps <= 0], planes, data, cond)"""
    T = p["T"]
    d = Q.qp_data(x0, ref, oa, od, p)
    c = Q.condense(d, T)
    pl, A = planes(d, c, obs, p, margin)
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
    return dict(H=H, g=g, G=G, h=h, planes=pl, rows=keep, m0=m0, data=d, cond=c)


def cert(b, w, lam):
    """the condensed KKT certificate of (w, lam) on build()'s problem (the quantities of test_gpu_kmpc_qp._cond_cert)"""
    grad = b["H"] @ w + b["g"] + b["G"].T @ lam
    sl = b["h"] - b["G"] @ w
    return dict(primal=float(max(0.0, -sl.min())), dual=float(lam.min()), comp=float(np.abs(lam * sl).max()),
                stat=float(np.abs(grad).max() / (1.0 + np.abs(b["g"]).max())))


def cert_ok(c):
    """the bars of test_gpu_kmpc_qp._cert_ok"""
    return c["primal"] <= 1e-9 and c["dual"] >= -1e-10 and c["comp"] <= 1e-9 and c["stat"] <= 1e-8


def lam_full(b, duals, avoid_duals):
    """the multipliers of build()'s rows from the GPU's duals [8T-2] and avoid_duals [2T+1]"""
    return np.concatenate([duals, avoid_duals[:-1][b["rows"]], avoid_duals[-1:]])


def _polish(H, g, G, h, w, lam):
    """exact_solve's point, refined: the KKT system of its active set (the rows with a multiplier) solved again with the residual formed in
    extended precision, three rounds.  At T = 31 the system's conditioning leaves ~1e-10 on the active rows, which multipliers of
    a few hundred turn into a complementarity residual above the certificate's 1e-9.  Kept only if no row and no multiplier turns wrong."""
    W = np.flatnonzero(lam > 0.0)
    if len(W) == 0:
        return w, lam
    n, k = len(w), len(W)
    K = np.block([[H, G[W].T], [G[W], np.zeros((k, k))]])
    rhs = np.concatenate([-g, h[W]]).astype(np.longdouble)
    KL = K.astype(np.longdouble)
    x = np.concatenate([w, lam[W]])
    for _ in range(3):
        r = np.asarray(rhs - KL @ x.astype(np.longdouble), dtype=np.float64)
        x = x + np.linalg.lstsq(K, r, rcond=None)[0]
    w2, l2 = x[:n], np.zeros(len(lam))
    l2[W] = x[n:]
    if l2.min() < 0.0 or (G @ w2 - h).max() > 1e-12 * (1.0 + np.abs(h).max()):
        return w, lam
    return w2, l2


def solve(x0, ref, oa, od, obs, p, margin=0.0, rho=1e4, lin=10.0):
    """exact optimum: dict(u [T][2], eps, lam (build()'s rows), avoid_lam [2T+1] (absent rows 0), degenerate, planes, cert, steer, speed, build)
    or None when infeasible (v0 outside its bounds)"""
    T = p["T"]
    if not Q.feasible(x0, p):
        return None
    b = build(x0, ref, oa, od, obs, p, margin, rho, lin)
    n = 2 * T
    ha = b["h"][b["m0"]:-1]
    eps0 = max(0.0, -float(ha.min()) if len(ha) else 0.0) + 1.0
    w0 = np.zeros(n + 1); w0[n] = eps0
    # w = D w' + w0 with D = diag(1, .., 1, sigma): the origin w' = 0 is feasible (eps = eps0), and sigma = 1 / sqrt(2 rho) makes the slack's
    # curvature 1 like the inputs' (2 rho = 2e4 beside them costs the KKT solves of exact_solve five digits).  The rows and hence the
    # multipliers are those of the unshifted, unscaled problem:  1/2 w'Hw + g'w = 1/2 w''(DHD)w' + (D (g + H w0))'w' + const,  (G D) w' <= h - G w0
    D = np.ones(n + 1); D[n] = 1.0 / math.sqrt(2.0 * rho)
    ws, lam, deg = Q.exact_solve(D[:, None] * b["H"] * D[None, :], D * (b["g"] + b["H"] @ w0), b["G"] * D[None, :], b["h"] - b["G"] @ w0)
    ws, lam = _polish(D[:, None] * b["H"] * D[None, :], D * (b["g"] + b["H"] @ w0), b["G"] * D[None, :], b["h"] - b["G"] @ w0, ws, lam)
    w = D * ws + w0
    al = np.zeros(n + 1)
    al[b["rows"]] = lam[b["m0"]:-1]
    al[n] = lam[-1]
    return dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=deg, planes=b["planes"], cert=cert(b, w, lam),
                steer=float(w[1]), speed=float(x0[2] + w[0] * p["DTK"]), build=b)


# ---- the two levine scenes of the closed-loop tests ------------------------------------------------------------------------------------
def parked_disc(cx, cy, cyaw, k=120, off=0.15, r=0.45):
    """a disc of radius r, `off` metres left of raceline waypoint k"""
    return np.array([cx[k] - off * math.sin(cyaw[k]), cy[k] + off * math.cos(cyaw[k]), 0.0, 0.0, r])


def moving_disc(cx, cy, cyaw, k=60, v=1.5, r=0.45):
    """a disc on waypoint k that moves at v m/s along the course heading there"""
    return np.array([cx[k], cy[k], v * math.cos(cyaw[k]), v * math.sin(cyaw[k]), r])


def disc_at(disc, t):
    """the disc's row at time t [s]"""
    return np.array([disc[0] + disc[2] * t, disc[1] + disc[3] * t, disc[2], disc[3], disc[4]])
