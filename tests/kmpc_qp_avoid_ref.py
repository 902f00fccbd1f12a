"""numpy restatement of the moving-disc avoidance rows of f1p_kmpc_qp_avoid_* (include/f1p.h) on top of tests/kmpc_qp_ref.py --
the yardstick of tests/test_kmpc_qp_avoid_host.py and tests/test_gpu_kmpc_qp_avoid.py.  A helper module, not a conftest.

The condensed QP of kmpc_qp_ref.condense is kept (u, its 8T-2 rows) and gains the slack eps as input 2T (cost rho eps^2 + lin eps, row
-eps <= 0) and at most two half-plane rows per step against the discs nearest to the linearisation path.  exact_solve wants a feasible
origin: eps is shifted (and scaled), eps = sigma eps' + eps0 with eps0 = max(0, -min h_avoid) + 1 and sigma = 1 / sqrt(2 rho).
"""
import math

import numpy as np

import kmpc_qp_ref as Q
import qp_avoid_ref as R

DEFAULTS = dict(margin=0.0, rho=1e4, lin=10.0)


def _heading(path, t):
    return path[3, t]


def planes(d, c, obs, p, margin):
    """-> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros: absent), A [2T, 2T]: the rows' u-coefficients -n.S_xy(t))"""
    return R.planes(d, c, obs, p["T"], 4, p["DTK"], _heading, margin)


def build(x0, ref, oa, od, obs, p, margin=0.0, rho=1e4, lin=10.0):
    """the avoidance QP over w = (u, eps): dict(H, g, G, h [rows: the plain 8T-2, the 2T avoidance rows in step order (absent ones left
    out: `rows` lists the kept ones' indices into the 2T), then -eps <= 0], planes, data, cond)"""
    d = Q.qp_data(x0, ref, oa, od, p)
    c = Q.condense(d, p["T"])
    return R.build(d, c, *planes(d, c, obs, p, margin), p["T"], rho, lin)


def cert(b, w, lam):
    """the condensed KKT certificate of (w, lam) on build()'s problem (the quantities of test_gpu_kmpc_qp._cond_cert)"""
    grad = b["H"] @ w + b["g"] + b["G"].T @ lam
    sl = b["h"] - b["G"] @ w
    return dict(primal=float(max(0.0, -sl.min())), dual=float(lam.min()), comp=float(np.abs(lam * sl).max()),
                stat=float(np.abs(grad).max() / (1.0 + np.abs(b["g"]).max())))


def cert_ok(c):
    """the bars of test_gpu_kmpc_qp._cert_ok"""
    return c["primal"] <= 1e-9 and c["dual"] >= -1e-10 and c["comp"] <= 1e-9 and c["stat"] <= 1e-8


lam_full = R.lam_full           # the multipliers of build()'s rows from the GPU's duals [8T-2] and avoid_duals [2T+1]


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
