"""numpy restatement of the moving-disc avoidance rows of f1p_stmpc_qp_avoid_* (include/f1p.h) on top of tests/stmpc_qp_ref.py --
the yardstick of tests/test_stmpc_qp_avoid_host.py and tests/test_gpu_stmpc_qp_avoid.py; to stmpc_qp_ref.py what kmpc_qp_avoid_ref.py is to
kmpc_qp_ref.py.  A helper module, not a conftest.

The condensed QP of stmpc_qp_ref.condense is kept (u = (steer_v_0, accel_0, ...), its 10T-2 rows) and gains the slack eps as input 2T (cost
rho eps^2 + lin eps, row -eps <= 0) and at most two half-plane rows per step against the discs nearest to the linearisation path
predict_motion(x0, oa, od_v).  The exact solvers want a well-scaled problem with a feasible origin: eps is shifted and scaled,
eps = sigma eps' + eps0 with eps0 = max(0, -min h_avoid) + 1 and sigma = 1 / sqrt(2 rho).
"""
import math

import numpy as np

import qp_avoid_ref as R
import stmpc_qp_ref as SQ
from kmpc_qp_avoid_ref import _polish, disc_at, moving_disc, parked_disc  # noqa: F401  (the levine scenes' discs are the kinematic tests')

DEFAULTS = dict(margin=0.0, rho=1e4, lin=10.0)


def _heading(path, t):
    return path[4, t] + path[6, t]                               # the direction of travel: yaw + beta


def planes(d, c, obs, p, margin):
    """-> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros: absent), A [2T, 2T]: the rows' u-coefficients -n.S_xy(t))"""
    return R.planes(d, c, obs, p["T"], 7, p["DT"], _heading, margin)


def build(x0, ref, oa, odv, obs, p, margin=0.0, rho=1e4, lin=10.0):
    """the avoidance QP over w = (u, eps): dict(H, g, G, h [rows: the plain 10T-2, the 2T avoidance rows in step order (absent ones left
    out: `rows` lists the kept ones' indices into the 2T), then -eps <= 0], planes, data, cond, rho, lin)"""
    d = SQ.qp_data(x0, ref, oa, odv, p)
    c = SQ.condense(d, p["T"])
    return R.build(d, c, *planes(d, c, obs, p, margin), p["T"], rho, lin)


def cert(b, w, lam):
    """the condensed KKT certificate of (w, lam) on build()'s problem (stmpc_qp_ref.cond_cert's quantities)"""
    return SQ.cond_cert(b, w, lam)


def cert_ok(c, lam):
    """DESIGN.md 5c's bars: stmpc_qp_ref.cert_ok with the complementarity relative to the multipliers' scale (they reach ~1e3 here)"""
    c = dict(c)
    c["comp"] /= 1.0 + float(np.max(lam))
    return SQ.cert_ok(c)


lam_full = R.lam_full           # the multipliers of build()'s rows from the GPU's duals [10T-2] and avoid_duals [2T+1]


def scaled(b):
    """build()'s problem over w' with w = D w' + w0 -> (dict(H, g, G, h), D, w0).  w0 = (0, eps0) makes the origin feasible; D = diag(1, ..,
    1, sigma), sigma = 1 / sqrt(2 rho), gives the slack the curvature 1 (2 rho = 2e4 beside the inputs' costs the KKT solves five digits).
    The rows and hence the multipliers are those of the unshifted, unscaled problem:
    1/2 w'Hw + g'w = 1/2 w''(DHD)w' + (D (g + H w0))'w' + const,  (G D) w' <= h - G w0"""
    n = len(b["g"]) - 1
    ha = b["h"][b["m0"]:-1]
    eps0 = max(0.0, -float(ha.min()) if len(ha) else 0.0) + 1.0
    w0 = np.zeros(n + 1); w0[n] = eps0
    D = np.ones(n + 1); D[n] = 1.0 / math.sqrt(2.0 * b["rho"])
    return dict(H=D[:, None] * b["H"] * D[None, :], g=D * (b["g"] + b["H"] @ w0), G=b["G"] * D[None, :], h=b["h"] - b["G"] @ w0), D, w0


def solve(x0, ref, oa, odv, obs, p, margin=0.0, rho=1e4, lin=10.0, lam_hint=None):
    """exact optimum: dict(u [T][2], eps, w, lam (build()'s rows), avoid_lam [2T+1] (absent rows 0), degenerate, planes, cert, certified,
    steer, speed, obj, build) or None when infeasible (delta0 / v0 outside their bounds) or the model is not finite"""
    T = p["T"]
    x0 = np.asarray(x0, float)
    if not SQ.feasible(x0, p):
        return None
    with np.errstate(all="ignore"):
        try:
            b = build(x0, ref, oa, odv, obs, p, margin, rho, lin)
        except ZeroDivisionError:
            return None
    if not (np.isfinite(b["H"]).all() and np.isfinite(b["g"]).all() and np.isfinite(b["h"]).all()):
        return None
    n = 2 * T
    cs, D, w0 = scaled(b)
    ws, lam, deg = SQ.exact(cs, lam_hint)
    ws, lam = _polish(cs["H"], cs["g"], cs["G"], cs["h"], ws, lam)
    w = D * ws + w0
    al = np.zeros(n + 1)
    al[b["rows"]] = lam[b["m0"]:-1]
    al[n] = lam[-1]
    ct = cert(b, w, lam)
    obj = float(0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"])
    return dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=bool(deg), planes=b["planes"], cert=ct,
                certified=cert_ok(ct, lam), steer=float(x0[2] + w[0] * p["DT"]), speed=float(x0[3] + w[1] * p["DT"]), obj=obj, build=b)


def u_bar(b, w, lam, ws, lam_s, deg):
    """DESIGN.md 5c's distance rule on build()'s problem: 1e-7, 1e-5 where degenerate, or the strong-convexity bound from both points'
    residuals (tests/test_gpu_stmpc_qp.py _u_bar), whichever is larger"""
    H, g, G, h = b["H"], b["g"], b["G"], b["h"]
    mu = np.linalg.eigvalsh(H).min()
    dr = np.linalg.norm((H @ w + g + G.T @ lam) - (H @ ws + g + G.T @ lam_s))
    gap = np.abs(lam * (h - G @ w)).sum() + np.abs(lam_s * (h - G @ ws)).sum()
    return max(1e-5 if deg else 1e-7, 2.0 * (dr + np.sqrt(dr * dr + 4.0 * mu * gap)) / (2.0 * mu))
