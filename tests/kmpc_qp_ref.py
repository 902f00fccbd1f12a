"""numpy restatement of the reference's linearised kinematic MPC QP (control/kinematic_mpc/kinematic_mpc.py:245-508) -- the yardstick of
f1p_kmpc_qp_* (tests/test_kmpc_qp_host.py, tests/test_gpu_kmpc_qp.py).  A helper module, not a conftest.

  * qp_data():     the problem as cvxpy would canonicalise it over z = [vec(xk); vec(uk)] (column-major):
                   1/2 z'Pz + q'z + r,  Aeq z = beq,  G z <= h, rows in the order the reference lists its constraints
                   (tools/gen_golden_kmpc_qp.py records the same data from the reference's own code: tests/golden/g16_kmpc_qp.npz)
  * condense():    the states eliminated (x = S u + s): 1/2 u'Hu + g'u + c over u = vec(uk), n = 2T, with the inequality rows in the
                   order of f1p_kmpc_qp_batch's duals (a upper, a lower, delta upper, delta lower, rate upper, rate lower, v_1..T upper,
                   v_1..T lower)
  * exact_solve(): scipy SLSQP, then an active-set polish that solves the equality-constrained KKT system exactly
  * certificate(): the KKT residuals of (z, duals) on the full problem
"""
import math

import numpy as np


def params(c):
    """the numbers of an mpc_config (f1tenth_planning_amd ... kinematic_mpc.mpc_config) the QP uses"""
    return dict(T=int(c.TK), DTK=float(c.DTK), WB=float(c.WB), MAX_STEER=float(c.MAX_STEER), MAX_DSTEER=float(c.MAX_DSTEER),
                MAX_SPEED=float(c.MAX_SPEED), MIN_SPEED=float(c.MIN_SPEED), MAX_ACCEL=float(c.MAX_ACCEL),
                Rk=np.asarray(c.Rk, float), Rdk=np.asarray(c.Rdk, float), Qk=np.asarray(c.Qk, float), Qfk=np.asarray(c.Qfk, float))


def default_params(T=8):
    return dict(T=T, DTK=0.1, WB=0.33, MAX_STEER=0.4189, MAX_DSTEER=np.deg2rad(180.0), MAX_SPEED=6.0, MIN_SPEED=0.0, MAX_ACCEL=3.0,
                Rk=np.diag([0.01, 100.0]), Rdk=np.diag([0.01, 100.0]), Qk=np.diag([13.5, 13.5, 5.5, 13.0]), Qfk=np.diag([13.5, 13.5, 5.5, 13.0]))


def predict_motion(x0, oa, od, p):
    """predict_motion_kinematic / update_state_kinematic (:208-243): [4][T+1]"""
    T = len(oa)
    path = np.zeros((4, T + 1))
    path[:, 0] = x0
    x, y, v, yaw = (float(s) for s in x0)
    for t in range(T):
        d = float(od[t])
        if d >= p["MAX_STEER"]:
            d = p["MAX_STEER"]
        elif d <= -p["MAX_STEER"]:
            d = -p["MAX_STEER"]
        x, y, yaw, v = (x + v * math.cos(yaw) * p["DTK"], y + v * math.sin(yaw) * p["DTK"],
                        yaw + (v / p["WB"]) * math.tan(d) * p["DTK"], v + float(oa[t]) * p["DTK"])
        v = min(max(v, p["MIN_SPEED"]), p["MAX_SPEED"]) if (v > p["MAX_SPEED"] or v < p["MIN_SPEED"]) else v
        path[:, t + 1] = (x, y, v, yaw)
    return path


def model(v, phi, p, delta=0.0):
    """get_kinematic_model_matrix (:245-278)"""
    DTK, WB = p["DTK"], p["WB"]
    A = np.eye(4)
    A[0, 2] = DTK * math.cos(phi)
    A[0, 3] = -DTK * v * math.sin(phi)
    A[1, 2] = DTK * math.sin(phi)
    A[1, 3] = DTK * v * math.cos(phi)
    A[3, 2] = DTK * math.tan(delta) / WB
    B = np.zeros((4, 2))
    B[2, 0] = DTK
    B[3, 1] = DTK * v / (WB * math.cos(delta) ** 2)
    C = np.zeros(4)
    C[0] = DTK * v * math.sin(phi) * phi
    C[1] = -DTK * v * math.cos(phi) * phi
    C[3] = -DTK * v * delta / (WB * math.cos(delta) ** 2)
    return A, B, C


def _quad(P, q, r, Cm, c, W):
    """add the quadratic form (Cm z + c)' W (Cm z + c) to 1/2 z'Pz + q'z + r"""
    P += 2.0 * Cm.T @ W @ Cm
    q += 2.0 * Cm.T @ (W @ c)
    return r + float(c @ W @ c)


def qp_data(x0, ref, oa, od, p):
    """The QP of mpc_prob_init_kinematic / mpc_prob_solve_kinematic (:283-450) at the linearisation point of linear_mpc_control_kinematic
    (:452-475): oa / od are the previous solution, NOT shifted; None = zeros.  z = [vec(xk) (x_t at 4 t + k); vec(uk) (u_t at NX + 2 t + j)]."""
    T = p["T"]
    oa = np.zeros(T) if oa is None else np.asarray(oa, float)
    od = np.zeros(T) if od is None else np.asarray(od, float)
    ref = np.asarray(ref, float)
    NX, NU = 4 * (T + 1), 2 * T
    nz = NX + NU
    X = lambda t, k: 4 * t + k            # noqa: E731
    U = lambda t, j: NX + 2 * t + j       # noqa: E731
    P = np.zeros((nz, nz)); q = np.zeros(nz); r = 0.0
    Eu = np.zeros((NU, nz)); Eu[np.arange(NU), NX + np.arange(NU)] = 1.0
    Ex = np.zeros((NX, nz)); Ex[np.arange(NX), np.arange(NX)] = 1.0
    Rb = np.kron(np.eye(T), p["Rk"])
    r = _quad(P, q, r, Eu, np.zeros(NU), Rb)                                       # :324-325
    Qb = np.zeros((NX, NX))
    for t in range(T + 1):
        Qb[4 * t:4 * t + 4, 4 * t:4 * t + 4] = p["Qfk"] if t == T else p["Qk"]
    r = _quad(P, q, r, Ex, -ref.reshape(-1, order="F"), Qb)                        # :327-328
    D = np.zeros((2 * (T - 1), nz))
    for t in range(T - 1):
        for j in range(2):
            D[2 * t + j, U(t + 1, j)] = 1.0
            D[2 * t + j, U(t, j)] = -1.0
    r = _quad(P, q, r, D, np.zeros(2 * (T - 1)), np.kron(np.eye(T - 1), p["Rdk"]))   # :330-331
    path = predict_motion(np.asarray(x0, float), oa, od, p)
    Aeq = np.zeros((4 * T + 4, nz)); beq = np.zeros(4 * T + 4)
    for t in range(T):                                                             # :370-377
        A, B, C = model(path[2, t], path[3, t], p, 0.0)
        for k in range(4):
            row = 4 * t + k
            Aeq[row, X(t + 1, k)] = 1.0
            Aeq[row, [X(t, i) for i in range(4)]] -= A[k]
            Aeq[row, [U(t, j) for j in range(2)]] -= B[k]
            beq[row] = C[k]
    for k in range(4):                                                             # :385
        Aeq[4 * T + k, X(0, k)] = 1.0
        beq[4 * T + k] = x0[k]
    rows, h = [], []

    def add(coef, bound):
        rows.append(coef); h.append(bound)

    for sgn in (1.0, -1.0):                                                        # :379-383 |diff(delta)| <= MAX_DSTEER DTK
        for t in range(T - 1):
            c = np.zeros(nz); c[U(t + 1, 1)] = sgn; c[U(t, 1)] = -sgn
            add(c, p["MAX_DSTEER"] * p["DTK"])
    for t in range(T + 1):                                                         # :386 v <= MAX_SPEED
        c = np.zeros(nz); c[X(t, 2)] = 1.0; add(c, p["MAX_SPEED"])
    for t in range(T + 1):                                                         # :387 v >= MIN_SPEED
        c = np.zeros(nz); c[X(t, 2)] = -1.0; add(c, -p["MIN_SPEED"])
    for j, bound in ((0, p["MAX_ACCEL"]), (1, p["MAX_STEER"])):                    # :388-389 |a| <= MAX_ACCEL, |delta| <= MAX_STEER
        for sgn in (1.0, -1.0):
            for t in range(T):
                c = np.zeros(nz); c[U(t, j)] = sgn; add(c, bound)
    return dict(P=P, q=q, r=r, Aeq=Aeq, beq=beq, G=np.array(rows), h=np.array(h), path=path)


def gpu_rows(T):
    """index into qp_data's G rows of each dual of f1p_kmpc_qp_batch (a upper, a lower, delta upper, delta lower, rate upper, rate lower,
    v_1..T upper, v_1..T lower); qp_data's v_0 rows have no dual there (x_0 is fixed)"""
    r0 = 0                      # rate upper
    v0 = 2 * (T - 1)            # v upper t = 0..T, then v lower t = 0..T
    b0 = v0 + 2 * (T + 1)       # a upper, a lower, d upper, d lower
    idx = list(range(b0, b0 + 4 * T)) + list(range(r0, r0 + 2 * (T - 1)))
    idx += [v0 + t for t in range(1, T + 1)] + [v0 + T + 1 + t for t in range(1, T + 1)]
    return np.array(idx)


def condense(d, T):
    """eliminate the states: z = Z u + z0.  Returns H, g, c (objective 1/2 u'Hu + g'u + c), Gc, hc in the GPU's row order, Z, z0."""
    NX, NU = 4 * (T + 1), 2 * T
    Ax, Au = d["Aeq"][:, :NX], d["Aeq"][:, NX:]
    Sx = np.linalg.solve(Ax, -Au)            # Ax is unit lower block-triangular: exact up to rounding
    sx = np.linalg.solve(Ax, d["beq"])
    Z = np.vstack([Sx, np.eye(NU)]); z0 = np.concatenate([sx, np.zeros(NU)])
    P, q = d["P"], d["q"]
    H = Z.T @ P @ Z
    g = Z.T @ (P @ z0 + q)
    c = 0.5 * z0 @ P @ z0 + q @ z0 + d["r"]
    idx = gpu_rows(T)
    G, h = d["G"][idx], d["h"][idx]
    Gc = G @ Z
    hc = h - G @ z0
    return dict(H=0.5 * (H + H.T), g=g, c=c, G=Gc, h=hc, Z=Z, z0=z0)


def feasible(x0, p):
    return p["MIN_SPEED"] <= x0[2] <= p["MAX_SPEED"]


def exact_solve(H, g, G, h, zero_feasible=True):
    """min 1/2 u'Hu + g'u  s.t. G u <= h (H positive definite), exactly.  scipy SLSQP gives a near-optimal point; it is pulled back toward
    u = 0 (feasible whenever the problem is: a = delta = 0) until it is feasible, and a primal active-set method polishes from there: each
    step solves the equality-constrained KKT system of the working set exactly, stops at a blocking row, drops a row with a negative
    multiplier, until the step is zero and every multiplier is >= 0 (Nocedal & Wright, Algorithm 16.3).
    Returns u, lam [m], degenerate (a row at its bound with a zero multiplier: the optimum is unique but the multipliers need not be,
    and the distance to it is then only bounded by the certificate)."""
    from scipy.optimize import minimize
    n, m = H.shape[0], len(h)
    res = minimize(lambda u: 0.5 * u @ H @ u + g @ u, np.zeros(n), jac=lambda u: H @ u + g, method="SLSQP",
                   constraints=[dict(type="ineq", fun=lambda u: h - G @ u, jac=lambda u: -G)], options=dict(ftol=1e-15, maxiter=500))
    u = res.x if np.all(np.isfinite(res.x)) else np.zeros(n)
    if zero_feasible:                                   # largest theta in [0, 1] with theta u feasible
        Gu = G @ u
        pos = Gu > h
        theta = min(1.0, float(np.min(h[pos] / Gu[pos]))) if pos.any() else 1.0
        u = max(theta, 0.0) * u
    scale = 1.0 + np.abs(g).max()
    tol_b = 1e-12 * (1.0 + np.abs(h).max())
    W = []
    for i in np.argsort(h - G @ u):                     # rows at their bound, a linearly independent subset
        if h[i] - G[i] @ u > tol_b:
            break
        if np.linalg.matrix_rank(G[W + [int(i)]]) == len(W) + 1:
            W.append(int(i))
    la = np.zeros(0)
    settled = True
    for _ in range(20 * m + 100):
        k = len(W)
        Gw = G[W]
        K = np.block([[H, Gw.T], [Gw, np.zeros((k, k))]])
        sol = np.linalg.lstsq(K, np.concatenate([-(H @ u + g), np.zeros(k)]), rcond=None)[0]
        p, la = sol[:n], sol[n:]
        if np.abs(p).max() <= 1e-11 * (1.0 + np.abs(u).max()):
            if k == 0 or la.min() >= -1e-12 * scale:
                break
            W.pop(int(np.argmin(la)))
            continue
        Gp = G @ p
        alpha, block = 1.0, -1
        tiny = 1e-12 * np.abs(p).max()
        for i in range(m):
            if i not in W and Gp[i] > tiny * np.abs(G[i]).sum():   # a row the step moves toward (hence independent of W)
                a = (h[i] - G[i] @ u) / Gp[i]
                if a < alpha:
                    alpha, block = max(a, 0.0), i
        u = u + alpha * p
        if block >= 0:
            W.append(block)
    else:
        settled = False                               # cycling among degenerate rows: flagged, the certificate decides
    # the final working set's KKT system once more, with its rows held at their bounds exactly (no drift from the steps)
    k = len(W)
    if k:
        K = np.block([[H, G[W].T], [G[W], np.zeros((k, k))]])
        sol = np.linalg.lstsq(K, np.concatenate([-g, h[W]]), rcond=None)[0]
        u, la = sol[:n], sol[n:]
    lam = np.zeros(m)
    lam[W] = np.maximum(la, 0.0)
    at_bound = h - G @ u <= 1e-9 * (1.0 + np.abs(h))
    degenerate = (not settled) or bool(np.any(at_bound & (lam <= 1e-9 * scale)))
    return u, lam, degenerate


def certificate(P, q, Aeq, beq, G, h, z, lam):
    """KKT residuals of (z, lam) on 1/2 z'Pz + q'z, Aeq z = beq, G z <= h: the equality multipliers are the least-squares fit of the
    stationarity equation (exact when Aeq has full row rank).  primal: max violation of the inequalities and equalities; dual: min lam;
    comp: max |lam_i (h_i - G_i z)|; stat: max |Pz + q + G'lam + Aeq'nu| / (1 + max |q|)."""
    grad = P @ z + q + G.T @ lam
    if Aeq is not None and len(Aeq):
        nu = np.linalg.lstsq(Aeq.T, -grad, rcond=None)[0]
        grad = grad + Aeq.T @ nu
        eq = float(np.abs(Aeq @ z - beq).max())
    else:
        eq = 0.0
    slack = h - G @ z
    return dict(primal=max(float(max(-slack.min(), 0.0)), eq), dual=float(lam.min()), comp=float(np.abs(lam * slack).max()),
                stat=float(np.abs(grad).max() / (1.0 + np.abs(q).max())))


def objective(d, z):
    return float(0.5 * z @ d["P"] @ z + d["q"] @ z + d["r"])


def solve_case(x0, ref, oa, od, p):
    """the reference's linear_mpc_control_kinematic, solved exactly: dict(u [T][2], xk [4][T+1], obj, lam (GPU row order), degenerate,
    steer, speed) or None when infeasible"""
    T = p["T"]
    if not feasible(x0, p):
        return None
    d = qp_data(x0, ref, oa, od, p)
    c = condense(d, T)
    u, lam, deg = exact_solve(c["H"], c["g"], c["G"], c["h"])
    z = c["Z"] @ u + c["z0"]
    return dict(u=u.reshape(T, 2), xk=z[:4 * (T + 1)].reshape(T + 1, 4).T, obj=objective(d, z), lam=lam, degenerate=deg,
                steer=u[1], speed=x0[2] + u[0] * p["DTK"], data=d, cond=c)


def nearest_index(px, py, cx, cy):
    """utils.nearest_point's index (the segment nearest to the point; ties to the first)"""
    P = np.column_stack([cx, cy])
    d = P[1:] - P[:-1]
    l2 = (d ** 2).sum(1)
    t = ((np.array([px, py]) - P[:-1]) * d).sum(1) / l2
    t = np.clip(t, 0.0, 1.0)
    proj = P[:-1] + t[:, None] * d
    dist = np.hypot(*(np.array([px, py]) - proj).T)
    return int(np.argmin(dist))


def ref_trajectory(state_xyvyaw, cx, cy, cyaw, sp, p, dlk=0.03):
    """calc_ref_trajectory_kinematic (:162-206), folding `cyaw` IN PLACE like the reference"""
    T = p["T"]
    x, y, v, yaw = state_xyvyaw
    ind = nearest_index(x, y, cx, cy)
    dind = abs(v) * p["DTK"] / dlk
    il = int(ind) + np.insert(np.cumsum(np.repeat(dind, T)), 0, 0).astype(int)
    il[il >= len(cx)] -= len(cx)
    m = cyaw - yaw > 4.5
    cyaw[m] = np.abs(cyaw[m] - (2 * np.pi))
    m = cyaw - yaw < -4.5
    cyaw[m] = np.abs(cyaw[m] + (2 * np.pi))
    return np.array([cx[il], cy[il], sp[il], cyaw[il]])
