"""numpy restatement of the reference's linearised dynamic single-track MPC QP (control/dynamic_mpc/dynamic_mpc.py:279-710, :995-1117) --
the yardstick of f1p_stmpc_qp_* (tests/test_stmpc_qp_host.py, tests/test_gpu_stmpc_qp.py).  A helper module, not a conftest.

  * predict_motion() / update_state() / model():  :279-300, :317-404, :428-535, in the reference's operation order
  * qp_data():     the problem as cvxpy would canonicalise it over z = [vec(x); vec(u)] (column-major, x_t at 7 t + k, u_t at 7 (T+1) + 2 t + j):
                   1/2 z'Pz + q'z + r,  Aeq z = beq,  G z <= h, rows in the order the reference lists its constraints
                   (tools/gen_golden_stmpc_qp.py records the same data from the reference's own code: tests/golden/g17_stmpc_qp.npz)
  * condense():    the states eliminated: 1/2 u'Hu + g'u + c over u = vec(u), n = 2T, inequality rows in f1p_stmpc_qp_batch's dual order
  * solve_case():  the exact optimum (exact(): an active-set polish that must pass the certificate, else kmpc_qp_ref.exact_solve)
                   and the output map
  * plan_step():   STMPCPlanner.plan with the QP solver on the host: the branch, the warm-start rules, both branches' exact solutions
"""
import math

import numpy as np

import kmpc_qp_ref as KQ
from kmpc_qp_ref import certificate, exact_solve  # noqa: F401  (re-exported for the tests)

PARAMS = np.array([3.74, 0.15875, 0.17145, 0.074, 4.718, 5.4562, 0.04712, 1.0489])


def default_params(T=40):
    return dict(T=T, DT=0.025, WB=0.33, MAX_STEER=0.4189, MAX_STEER_V=3.2, MAX_SPEED=6.0, MIN_SPEED=0.0, MAX_ACCEL=3.0,
                R=np.diag([0.5, 0.01]), Rd=np.diag([0.3, 0.01]), Q=np.diag([32.0, 32.0, 0.0, 1.0, 0.5, 0.0, 0.0]),
                Qf=np.diag([32.0, 32.0, 0.0, 1.0, 0.5, 0.0, 0.0]), vp=PARAMS.copy())


def kin_params(TK=8):
    """STMPCPlanner's kinematic branch: its mpc_config's TK, DTK, Rk, Rdk, Qk, Qfk (:40-86) -- the kinematic planner's QP (:712-833)"""
    return KQ.default_params(TK)


def _consts(vp, a):
    mass, l_f, l_r, h_CoG, c_f, c_r, Iz, mu = (float(x) for x in vp)
    g = 9.81
    K = (mu * mass) / ((l_f + l_r) * Iz)
    T = (g * l_r) - (a * h_CoG)
    V = (g * l_f) + (a * h_CoG)
    F = l_f * c_f
    R = l_r * c_r
    M = (mu * c_f) / (l_f + l_r)
    N = (mu * c_r) / (l_f + l_r)
    A1 = K * F * T
    A2 = K * (R * V - F * T)
    A3 = K * (l_f * l_f * c_f * T + l_r * l_r * c_r * V)
    A4 = M * T
    A5 = N * V + M * T
    A6 = N * V * l_r - M * T * l_f
    return dict(K=K, F=F, R=R, M=M, N=N, A1=A1, A2=A2, A3=A3, A4=A4, A5=A5, A6=A6, l_f=l_f, l_r=l_r, c_f=c_f, c_r=c_r, h=h_CoG)


def update_state(s, a, delta_v, p):
    """update_state :317-404 on s = [x, y, delta, v, yaw, yawrate, beta] (a new array)"""
    x, y, delta, v, yaw, yr, beta = (float(z) for z in s)
    a, delta_v = float(a), float(delta_v)
    if delta_v >= p["MAX_STEER_V"]:
        delta_v = p["MAX_STEER_V"]
    elif delta_v <= -p["MAX_STEER_V"]:
        delta_v = -p["MAX_STEER_V"]
    if a >= p["MAX_ACCEL"]:
        a = p["MAX_ACCEL"]
    elif a <= -p["MAX_ACCEL"]:
        a = -p["MAX_ACCEL"]
    k = _consts(p["vp"], a)
    DT = p["DT"]
    x_new = x + v * math.cos(yaw + beta) * DT
    y_new = y + v * math.sin(yaw + beta) * DT
    delta_new = delta + delta_v * DT
    v_new = v + a * DT
    yaw_new = yaw + v / p["WB"] * math.tan(delta) * DT
    yr_new = yr + (k["A1"] * delta + k["A2"] * beta - k["A3"] * (yr / v)) * DT
    beta_new = beta + (k["A4"] * (delta / v) - k["A5"] * (beta / v) + k["A6"] * (yr / (v * v)) - yr) * DT
    if v_new > p["MAX_SPEED"]:
        v_new = p["MAX_SPEED"]
    elif v_new < p["MIN_SPEED"]:
        v_new = p["MIN_SPEED"]
    if delta_new >= p["MAX_STEER"]:
        delta_new = p["MAX_STEER"]
    elif delta_new <= -p["MAX_STEER"]:
        delta_new = -p["MAX_STEER"]
    return np.array([x_new, y_new, delta_new, v_new, yaw_new, yr_new, beta_new])


def predict_motion(x0, oa, odv, p):
    """predict_motion :279-300: [7][T+1] (zip over the first T entries of oa / od_v)"""
    T = p["T"]
    path = np.zeros((7, T + 1))
    path[:, 0] = x0
    s = np.asarray(x0, float)
    for t in range(T):
        s = update_state(s, oa[t], odv[t], p)
        path[:, t + 1] = s
    return path


def model(delta, v, yaw, yr, beta, a, p):
    """get_dynamic_model_matrix :428-535"""
    k = _consts(p["vp"], float(a))
    DT, h = p["DT"], k["h"]
    K, F, R, M, N, l_f, l_r, c_f, c_r = (k[n] for n in ("K", "F", "R", "M", "N", "l_f", "l_r", "c_f", "c_r"))
    A1, A2, A3, A4, A5, A6 = (k[n] for n in ("A1", "A2", "A3", "A4", "A5", "A6"))
    B1 = (-h * F * K) * delta + (h * K * (F + R)) * beta - (h * K * ((l_r * l_r * c_r) - (l_f * l_f * c_f))) * (yr / v)
    B2 = (-h * M) * (delta / v) - h * (N - M) * (beta / v) + h * (l_f * M + l_r * N) * (yr / (v * v))
    A = np.zeros((7, 7))
    A[0, 0] = A[1, 1] = A[2, 2] = A[3, 3] = A[4, 4] = 1.0
    A[5, 5] = -DT * (A3 / v) + 1
    A[6, 6] = -DT * A5 + 1
    A[0, 3] = DT * math.cos(yaw + beta)
    A[0, 4] = -DT * v * math.sin(yaw + beta)
    A[0, 6] = -DT * v * math.sin(yaw + beta)
    A[1, 3] = DT * math.sin(yaw + beta)
    A[1, 4] = DT * v * math.cos(yaw + beta)
    A[1, 6] = DT * v * math.cos(yaw + beta)
    A[4, 5] = DT
    A[5, 2] = DT * A1
    A[5, 3] = DT * A3 * (yr / (v * v))
    A[5, 6] = DT * A2
    A[6, 2] = DT * (A4 / v)
    A[6, 3] = DT * (-A4 * beta * v + A5 * beta * v - A6 * 2 * yr) / (v * v * v)
    A[6, 5] = DT * ((A6 / (v * v)) - 1)
    B = np.zeros((7, 2))
    B[2, 0] = DT
    B[3, 1] = DT
    B[5, 1] = DT * B1
    B[6, 1] = DT * B2
    C = np.zeros(7)
    C[0] = DT * (v * math.sin(yaw + beta) * yaw + v * math.sin(yaw + beta) * beta)
    C[1] = DT * (-v * math.cos(yaw + beta) * yaw - v * math.cos(yaw + beta) * beta)
    C[5] = DT * (-A3 * (yr / v) - B1 * a)
    C[6] = DT * (((A4 * delta * v - A5 * beta * v + A6 * 2 * yr) / (v * v)) - B2 * a)
    return A, B, C


def qp_data(x0, ref, oa, odv, p):
    """The QP of mpc_prob_init / mpc_prob_solve (:575-948) at the linearisation point of linear_mpc_control (:995-1040): oa / od_v the
    previous solution, NOT shifted; None = zeros.  Built like cvxpy canonicalises it (the recording stand-in's arithmetic)."""
    T = p["T"]
    oa = np.zeros(T) if oa is None else np.asarray(oa, float)
    odv = np.zeros(T) if odv is None else np.asarray(odv, float)
    ref = np.asarray(ref, float)
    x0 = np.asarray(x0, float)
    NX, NU = 7 * (T + 1), 2 * T
    nz = NX + NU
    X = lambda t, k: 7 * t + k            # noqa: E731
    U = lambda t, j: NX + 2 * t + j       # noqa: E731
    P = np.zeros((nz, nz)); q = np.zeros(nz); r = 0.0
    Eu = np.zeros((NU, nz)); Eu[np.arange(NU), NX + np.arange(NU)] = 1.0
    Ex = np.zeros((NX, nz)); Ex[np.arange(NX), np.arange(NX)] = 1.0
    r = KQ._quad(P, q, r, Eu, np.zeros(NU), np.kron(np.eye(T), p["R"]))                       # :616
    Qb = np.zeros((NX, NX))
    for t in range(T + 1):
        Qb[7 * t:7 * t + 7, 7 * t:7 * t + 7] = p["Qf"] if t == T else p["Q"]
    r = KQ._quad(P, q, r, Ex, -ref.reshape(-1, order="F"), Qb)                                # :619
    D = np.zeros((2 * (T - 1), nz))
    for t in range(T - 1):
        for j in range(2):
            D[2 * t + j, U(t + 1, j)] = 1.0
            D[2 * t + j, U(t, j)] = -1.0
    r = KQ._quad(P, q, r, D, np.zeros(2 * (T - 1)), np.kron(np.eye(T - 1), p["Rd"]))          # :622
    path = predict_motion(x0, oa, odv, p)
    Aeq = np.zeros((7 * T + 7, nz)); beq = np.zeros(7 * T + 7)
    for t in range(T):                                                                           # :677-683
        A, B, C = model(path[2, t], path[3, t], path[4, t], path[5, t], path[6, t], oa[t], p)
        for k in range(7):
            row = 7 * t + k
            Aeq[row, X(t + 1, k)] = 1.0
            Aeq[row, [X(t, i) for i in range(7)]] -= A[k]
            Aeq[row, [U(t, j) for j in range(2)]] -= B[k]
            beq[row] = C[k]
    for k in range(7):                                                                           # :688
        Aeq[7 * T + k, X(0, k)] = 1.0
        beq[7 * T + k] = x0[k]
    rows, h = [], []

    def add(coef, bound):
        rows.append(coef); h.append(bound)

    for sgn in (1.0, -1.0):                                                                      # :685 |diff(u0)| <= MAX_STEER_V
        for t in range(T - 1):
            c = np.zeros(nz); c[U(t + 1, 0)] = sgn; c[U(t, 0)] = -sgn
            add(c, p["MAX_STEER_V"])
    for k, sgn, bound in ((2, 1.0, p["MAX_STEER"]), (2, -1.0, p["MAX_STEER"]), (3, 1.0, p["MAX_SPEED"]), (3, -1.0, -p["MIN_SPEED"])):
        for t in range(T + 1):                                                                   # :689-700
            c = np.zeros(nz); c[X(t, k)] = sgn; add(c, bound)
    for j, bound in ((0, p["MAX_STEER_V"]), (1, p["MAX_ACCEL"])):                                # :701-706
        for sgn in (1.0, -1.0):
            for t in range(T):
                c = np.zeros(nz); c[U(t, j)] = sgn; add(c, bound)
    return dict(P=P, q=q, r=r, Aeq=Aeq, beq=beq, G=np.array(rows), h=np.array(h), path=path)


def gpu_rows(T):
    """index into qp_data's G rows of each dual of f1p_stmpc_qp_batch: rate upper, lower (T-1 each), delta_1..T upper, lower,
    v_1..T upper, lower, u0 upper, lower, u1 upper, lower (T each); the t = 0 delta / v rows have no dual there (x_0 is fixed)"""
    b = 2 * (T - 1)
    idx = list(range(0, 2 * (T - 1)))
    for blk in range(4):                                         # delta upper, delta lower, v upper, v lower: t = 1..T
        idx += [b + blk * (T + 1) + t for t in range(1, T + 1)]
    b0 = b + 4 * (T + 1)
    idx += list(range(b0, b0 + 4 * T))
    return np.array(idx)


def condense(d, T):
    """eliminate the states: z = Z u + z0 -> H, g, c, Gc, hc (GPU row order), Z, z0"""
    NX, NU = 7 * (T + 1), 2 * T
    from scipy.linalg import solve_triangular
    perm = np.r_[7 * T:7 * T + 7, 0:7 * T]               # the x_0 rows first: Ax is then unit lower triangular
    Ax, Au, b = d["Aeq"][perm, :NX], d["Aeq"][perm, NX:], d["beq"][perm]
    Sx = solve_triangular(Ax, -Au, lower=True, unit_diagonal=True)
    sx = solve_triangular(Ax, b, lower=True, unit_diagonal=True)
    Z = np.vstack([Sx, np.eye(NU)]); z0 = np.concatenate([sx, np.zeros(NU)])
    P, q = d["P"], d["q"]
    H = Z.T @ P @ Z
    g = Z.T @ (P @ z0 + q)
    c = 0.5 * z0 @ P @ z0 + q @ z0 + d["r"]
    idx = gpu_rows(T)
    G, h = d["G"][idx], d["h"][idx]
    return dict(H=0.5 * (H + H.T), g=g, c=c, G=G @ Z, h=h - G @ z0, Z=Z, z0=z0)


def feasible(x0, p):
    return abs(x0[2]) <= p["MAX_STEER"] and p["MIN_SPEED"] <= x0[3] <= p["MAX_SPEED"]


def objective(d, z):
    return float(0.5 * z @ d["P"] @ z + d["q"] @ z + d["r"])


def solve_case(x0, ref, oa, odv, p):
    """linear_mpc_control solved exactly: dict(u [T][2], x [7][T+1], obj, lam (GPU row order), degenerate, steer, speed, data, cond),
    or None when infeasible or the model is not finite"""
    T = p["T"]
    x0 = np.asarray(x0, float)
    if not feasible(x0, p):
        return None
    with np.errstate(all="ignore"):
        try:
            d = qp_data(x0, ref, oa, odv, p)
        except ZeroDivisionError:
            return None
    if not all(np.isfinite(d[m]).all() for m in ("Aeq", "beq")):
        return None
    c = condense(d, T)
    u, lam, deg = exact(c)
    z = c["Z"] @ u + c["z0"]
    return dict(u=u.reshape(T, 2), x=z[:7 * (T + 1)].reshape(T + 1, 7).T, obj=objective(d, z), lam=lam, degenerate=deg,
                steer=x0[2] + u[0] * p["DT"], speed=x0[3] + u[1] * p["DT"], data=d, cond=c)


def cond_cert(c, u, lam):
    grad = c["H"] @ u + c["g"] + c["G"].T @ lam
    sl = c["h"] - c["G"] @ u
    return dict(primal=float(max(0.0, -sl.min())), dual=float(lam.min()), comp=float(np.abs(lam * sl).max()),
                stat=float(np.abs(grad).max() / (1.0 + np.abs(c["g"]).max())))


def cert_ok(cert):
    return cert["primal"] <= 1e-9 and cert["dual"] >= -1e-10 and cert["comp"] <= 1e-9 and cert["stat"] <= 1e-8


def exact_ok(c, u, lam):
    """cert_ok with the complementarity relative to the multipliers' scale: an exact vertex's slacks are ~1e-12 (rounding in h - G u), and
    the dynamic problem's multipliers reach ~1e3"""
    cert = cond_cert(c, u, lam)
    cert["comp"] /= 1.0 + lam.max()
    return cert_ok(cert)


def plan_step(state, warm, ref_dyn, ref_kin, p, pk, v_ks=2.0):
    """STMPCPlanner.plan with the QP solver (:133-191) on the host.  warm = (oa, od_v) or None (the reference's self.oa / self.odelta_v);
    ref_dyn [7][T+1] / ref_kin [4][TK+1] the branch's reference.  Returns (steer, speed, new warm, branch, degenerate) -- the new warm
    None when the solve fails (steer / speed NaN)."""
    s = np.asarray(state, float)
    if s[3] <= v_ks:                                             # kinematic branch (:168-180); reset when len(oa) > TK (:1052)
        TK = pk["T"]
        oa, od = (None, None) if warm is None or len(warm[0]) > TK else warm
        sol = KQ.solve_case(np.array([s[0], s[1], s[3], s[4]]), ref_kin, oa, od, pk)
        if sol is None:
            return np.nan, np.nan, None, 0, False
        return sol["steer"], sol["speed"], (sol["u"][:, 0].copy(), sol["u"][:, 1].copy()), 0, sol["degenerate"]
    T = p["T"]                                                   # dynamic branch (:181-191); reset when len(oa) < T (:1005)
    oa, odv = (None, None) if warm is None or len(warm[0]) < T else (warm[0][:T], warm[1][:T])
    sol = solve_case(s, ref_dyn, oa, odv, p)
    if sol is None:
        return np.nan, np.nan, None, 1, False
    return sol["steer"], sol["speed"], (sol["u"][:, 1].copy(), sol["u"][:, 0].copy()), 1, sol["degenerate"]


def plant(state, steer, speed, p):
    """the closed loop's vehicle: update_state with a = (speed - v) / DT and steering speed (steer - delta) / DT"""
    s = np.asarray(state, float)
    return update_state(s, (speed - s[3]) / p["DT"], (steer - s[2]) / p["DT"], p)


def fast_condense(x0, ref, oa, odv, p):
    """condense() built directly from the model (no full-space matrices): H, g, c, G, h in the GPU's row order -- for many egos"""
    T = p["T"]
    n = 2 * T
    x0 = np.asarray(x0, float)
    oa = np.zeros(T) if oa is None else np.asarray(oa, float)
    odv = np.zeros(T) if odv is None else np.asarray(odv, float)
    path = predict_motion(x0, oa, odv, p)
    S = np.zeros((7, n)); s = x0.copy()
    H = np.zeros((n, n)); g = np.zeros(n)
    c = float((x0 - ref[:, 0]) @ p["Q"] @ (x0 - ref[:, 0]))
    for t in range(T):
        A, B, C = model(path[2, t], path[3, t], path[4, t], path[5, t], path[6, t], oa[t], p)
        S = A @ S
        S[:, 2 * t:2 * t + 2] = B
        s = A @ s + C
        W = p["Qf"] if t == T - 1 else p["Q"]
        e = s - ref[:, t + 1]
        H += 2.0 * S.T @ W @ S
        g += 2.0 * S.T @ (W @ e)
        c += float(e @ W @ e)
    H += 2.0 * np.kron(np.eye(T), p["R"])
    Dm = np.zeros((2 * (T - 1), n))
    for t in range(T - 1):
        for j in range(2):
            Dm[2 * t + j, 2 * (t + 1) + j] = 1.0
            Dm[2 * t + j, 2 * t + j] = -1.0
    H += 2.0 * Dm.T @ np.kron(np.eye(T - 1), p["Rd"]) @ Dm
    DT = p["DT"]
    E0, E1 = np.zeros((T, n)), np.zeros((T, n))
    E0[np.arange(T), 2 * np.arange(T)] = 1.0
    E1[np.arange(T), 2 * np.arange(T) + 1] = 1.0
    rate = E0[1:] - E0[:-1]
    L = np.tril(np.ones((T, T)))
    pre0, pre1 = DT * (L @ E0), DT * (L @ E1)
    d0, v0 = x0[2], x0[3]
    G = np.vstack([rate, -rate, pre0, -pre0, pre1, -pre1, E0, -E0, E1, -E1])
    h = np.concatenate([np.full(2 * (T - 1), p["MAX_STEER_V"]), np.full(T, p["MAX_STEER"] - d0), np.full(T, p["MAX_STEER"] + d0),
                        np.full(T, p["MAX_SPEED"] - v0), np.full(T, v0 - p["MIN_SPEED"]), np.full(2 * T, p["MAX_STEER_V"]),
                        np.full(2 * T, p["MAX_ACCEL"])])
    return dict(H=0.5 * (H + H.T), g=g, c=c, G=G, h=h)


def polish(c, lam_hint):
    """the exact optimum from a guess of the active set (rows with lam_hint > 0): the equality-constrained KKT system of those rows,
    solved exactly; None unless (u, lam) passes the certificate (the optimum of a strictly convex QP is unique, so a passing point IS
    the exact optimum, whatever produced the guess).  Returns u, lam, degenerate."""
    H, g, G, h = c["H"], c["g"], c["G"], c["h"]
    n = H.shape[0]
    W = list(np.flatnonzero(lam_hint > 1e-12 * (1.0 + np.abs(g).max())))
    for _ in range(8):
        k = len(W)
        K = np.block([[H, G[W].T], [G[W], np.zeros((k, k))]])
        sol = np.linalg.lstsq(K, np.concatenate([-g, h[W]]), rcond=None)[0]
        u, la = sol[:n], sol[n:]
        if k and la.min() < 0:                           # dependent active rows: the multipliers are not unique, take nonnegative ones
            from scipy.optimize import nnls
            la = nnls(G[W].T, -(H @ u + g))[0]
        lam = np.zeros(len(h)); lam[W] = la
        if exact_ok(c, u, lam):
            at_bound = h - G @ u <= 1e-9 * (1.0 + np.abs(h))
            return u, lam, bool(np.any(at_bound & (lam <= 1e-9 * (1.0 + np.abs(g).max()))))
        viol = np.flatnonzero(G @ u - h > 1e-12 * (1.0 + np.abs(h)))              # rows the guess left out, then rows pulling the wrong way
        W = sorted(set(w for w, l in zip(W, la) if l > 0) | set(viol.tolist()))
    return None


def ipm_hint(c, iters=80):
    """a plain dense primal-dual interior point (Mehrotra) in numpy: only a GUESS of the active set for polish(), which decides"""
    H, g, G, h = c["H"], c["g"], c["G"], c["h"]
    m = len(h)
    u = np.zeros(H.shape[0]); s = np.maximum(h, 1.0); lam = np.ones(m)
    for _ in range(iters):
        rd = H @ u + g + G.T @ lam
        rp = G @ u + s - h
        mu = s @ lam / m
        if max(np.abs(rd).max(), np.abs(rp).max()) < 1e-12 and mu < 1e-14:
            break
        try:
            L = np.linalg.cholesky(H + G.T @ ((lam / s)[:, None] * G))
        except np.linalg.LinAlgError:                    # lambda / s ~ 1e16 on the active rows: the guess is as good as it gets
            break

        def newton(rc):
            rhs = -rd - G.T @ ((lam * rp - rc) / s)
            du = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            ds = -rp - G @ du
            return du, ds, (-rc - lam * ds) / s

        def amax(ds, dl):
            a = 1.0
            if (ds < 0).any():
                a = min(a, float(np.min(-s[ds < 0] / ds[ds < 0])))
            if (dl < 0).any():
                a = min(a, float(np.min(-lam[dl < 0] / dl[dl < 0])))
            return a
        du, ds, dl = newton(s * lam)
        a = amax(ds, dl)
        sigma = (((s + a * ds) @ (lam + a * dl)) / (s @ lam)) ** 3
        du, ds, dl = newton(s * lam + ds * dl - sigma * mu)
        a = min(1.0, 0.99 * amax(ds, dl))
        u, s, lam = u + a * du, s + a * ds, lam + a * dl
    return lam


def exact(c, lam_hint=None):
    """polish() from the hint (default: ipm_hint's) when it certifies, else exact_solve(): (u, lam, degenerate)"""
    try:
        r = polish(c, ipm_hint(c) if lam_hint is None else lam_hint)
    except np.linalg.LinAlgError:
        r = None
    if r is not None:
        return r
    return exact_solve(c["H"], c["g"], c["G"], c["h"])
