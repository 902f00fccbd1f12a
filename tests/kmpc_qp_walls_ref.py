"""numpy restatement of the wall rows of f1p_kmpc_qp_walls_* (include/f1p.h) on top of tests/kmpc_qp_ref.py, tests/qp_avoid_ref.py
and tests/kmpc_qp_avoid_ref.py -- the yardstick of tests/test_kmpc_qp_walls_host.py and tests/test_gpu_kmpc_qp_walls.py.  A helper module, not
a conftest; pure numpy; nothing here is shared with the library's code.

A grid here is (cells u8 [h][w] with row index = gy, i.e. row 0 is the BOTTOM row of the map image, 1 = occupied; res; (ox, oy)): the ACTIVE
bitmap unpacked.  from_image() turns an image-ordered array (row 0 at the top, what Context.grid_debug_read returns) into it.

Per step t = 1..T and side sigma = +1 (left, slot 16) / -1 (right, slot 17): l = sigma (-sin psibar_t, cos psibar_t), the samples
q_k = pbar_t + ((double)k h) l for k = 1 .. n_samples with h = res / 2; k*: the first occupied one (outside the image or not finite:
occupied); the contact c = q_{k*-1} (q_0 = pbar_t), clear = (k* - 1) h, n = -l, the row -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - wall_margin.
Of the live discs (clear = dist - r) and the two wall candidates the two smallest clear are the step's rows, ties to the lower slot.
"""
import math

import numpy as np

import kmpc_qp_avoid_ref as A
import kmpc_qp_ref as Q
import qp_avoid_ref as R

SLOT_L, SLOT_R = 16, 17
DEFAULTS = dict(n_samples=48, wall_margin=0.0)
EDGE = 1e-9                        # a tested sample this close [cells] to a cell's edge: a last-ulp difference in sincos could move its cell


def from_image(cells_img):
    """image row order (row 0 at the top) -> gy order"""
    return np.ascontiguousarray(np.asarray(cells_img, dtype=np.uint8)[::-1])


def cell(grid, x, y):
    """f1p_set_grid's cell rule -> (gx, gy), or None outside the image / for a non-finite coordinate"""
    cells, res, (ox, oy) = grid
    inv = 1.0 / res
    u, v = (x - ox) * inv, (y - oy) * inv
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    fx, fy = math.floor(u), math.floor(v)
    if fx < 0 or fy < 0 or fx >= cells.shape[1] or fy >= cells.shape[0]:
        return None
    return int(fx), int(fy)


def occupied(grid, x, y):
    c = cell(grid, x, y)
    return True if c is None else bool(grid[0][c[1], c[0]])


def near_edge(grid, x, y):
    _, res, (ox, oy) = grid
    inv = 1.0 / res
    u, v = (x - ox) * inv, (y - oy) * inv
    if not (math.isfinite(u) and math.isfinite(v)):
        return False
    return abs(u - round(u)) <= EDGE or abs(v - round(v)) <= EDGE


def sample(grid, px, py, lx, ly, k):
    s = float(k) * (0.5 * grid[1])
    return px + s * lx, py + s * ly


def march(grid, px, py, lx, ly, n_samples):
    """-> (k* in 1 .. n_samples, 0: none; edge: a tested sample lies within EDGE of a cell edge)"""
    edge = False
    for k in range(1, n_samples + 1):
        qx, qy = sample(grid, px, py, lx, ly, k)
        edge |= near_edge(grid, qx, qy)
        if occupied(grid, qx, qy):
            return k, edge
    return 0, edge


def wall_candidates(grid, px, py, psi, n_samples):
    """-> ([(clear, slot, (cx, cy), (nx, ny)) of the sides that have a candidate, left first], edge)"""
    sn, cs = math.sin(psi), math.cos(psi)
    out, edge = [], False
    for slot, (lx, ly) in ((SLOT_L, (-sn, cs)), (SLOT_R, (sn, -cs))):
        k, e = march(grid, px, py, lx, ly, n_samples)
        edge |= e
        if k == 0:
            continue
        c = (px, py) if k == 1 else sample(grid, px, py, lx, ly, k - 1)
        out.append((float(k - 1) * (0.5 * grid[1]), slot, c, (-lx, -ly)))
    return out, edge


def planes(d, c, obs, grid, p, n_samples, margin=0.0, wall_margin=0.0):
    """-> (planes [T, 2, 4] = (n_x, n_y, right-hand side, slot; slot -1 and zeros: absent), A [2T, 2T]: the rows' u-coefficients, edge)"""
    T, dt = p["T"], p["DTK"]
    path, Z, z0 = d["path"], c["Z"], c["z0"]
    obs = np.zeros((0, 5)) if obs is None else np.asarray(obs, float).reshape(-1, 5)
    pl = np.zeros((T, 2, 4))
    pl[:, :, 3] = -1.0
    Am = np.zeros((2 * T, 2 * T))
    edge = False
    for t in range(1, T + 1):
        tau = float(t) * dt
        px, py, psi = path[0, t], path[1, t], path[3, t]
        cands = []                                               # (clear, slot, centre / contact, normal, what the right-hand side takes off)
        for m, (x, y, vx, vy, r) in enumerate(obs):
            if not r >= 0.0:
                continue
            cx, cy = x + vx * tau, y + vy * tau
            dx, dy = px - cx, py - cy
            dist = math.sqrt(dx * dx + dy * dy)
            n = (-math.cos(psi), -math.sin(psi)) if dist < 1e-9 else (dx / dist, dy / dist)
            cands.append((dist - r, m, (cx, cy), n, r + margin))
        walls, e = wall_candidates(grid, px, py, psi, n_samples)
        edge |= e
        cands += [(cl, slot, cc, n, wall_margin) for cl, slot, cc, n in walls]
        cands.sort(key=lambda q: (q[0], q[1]))
        for k, (cl, slot, (cx, cy), (nx_, ny_), off) in enumerate(cands[:2]):
            rhs = nx_ * (z0[4 * t] - cx) + ny_ * (z0[4 * t + 1] - cy) - off
            pl[t - 1, k] = (nx_, ny_, rhs, slot)
            Am[2 * (t - 1) + k] = -(nx_ * Z[4 * t] + ny_ * Z[4 * t + 1])
    return pl, Am, edge


def build(x0, ref, oa, od, obs, grid, p, n_samples, margin=0.0, rho=1e4, lin=10.0, wall_margin=0.0):
    """qp_avoid_ref.build on the rows above; the dict gains `edge`"""
    d = Q.qp_data(x0, ref, oa, od, p)
    c = Q.condense(d, p["T"])
    pl, Am, edge = planes(d, c, obs, grid, p, n_samples, margin, wall_margin)
    b = R.build(d, c, pl, Am, p["T"], rho, lin)
    b["edge"] = edge
    return b


cert, cert_ok, lam_full = A.cert, A.cert_ok, A.lam_full


def solve_built(b, x0, p):
    """kmpc_qp_avoid_ref.solve's shift, scale and polish around kmpc_qp_ref.exact_solve, on a built problem"""
    T, rho = p["T"], b["rho"]
    n = 2 * T
    ha = b["h"][b["m0"]:-1]
    eps0 = max(0.0, -float(ha.min()) if len(ha) else 0.0) + 1.0
    w0 = np.zeros(n + 1); w0[n] = eps0
    D = np.ones(n + 1); D[n] = 1.0 / math.sqrt(2.0 * rho)
    Hs, gs, Gs, hs = D[:, None] * b["H"] * D[None, :], D * (b["g"] + b["H"] @ w0), b["G"] * D[None, :], b["h"] - b["G"] @ w0
    ws, lam, deg = Q.exact_solve(Hs, gs, Gs, hs)
    ws, lam = A._polish(Hs, gs, Gs, hs, ws, lam)
    w = D * ws + w0
    al = np.zeros(n + 1)
    al[b["rows"]] = lam[b["m0"]:-1]
    al[n] = lam[-1]
    return dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=deg, planes=b["planes"], cert=cert(b, w, lam),
                steer=float(w[1]), speed=float(x0[2] + w[0] * p["DTK"]), build=b, edge=b["edge"])


def solve(x0, ref, oa, od, obs, grid, p, n_samples, margin=0.0, rho=1e4, lin=10.0, wall_margin=0.0):
    """exact optimum of the wall problem, kmpc_qp_avoid_ref.solve's dict (+ edge), or None when infeasible (v0 outside its bounds) or an
    input is not finite"""
    if not np.isfinite(np.asarray(x0, float)).all() or not Q.feasible(x0, p):
        return None
    return solve_built(build(x0, ref, oa, od, obs, grid, p, n_samples, margin, rho, lin, wall_margin), x0, p)


def brute_first_hit(grid, px, py, lx, ly, n_samples):
    """the march by a scan of the whole grid: every sample's cell looked up in the list of occupied cells' (gx, gy) -> k* (0: none)"""
    cells, res, (ox, oy) = grid
    occ = {(int(gx), int(gy)) for gy, gx in zip(*np.nonzero(cells))}
    for k in range(1, n_samples + 1):
        s = float(k) * (0.5 * res)
        x, y = px + s * lx, py + s * ly
        u, v = (x - ox) * (1.0 / res), (y - oy) * (1.0 / res)
        inside = math.isfinite(u) and math.isfinite(v) and 0.0 <= u < cells.shape[1] and 0.0 <= v < cells.shape[0]
        if not inside or (int(u), int(v)) in occ:
            return k
    return 0
