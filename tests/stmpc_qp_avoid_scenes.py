"""The scenes of the dynamic QP's avoidance-row tests (tests/test_stmpc_qp_avoid_host.py, tests/test_gpu_stmpc_qp_avoid.py), built and solved
on the CPU with tests/stmpc_qp_avoid_ref.py: batches of dynamic-branch states (v > V_KS) along levine with a non-zero previous solution,
whose discs cover every family of rows.  A helper module, not a conftest; nothing here touches a GPU."""
import functools
import math
import os

import numpy as np

import kmpc_qp_ref as KQ
import stmpc_qp_avoid_ref as A
import stmpc_qp_ref as SQ
import tracker_ref as TR
from f1tenth_planning_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE = "g22_stmpc_qp_avoid.npz"       # tools/gen_golden_stmpc_qp_avoid.py: solve_scene() of every shape
EPS_MAX = 0.05                               # every scene's slack stays below this [m]: squeezed egos (decimetres) are not these tests' matter


def levine():
    lev = np.load(os.path.join(GOLDEN, "tracks.npz"), allow_pickle=False)["levine"]
    return tuple(np.ascontiguousarray(lev[:, c]) for c in (1, 2, 3, 5))          # cx, cy, cyaw, sp


def lds_bytes(T):
    """the avoidance variant's LDS per ego at horizon T, from the library's own layout function"""
    return int(_abi.load_library().f1p_stmpc_qp_avoid_lds_bytes(T))


@functools.lru_cache(maxsize=None)
def opt_in_horizon():
    """the last horizon whose layout stays within 64 KiB (the kernel runs without the opt-in); the next one takes the other launch path"""
    T = 2
    while lds_bytes(T + 1) <= 64 * 1024:
        T += 1
    return T


CAP = _abi.STMPC_QP_AVOID_MAX_T
FAMILIES = ("no_live", "inactive", "active", "inside", "on_pbar", "selection", "empty_between", "nan_live", "v0_out", "near")
HORIZONS = (2, 10, opt_in_horizon(), opt_in_horizon() + 1, CAP)
# (T, M, margin): every horizon x M at margin 0, and one batch with a margin: there the family "near" (discs whose edge is 0.01 m beside the
# plain optimum's trajectory: rows that only the margin of 0.015 m makes bind) is the margin's own.  (A larger margin would push the slack
# of "inside" and "on_pbar", which no input can help, past EPS_MAX.)
SHAPES = tuple((T, M, 0.0) for T in HORIZONS for M in (1, 4, 16)) + ((10, 4, 0.015),)


def n_egos(T):
    return 16 if T == CAP else 32


def family(e):
    """ego e belongs to family e % 10, its variant within the family is j = e // 10"""
    return FAMILIES[e % len(FAMILIES)], e // len(FAMILIES)


def _beside(path, t, lat, r, v=(0.0, 0.0), DT=0.025):
    """a disc row whose centre is `lat` metres left of the path's point at step t (seen along the direction of travel yaw + beta) WHEN the
    ego gets there (it moves at v until then)"""
    x, y, hd = path[0, t], path[1, t], path[4, t] + path[6, t]
    cx, cy = x - lat * math.sin(hd), y + lat * math.cos(hd)
    tau = float(t) * DT
    return [cx - v[0] * tau, cy - v[1] * tau, v[0], v[1], r]


def _base(T):
    """states along levine above V_KS, their references, and a small random control sequence"""
    E = n_egos(T)
    cx, cy, cyaw, sp = levine()
    rng = np.random.default_rng(1000 * T)
    # on the straights: no corner within 5.5 m (a second at MAX-ish speed), where the plain optimum brakes to ~0.4 m/s within the horizon and
    # the linearised model (terms in 1 / v) is no longer a problem any solver settles -- not what the avoidance rows are about
    ahead = int(5.5 / float(np.hypot(cx[1] - cx[0], cy[1] - cy[0])))
    turn = np.array([np.abs(np.angle(np.exp(1j * (cyaw[q:q + ahead] - cyaw[q])))).max() for q in range(len(cx) - ahead)])
    straight = np.flatnonzero(turn < 0.1)
    k = straight[(np.arange(E) * len(straight)) // E]
    v = rng.uniform(2.5, 5.0, E)
    yaw = cyaw[k] + rng.normal(0.0, 0.05, E)
    lat = rng.normal(0.0, 0.05, E)
    x0 = np.column_stack([cx[k] - lat * np.sin(cyaw[k]), cy[k] + lat * np.cos(cyaw[k]), rng.normal(0.0, 0.03, E), v, yaw, rng.normal(0.0, 0.1, E),
                          rng.normal(0.0, 0.01, E)])
    oa = rng.normal(0.0, 0.5, (E, T)).clip(-3.0, 3.0)
    odv = rng.normal(0.0, 0.1, (E, T)).clip(-3.2, 3.2)
    ref = np.array([TR.stmpc_ref_ref(KQ.nearest_index(s[0], s[1], cx, cy), s[[0, 1, 3, 4]], cx, cy, cyaw, sp, T) for s in x0])
    return x0, ref, oa, odv


PREV = {}            # T -> (oa, odv): set by tools/gen_golden_stmpc_qp_avoid.py while it writes the file the tests read them from


def compute_prev(T):
    """the scenes' previous solution (oa, odv) [E, T]: the plain QP's optimum from _base's random sequence, plus a little noise -- what a
    warm-started planner holds: the linearisation path then runs within centimetres of the next optimum's trajectory, so a disc placed
    beside one step of it is not cut by the half-planes of the steps around it.  Recorded in the golden file (it costs a solve per ego)."""
    x0, ref, oa0, odv0 = _base(T)
    p = SQ.default_params(T)
    rng = np.random.default_rng(7000 * T)
    oa, odv = np.empty_like(oa0), np.empty_like(odv0)
    for e in range(len(x0)):
        u = SQ.solve_case(x0[e], ref[e], oa0[e], odv0[e], p)["u"]
        oa[e] = (u[:, 1] + rng.normal(0.0, 0.02, T)).clip(-3.0, 3.0)
        odv[e] = (u[:, 0] + rng.normal(0.0, 0.01, T)).clip(-3.2, 3.2)
    return oa, odv


@functools.lru_cache(maxsize=None)
def exact_scene(T, M):
    """-> x0 [E, 7], ref [E, 7, T+1], oa, odv [E, T] (a non-zero previous solution), obs [E, M, 5], fam {family: egos}.  What a family promises
    is asserted from the yardstick's output (assert_families), not assumed."""
    E = n_egos(T)
    p = SQ.default_params(T)
    x0, ref, _, _ = _base(T)                                     # (the states and the previous solution are the horizon's, whatever M)
    if T in PREV:
        oa, odv = PREV[T]
    else:
        g = np.load(os.path.join(GOLDEN, GOLDEN_FILE), allow_pickle=False)
        oa, odv = g[f"T{T}_prev_oa"].copy(), g[f"T{T}_prev_odv"].copy()
    obs = np.zeros((E, M, 5))
    obs[:, :, 4] = -1.0
    fam = {f: [] for f in FAMILIES}
    tm = max(1, T // 2)                                          # a step in the middle of the horizon
    for e in range(E):
        f, j = family(e)
        path = SQ.predict_motion(x0[e], oa[e], odv[e], p)
        hd0 = x0[e, 4] + x0[e, 6]
        fam[f].append(e)
        if f == "no_live":                                       # empty slots of every kind: r < 0, r NaN, NaN coordinates beside them
            obs[e, :, 4] = [-1.0, np.nan, -0.5][j % 3]
            if j >= 2:
                obs[e, :, :4] = np.nan
        elif f == "inactive":                                    # far beside the path
            for m in range(min(M, 1 + j % 3)):
                obs[e, m] = _beside(path, min(T, 1 + m), 4.0 + j, 0.45)
        elif f == "active":                                      # the disc's edge 0.02 .. 0.16 mm over the plain QP's own trajectory: a small
            t = min(T, max(2, tm + j % 3))                       # push, so the multipliers stay below lin and eps at 0; j >= 2: a moving disc
            xs = SQ.solve_case(x0[e], ref[e], oa[e], odv[e], p)["x"]
            vv = (0.3 * math.cos(hd0), 0.3 * math.sin(hd0)) if j >= 2 else (0.0, 0.0)
            at = path.copy(); at[:2] = xs[:2]
            o = _beside(at, t, (-1.0 if j % 2 else 1.0) * 0.40, 0.40, vv)
            if T == 2:                                           # no input moves p_2 sideways (only a_0 moves it, along the path): the disc is ahead
                hd = path[4, t] + path[6, t]
                o[0] = xs[0, t] + 0.40 * math.cos(hd) - vv[0] * float(t) * p["DT"]
                o[1] = xs[1, t] + 0.40 * math.sin(hd) - vv[1] * float(t) * p["DT"]
            c = np.array([o[0] + o[2] * (float(t) * p["DT"]), o[1] + o[3] * (float(t) * p["DT"])])
            nrm = (path[:2, t] - c) / np.hypot(*(path[:2, t] - c))          # the row's normal comes from the path, not from the plain optimum
            # ... so this is the row's violation at the plain optimum (at T = 2 only a_0 moves p_2, by DT^2 per m/s^2: a smaller push there)
            o[4] = float(nrm @ (xs[:2, t] - c)) + (2e-5 if T > 2 else 1e-6) * 2 ** j
            obs[e, 0] = o
        elif f == "inside":                                      # the ego is 10 .. 25 mm inside it at step 1, which no input moves
            obs[e, M - 1] = _beside(path, 1, (-1.0 if j % 2 else 1.0) * (0.45 - 0.01 - 0.005 * j), 0.45)
        elif f == "on_pbar":                                     # exactly on the path's point: the fallback normal
            t = min(T, 1 + 3 * j)
            obs[e, 0] = [path[0, t], path[1, t], 0.0, 0.0, 0.03]
        elif f == "selection":                                   # more live slots near one step than rows: clearances 0.1 m apart; j = 0: ties;
            t = min(T, 2 + j % 3)                                # j = 1: slot 0 moves (it is where the pattern puts it when the ego gets there)
            for m in range(M):
                hd = path[4, t] + path[6, t]                     # (it moves away from the path, to the side it is on)
                vv = (-0.37 * math.sin(hd), 0.37 * math.cos(hd)) if (j == 1 and m == 0) else (0.0, 0.0)   # (0.1 m in no whole number of steps)
                obs[e, m] = _beside(path, t, (0.55 + 0.1 * ((m * 5 + j) % M)) * (-1.0 if m % 2 else 1.0), 0.30, vv)
            if j == 0 and M >= 3:
                obs[e, 1:] = obs[e, 0]
        elif f == "empty_between":                               # live slots at both ends, empty ones of every kind between
            obs[e, 0] = _beside(path, min(T, 2), 0.6, 0.42)
            obs[e, M - 1] = _beside(path, min(T, 3), -0.7, 0.45)
            for m in range(1, M - 1):
                obs[e, m] = [np.nan, 1.0, np.nan, 0.0, [-1.0, np.nan][m % 2]]
        elif f == "nan_live":                                    # a live slot with a non-finite number: status 3
            obs[e, 0] = _beside(path, 1, 1.0, 0.45)
            obs[e, M - 1] = _beside(path, 1, 1.0, 0.45)
            obs[e, M - 1, j % 4] = [np.nan, np.inf, -np.inf][j % 3]
        elif f == "v0_out":                                      # status 1: the speed, or the steering angle, outside its bounds at t = 0
            if j % 2:
                x0[e, 2] = 0.42
            else:
                x0[e, 3] = 6.2
            obs[e, 0] = _beside(path, 1, 1.0, 0.45)
        elif f == "near":                                        # the edge 0.01 m beside the plain QP's own trajectory at a middle step: the row
            t = min(T, max(2, tm + j))                           # cannot bind unless a margin above 0.01 m widens the disc
            xs = SQ.solve_case(x0[e], ref[e], oa[e], odv[e], p)["x"]
            at = path.copy(); at[:2] = xs[:2]
            o = _beside(at, t, (-1.0 if j % 2 else 1.0) * 0.43, 0.40)
            c = np.array(o[:2])
            nrm = (path[:2, t] - c) / np.hypot(*(path[:2, t] - c))
            o[4] = float(nrm @ (xs[:2, t] - c)) - 0.01
            obs[e, 0] = o
    for a in (x0, ref, oa, odv, obs):
        a.setflags(write=False)
    return x0, ref, oa, odv, obs, fam


def solve_scene(T, M, margin=0.0):
    """the yardstick's solution per ego, computed here; None where the GPU reports a status instead (nan_live: 3, v0_out: 1)"""
    x0, ref, oa, odv, obs, fam = exact_scene(T, M)
    p = SQ.default_params(T)
    return tuple(None if e in fam["nan_live"] else A.solve(x0[e], ref[e], oa[e], odv[e], obs[e], p, margin=margin) for e in range(n_egos(T)))


def _key(T, M, margin):
    return f"T{T}_M{M}_" + (f"m{int(round(1000 * margin))}_" if margin else "")


def pack(sols, T):
    """solve_scene's output as the golden file's arrays: per ego the optimum's ACTIVE SET (the rows of build()'s problem with a multiplier),
    from which from_active_set() has the point and the multipliers back by one linear solve -- a tenth of the bytes of the numbers"""
    nz = [np.flatnonzero(s["lam"] > 0.0) if s else np.zeros(0, int) for s in sols]
    width = max(1, max(len(z) for z in nz))
    rows = np.full((len(sols), width), -1, np.int16)
    for e, z in enumerate(nz):
        rows[e, :len(z)] = z
    return dict(solved=np.array([s is not None for s in sols]), active=rows, degenerate=np.array([bool(s and s["degenerate"]) for s in sols]))


def from_active_set(b, rows):
    """(w, lam) of build()'s problem from its optimum's active set: the equality-constrained KKT system of those rows on the shifted and
    scaled problem, solved with the yardstick's extended-precision refinement.  Whether it IS the optimum the certificate decides."""
    cs, D, w0 = A.scaled(b)
    lam0 = np.zeros(len(b["h"]))
    lam0[rows] = 1.0
    ws, lam = A._polish(cs["H"], cs["g"], cs["G"], cs["h"], np.zeros(len(D)), lam0)
    if len(rows) == 0:
        ws = np.linalg.solve(cs["H"], -cs["g"])
    return D * ws + w0, lam


@functools.lru_cache(maxsize=None)
def exact_solutions(T, M, margin=0.0):
    """solve_scene(T, M, margin) as recorded in the golden file: the point and the multipliers are the record's, the problem and the
    certificate are rebuilt here (so a record that is not the optimum of THIS problem does not certify)"""
    x0, ref, oa, odv, obs, fam = exact_scene(T, M)
    p = SQ.default_params(T)
    g = np.load(os.path.join(GOLDEN, GOLDEN_FILE), allow_pickle=False)
    k = _key(T, M, margin)
    n = 2 * T
    out = []
    for e in range(n_egos(T)):
        if not g[k + "solved"][e]:
            out.append(None)
            continue
        b = A.build(x0[e], ref[e], oa[e], odv[e], obs[e], p, margin=margin)
        r = g[k + "active"][e]
        w, lam = from_active_set(b, r[r >= 0])
        al = np.zeros(n + 1)
        al[b["rows"]] = lam[b["m0"]:-1]
        al[n] = lam[-1]
        ct = A.cert(b, w, lam)
        out.append(dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=bool(g[k + "degenerate"][e]),
                        planes=b["planes"], cert=ct, certified=A.cert_ok(ct, lam), steer=float(x0[e, 2] + w[0] * p["DT"]),
                        speed=float(x0[e, 3] + w[1] * p["DT"]), obj=float(0.5 * w @ b["H"] @ w + b["g"] @ w + b["cond"]["c"]), build=b))
    return tuple(out)


def expected_status(T, M):
    fam = exact_scene(T, M)[5]
    st = np.zeros(n_egos(T), np.int32)
    st[fam["nan_live"]] = 3
    st[fam["v0_out"]] = 1
    return st


def assert_families(T, M, margin, obs, sols, fam):
    p = SQ.default_params(T)
    live = lambda e: int((obs[e, :, 4] >= 0).sum())      # noqa: E731
    amax = lambda s: float(s["avoid_lam"][:-1].max())    # noqa: E731
    assert all(s["eps"] < EPS_MAX for s in sols if s is not None), max(s["eps"] for s in sols if s is not None)
    for e in fam["no_live"]:
        assert live(e) == 0 and len(sols[e]["build"]["rows"]) == 0 and (sols[e]["planes"][:, :, 3] == -1).all() and abs(sols[e]["eps"]) <= 1e-9
    for e in fam["inactive"]:
        assert live(e) >= 1 and len(sols[e]["build"]["rows"]) >= T and amax(sols[e]) == 0.0 and abs(sols[e]["eps"]) <= 1e-9
    if margin == 0.0:                                            # (a margin is a push of its own size: the slack takes part of it)
        assert sum(amax(sols[e]) > 1e-6 and sols[e]["eps"] <= 1e-9 for e in fam["active"]) >= 1, [(amax(sols[e]), sols[e]["eps"]) for e in fam["active"]]
    else:
        assert all(amax(sols[e]) > 1e-6 for e in fam["active"])
    assert all(sols[e]["eps"] > 5e-3 for e in fam["inside"]), [sols[e]["eps"] for e in fam["inside"]]
    for e in fam["on_pbar"]:
        d = sols[e]["build"]["data"]
        t = min(T, 1 + 3 * family(e)[1])
        n = sols[e]["planes"][t - 1, 0, :2]
        hd = d["path"][4, t] + d["path"][6, t]
        assert sols[e]["planes"][t - 1, 0, 3] == 0 and np.array_equal(n, [-math.cos(hd), -math.sin(hd)])
    if M >= 3:
        moving = 0
        for e in fam["selection"]:
            assert live(e) == M > 2
            moving += bool((obs[e, :, 2:4] != 0).any())
            path = sols[e]["build"]["data"]["path"]
            for t in range(1, T + 1):
                tau = float(t) * p["DT"]
                cl = np.array([math.hypot(path[0, t] - (o[0] + o[2] * tau), path[1, t] - (o[1] + o[3] * tau)) - o[4] for o in obs[e]])
                order = np.argsort(cl, kind="stable")
                assert list(sols[e]["planes"][t - 1, :, 3]) == list(order[:2])
                gaps = np.diff(cl[order])
                assert ((gaps >= 1e-6) | (gaps == 0.0)).all()           # never a rounding matter: well apart, or the very same disc
        assert moving >= 1
        for e in fam["empty_between"]:
            assert live(e) == 2 and obs[e, 0, 4] >= 0 and obs[e, M - 1, 4] >= 0
            assert set(np.unique(sols[e]["planes"][:, :, 3])) == {0.0, float(M - 1)}
    for e in fam["nan_live"]:
        assert sols[e] is None and live(e) >= 1 and not np.isfinite(obs[e][obs[e, :, 4] >= 0]).all()
    for e in fam["v0_out"]:
        assert sols[e] is None
    for e in fam["near"]:                                        # the margin's family: rows present either way, binding only with the margin
        assert live(e) == 1 and len(sols[e]["build"]["rows"]) == T
        if margin == 0.0 and T <= 10:                            # (at longer horizons the path the normals come from leaves the plain optimum's
            assert amax(sols[e]) == 0.0                          # trajectory, and a neighbouring step's half-plane may cut into it)
    if margin > 0.01:
        assert sum(amax(sols[e]) > 1e-6 for e in fam["near"]) >= 1, [amax(sols[e]) for e in fam["near"]]


def uncertified(sols):
    return sum(1 for s in sols if s is not None and not s["certified"])
