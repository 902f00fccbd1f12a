"""The scenes of the dynamic QP's wall-row tests (tests/test_stmpc_qp_walls_host.py, tests/test_gpu_stmpc_qp_walls.py), built and solved on the
CPU with tests/stmpc_qp_walls_ref.py: the hand-made 96 x 64 grid of tests/kmpc_qp_walls_scenes.py and batches of dynamic-branch states
(v > V_KS = 2 m/s) whose poses cover every family of rows.  A helper module, not a conftest; nothing here touches a GPU.

The grid (kmpc_qp_walls_scenes): cells of 0.1 m, origin (-1.23, 0.57); free are the corridor gx 4..59, gy 24..35 (1.2 m wide, along +x), the
notch gx 24..35, gy 36..43 (the corridor's left wall set back by 0.8 m) and the region gx 64..95 (3.2 m wide, open to the image's right, top
and bottom borders).  An ego covers at most 2.2 m within its horizon (T = 40: 1 s at 2.05 .. 2.15 m/s; shorter horizons are faster): the
straight walls the families lean on are the corridor behind the notch (2.4 m) and the free region's borders (6.4 m).
The previous solution is the plain QP's optimum plus a little noise, what a warm-started planner holds (a random one squeezes
every ego); it costs a solve per ego and is recorded in the golden file beside the long shapes' optima.
"""
import functools
import math
import os

import numpy as np

import grid_ref as GR
import kmpc_qp_walls_scenes as KS
import stmpc_qp_avoid_scenes as AS
import stmpc_qp_ref as SQ
import stmpc_qp_walls_ref as W
from kmpc_qp_walls_scenes import ORIGIN, RES, grid_image, grid_of, wx, wy  # noqa: F401

GOLDEN = KS.GOLDEN
GOLDEN_FILE = "g24_stmpc_qp_walls.npz"      # tools/gen_golden_stmpc_qp_walls.py
N_SAMPLES = 20                              # the scenes' reach: 20 x 0.05 m = 1.0 m
CAP = AS.CAP
FAMILIES = ("exact_reach", "both_sides", "beta", "one_side", "no_wall", "disc_and_wall", "two_discs", "leaves_image", "inside_wall",
            "outside_image", "v0_out", "nan_state")


def B():
    """the first horizon whose LDS layout crosses 64 KiB: the kernel's other launch path (f1p_stmpc_qp_avoid_lds_bytes)"""
    return AS.opt_in_horizon() + 1


def shapes():
    return ((2, 0), (10, 0), (10, 4), (24, 4), (B(), 0), (CAP, 16))


RECORDED = lambda T: T >= 24                # noqa: E731  the shapes whose optima the golden file holds (minutes of exact solves); shorter: solved in the test


def n_egos(T):
    return 16 if T == CAP else 36


def family_of(e):
    return FAMILIES[e % len(FAMILIES)]


def _beside(path, t, lat, r):
    """a parked disc whose centre is `lat` metres left of the path's point at step t, seen along the direction of travel"""
    x, y, hd = path[0, t], path[1, t], W.heading(path, t)
    return [x - lat * math.sin(hd), y + lat * math.cos(hd), 0.0, 0.0, r]


@functools.lru_cache(maxsize=None)
def base(T):
    """-> x0 [E, 7], ref [E, 7, T+1], fam {family: egos}: the states and references of horizon T, whatever M"""
    E = n_egos(T)
    p = SQ.default_params(T)
    rng = np.random.default_rng(9000 * T + 1)
    horizon = T * p["DT"]
    x0 = np.zeros((E, 7))
    ref = np.zeros((E, 7, T + 1))
    fam = {f: [] for f in FAMILIES}
    for e in range(E):
        f, j = family_of(e), e // len(FAMILIES)
        fam[f].append(e)
        v = max(2.05 + rng.uniform(0.0, 0.1), min(4.0, rng.uniform(0.7, 1.2) / horizon))
        delta, yr, beta = rng.normal(0.0, 0.02), rng.normal(0.0, 0.05), rng.normal(0.0, 0.005)
        x, y, yaw = wx(5) + rng.uniform(0.0, 0.4), wy(30) + rng.uniform(-0.25, 0.25), rng.normal(0.0, 0.03)   # the corridor before the notch, heading +x
        if f == "no_wall":                                       # the middle of the free region, heading +y: 1.6 m to either side
            x, y, yaw = wx(80) + rng.uniform(-0.3, 0.3), wy(10) + rng.uniform(0.0, 2.0), math.pi / 2 + rng.normal(0.0, 0.03)
        elif f == "one_side":                                    # heading +y, 0.25 .. 0.45 m from the free region's left border: the right one is 2.7 m away
            x, y, yaw = wx(64) + rng.uniform(0.25, 0.45), wy(10) + rng.uniform(0.0, 2.0), math.pi / 2 + rng.normal(0.0, 0.02)
        elif f == "both_sides":                                  # the corridor behind the notch: 2.4 m of two straight walls
            x = wx(36) + rng.uniform(0.03, 0.1)
            y = wy(30) + (-1.0 if j % 2 else 1.0) * rng.uniform(0.08, 0.2)      # nearer to the left wall, or to the right one
        elif f == "disc_and_wall" or f == "two_discs":
            y = wy(30) + rng.uniform(0.05, 0.2)                  # nearer to the left wall
        elif f == "exact_reach":                                 # behind the notch, heading exactly +x with nothing that turns it: the left wall's first
            yaw = delta = yr = beta = 0.0                        # occupied sample is number N_SAMPLES (j even) or N_SAMPLES + 1 (j odd) at every step
            x, y = wx(36) + rng.uniform(0.03, 0.1), wy(36) - (N_SAMPLES * 0.05 - 0.02 if j % 2 == 0 else N_SAMPLES * 0.05 + 0.03)
        elif f == "beta":                                        # slipping (a third of it is gone a step later): the direction of travel points to the right
            yaw, beta = 0.05, -0.30 - 0.02 * (j % 3)             # of the yaw; just before the notch's corner, 0.3 .. 0.4 m under the left wall: the march along the
            x, y = wx(24) - v * p["DT"] - rng.uniform(0.01, 0.03), wy(36) - rng.uniform(0.3, 0.4)   # direction of travel enters the notch, the yaw's does not
        elif f == "leaves_image":                                # 0.2 .. 0.4 m from the image's right border, heading +y
            x, y, yaw = wx(96) - rng.uniform(0.2, 0.4), wy(10) + rng.uniform(0.0, 2.0), math.pi / 2 + rng.normal(0.0, 0.02)
        elif f == "inside_wall":                                 # in the occupied band below the corridor
            y = wy(24) - rng.uniform(0.25, 0.45)
        elif f == "outside_image":
            x, y = ORIGIN[0] - rng.uniform(1.0, 3.0), ORIGIN[1] - rng.uniform(1.0, 3.0)
        x0[e] = (x, y, delta, v, yaw, yr, beta)
        # the reference: straight on at the ego's speed, pulled to one side -- by up to 0.5 m, into a wall, where the family does not promise
        # which rows there are: the plain optimum the path comes from then ends inside the wall, pinned with a positive slack
        wide = f in ("beta", "disc_and_wall", "inside_wall", "outside_image", "v0_out", "nan_state")
        lat = rng.uniform(-0.5, 0.5) if wide else rng.uniform(-0.1, 0.1)
        tt = np.arange(T + 1) * p["DT"]
        hd = yaw + beta
        ref[e, 0], ref[e, 1] = x + v * tt * math.cos(hd) - lat * math.sin(hd), y + v * tt * math.sin(hd) + lat * math.cos(hd)
        ref[e, 3], ref[e, 4] = v, yaw
    x0.setflags(write=False); ref.setflags(write=False)
    return x0, ref, fam


PREV = {}            # T -> (oa, odv): set by tools/gen_golden_stmpc_qp_walls.py while it writes the file the tests read them from


def compute_prev(T):
    """the scenes' previous solution (oa, odv) [E, T]: the plain QP's optimum from zeros plus a little noise; exact_reach keeps odv = 0"""
    x0, ref, fam = base(T)
    p = SQ.default_params(T)
    rng = np.random.default_rng(9000 * T + 2)
    E = n_egos(T)
    oa, odv = np.zeros((E, T)), np.zeros((E, T))
    for e in range(E):
        u = SQ.solve_case(x0[e], ref[e], np.zeros(T), np.zeros(T), p)["u"]
        oa[e] = (u[:, 1] + rng.normal(0.0, 0.02, T)).clip(-3.0, 3.0)
        odv[e] = (u[:, 0] + rng.normal(0.0, 0.01, T)).clip(-3.2, 3.2)
    odv[fam["exact_reach"]] = 0.0
    return oa, odv


def golden():
    return np.load(os.path.join(GOLDEN, GOLDEN_FILE), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def scene(T, M):
    """-> x0 [E, 7], ref [E, 7, T+1], oa, odv [E, T], obs [E, M, 5], fam {family: egos}.  What a family promises is asserted from the
    yardstick's output (assert_families), not assumed.  v0_out and nan_state spoil x0 after everything else was laid out."""
    x0, ref, fam = base(T)
    x0 = x0.copy()
    E = n_egos(T)
    p = SQ.default_params(T)
    if T in PREV:
        oa, odv = PREV[T]
    else:
        g = golden()
        oa, odv = g[f"T{T}_prev_oa"].copy(), g[f"T{T}_prev_odv"].copy()
    obs = np.zeros((E, M, 5))
    obs[:, :, 4] = -1.0
    tm = max(1, T // 2)
    for e in range(E):
        f, j = family_of(e), e // len(FAMILIES)
        path = SQ.predict_motion(x0[e], oa[e], odv[e], p)
        if f == "disc_and_wall" and M >= 1:                      # one disc 0.15 m off the path in the middle of the horizon: nearer than both walls
            obs[e, M - 1] = _beside(path, tm, -(0.15 + 0.30), 0.30)
        elif f == "two_discs" and M >= 2:                        # two of them, clearances 0.10 and 0.20 m
            obs[e, 0] = _beside(path, tm, -(0.20 + 0.30), 0.30)
            obs[e, M - 1] = _beside(path, tm, 0.10 + 0.25, 0.25)
        elif f == "both_sides" and M >= 1:                       # a far disc: a live slot that never gets a row, both walls are nearer
            obs[e, 0] = _beside(path, 1, 3.0, 0.3)
        elif f == "v0_out":                                      # status 1: the speed, or the steering angle, outside its bounds at t = 0
            if j % 2:
                x0[e, 2] = 0.42
            else:
                x0[e, 3] = 6.2
        elif f == "nan_state":
            x0[e, (0, 1, 4, 6)[j % 4]] = [np.nan, np.inf, -np.inf][j % 3]
    for a in (x0, oa, odv, obs):
        a.setflags(write=False)
    return x0, ref, oa, odv, obs, fam


def solve_scene(T, M, grid=None):
    """the yardstick's solution per ego, computed here; None where the GPU reports a status instead (nan_state: 3, v0_out: 1)"""
    x0, ref, oa, odv, obs, _ = scene(T, M)
    p = SQ.default_params(T)
    g = grid_of() if grid is None else grid
    return tuple(W.solve(x0[e], ref[e], oa[e], odv[e], obs[e], g, p, N_SAMPLES) for e in range(n_egos(T)))


pack, from_active_set = AS.pack, AS.from_active_set            # the golden file's form: per ego the optimum's active set


@functools.lru_cache(maxsize=None)
def solutions(T, M):
    """solve_scene(T, M) on the hand-made grid.  The recorded shapes: the active sets of the golden file, from which the point and the
    multipliers come back by one linear solve on the problem rebuilt here, re-certified (a record that is not the optimum of THIS problem
    does not certify); the short horizons are solved outright."""
    if not RECORDED(T):
        return solve_scene(T, M)
    x0, ref, oa, odv, obs, _ = scene(T, M)
    p = SQ.default_params(T)
    g, k, grid = golden(), f"T{T}_M{M}_", grid_of()
    out = []
    for e in range(n_egos(T)):
        if not g[k + "solved"][e]:
            out.append(None)
            continue
        b = W.build(x0[e], ref[e], oa[e], odv[e], obs[e], grid, p, N_SAMPLES)
        r = g[k + "active"][e]
        w, lam = from_active_set(b, r[r >= 0])
        out.append(W.result(b, x0[e], p, w, lam, g[k + "degenerate"][e]))
    return tuple(out)


# The feasible egos on which the interior point stops at its last iterate (status 2, DESIGN.md 5s "Status 2"), as recorded on an MI355X.  The
# kernel's arithmetic does not depend on an ego's neighbours, so the record is exact; every other feasible ego must converge.  An ego listed
# here is held to every bar of a converged one.
NOT_CONVERGED = {}


def expected_status(T, M):
    fam = scene(T, M)[5]
    st = np.zeros(n_egos(T), np.int32)
    st[list(NOT_CONVERGED.get((T, M), ()))] = 2
    st[fam["nan_state"]] = 3
    st[fam["v0_out"]] = 1
    return st


def occupied_path(grid, sol):
    path = sol["build"]["data"]["path"]
    return all(W.occupied(grid, path[0, t], path[1, t]) for t in range(1, path.shape[1]))


def yaw_heading(path, t):
    return path[4, t]


def assert_families(T, M, sols):
    """every family is populated with what it promises, read from the yardstick's planes"""
    x0, ref, oa, odv, obs, fam = scene(T, M)
    p = SQ.default_params(T)
    grid = grid_of()
    assert all(len(v) >= (1 if T == CAP else 3) for v in fam.values())
    slots = lambda e: sols[e]["planes"][:, :, 3]               # noqa: E731
    walls = lambda e: np.isin(slots(e), (W.SLOT_L, W.SLOT_R))  # noqa: E731
    for e in range(n_egos(T)):
        if sols[e] is not None:                                  # every linearisation path stays inside the image but outside_image's
            path = sols[e]["build"]["data"]["path"]
            inside = all(W.cell(grid, path[0, t], path[1, t]) is not None for t in range(T + 1))
            assert inside == (family_of(e) != "outside_image"), e
    for e in fam["no_wall"]:
        assert not walls(e).any() and (slots(e) == -1).all()
    for e in fam["one_side"]:
        assert (walls(e).sum(axis=1) == 1).all() and (slots(e)[:, 0] == W.SLOT_L).all()
    for e in fam["both_sides"]:
        assert (walls(e).sum(axis=1) == 2).all()
        assert {tuple(r) for r in slots(e)} <= {(W.SLOT_L, W.SLOT_R), (W.SLOT_R, W.SLOT_L)}
    if len(fam["both_sides"]) >= 2:
        assert len({tuple(r) for e in fam["both_sides"] for r in slots(e)}) == 2               # nearer left and nearer right both occur
    if M >= 1:
        for e in fam["disc_and_wall"]:
            s = slots(e)
            assert ((s[:, 0] == M - 1) & np.isin(s[:, 1], (W.SLOT_L, W.SLOT_R))).any(), s
    if M >= 2:
        for e in fam["two_discs"]:
            s = slots(e)
            assert (np.sort(s, axis=1) == (0, M - 1)).all(axis=1).any(), s                     # a step without a wall row
    for e in fam["exact_reach"]:
        path = sols[e]["build"]["data"]["path"]
        j = e // len(FAMILIES)
        for t in range(1, T + 1):
            hd = W.heading(path, t)
            k, _ = W.march(grid, path[0, t], path[1, t], -math.sin(hd), math.cos(hd), N_SAMPLES)
            k1, _ = W.march(grid, path[0, t], path[1, t], -math.sin(hd), math.cos(hd), N_SAMPLES + 1)
            assert (k, k1) == ((N_SAMPLES, N_SAMPLES) if j % 2 == 0 else (0, N_SAMPLES + 1)), (e, t, k, k1)
        assert (W.SLOT_L in slots(e)) == (j % 2 == 0)
    assert {e // len(FAMILIES) % 2 for e in fam["exact_reach"]} == {0, 1}
    for e in fam["beta"]:                                        # the march along the bare yaw finds another k* at some step: another set of rows
        s = sols[e]
        d, c = s["build"]["data"], s["build"]["cond"]
        path = d["path"]
        assert abs(path[6, 1]) > 0.05
        other = W.planes(d, c, obs[e], grid, p, N_SAMPLES, heading=yaw_heading)[0]
        assert not np.array_equal(other[:, :, 3], s["planes"][:, :, 3]), e
        differ = 0
        for t in range(1, T + 1):
            for sg in (1.0, -1.0):
                ks = [W.march(grid, path[0, t], path[1, t], -sg * math.sin(a), sg * math.cos(a), N_SAMPLES)[0] for a in (W.heading(path, t), path[4, t])]
                differ += ks[0] != ks[1]
        assert differ >= 1, e
    for e in fam["leaves_image"]:
        s = sols[e]
        assert (slots(e)[:, 0] == W.SLOT_R).all() and (slots(e)[:, 1] == -1).all()
        path = s["build"]["data"]["path"]
        for t in range(1, T + 1):                                # the contact is inside the image, the sample after it is not
            hd = W.heading(path, t)
            k, _ = W.march(grid, path[0, t], path[1, t], math.sin(hd), -math.cos(hd), N_SAMPLES)
            q = W.sample(grid, path[0, t], path[1, t], math.sin(hd), -math.cos(hd), k)
            assert W.cell(grid, *q) is None and k >= 2
    for e in fam["inside_wall"]:
        s = sols[e]
        assert occupied_path(grid, s) and (np.sort(slots(e), axis=1) == (W.SLOT_L, W.SLOT_R)).all()
        pl = s["planes"]
        assert np.array_equal(pl[:, 0, :2], -pl[:, 1, :2])     # pinned between two contacts that coincide: opposite normals
    for e in fam["outside_image"]:
        assert (slots(e) == (W.SLOT_L, W.SLOT_R)).all()
    for e in fam["v0_out"] + fam["nan_state"]:
        assert sols[e] is None
    assert not SQ.feasible(x0[fam["v0_out"][0]], p) and not np.isfinite(x0[fam["nan_state"]]).all(axis=1).any()


def uncertified(sols):
    return sum(1 for s in sols if s is not None and not s["certified"])


def edge_sensitive(sols):
    return [e for e, s in enumerate(sols) if s is not None and s["edge"]]


# ---- the closed loop beside a wall (tests/test_gpu_stmpc_qp_walls.py; emulated on the CPU in tests/test_stmpc_qp_walls_host.py) -----------------
LOOP = dict(T=10, TK=8, steps=100, reach=1.0, margin=0.1, inflate=0.35, n_samples=20, v=3.0,
            starts=((-0.513, 0.413, 0.01), (-0.207, 0.562, -0.02)))            # off the cells' edges and the axes: no edge-sensitive march


def band_track():
    """a 24 m x 4 m map of 0.1 m cells with a 2 m wide corridor along +x, to be inflated by 0.35 m (three cells: |y| < 0.7 stays free); the
    raceline, at 3 m/s, runs 0.15 m from the left wall -- inside the inflated band -- until x = 8 m and returns to the centre line by x = 10 m
    -> (img, res, origin, [x, y, yaw, v])"""
    res, origin = 0.1, (-2.0, -2.0)
    img = np.zeros((40, 240), np.uint8)
    img[10:30, :] = 255                                          # gy 10 .. 29 free (symmetric: the image's row order does not matter)
    x = np.arange(-1.0, 20.0, 0.05)
    blend = lambda a, b: 0.5 - 0.5 * np.cos(np.pi * np.clip((x - a) / (b - a), 0.0, 1.0))      # noqa: E731
    y = 0.85 * (1.0 - blend(8.0, 10.0))                          # the wall's edge is at y = 1.0
    yaw = np.arctan2(np.gradient(y), np.gradient(x))
    return img, res, origin, [x, y, yaw, np.full_like(x, LOOP["v"])]


def band_grid_inflated():
    """the yardstick's grid of band_track()'s map after set_map(inflate=0.35), by tests/grid_ref.py's restatement of f1p_inflate_grid: three
    more occupied cells on either side of the corridor (and at the image's ends: outside counts as occupied)"""
    img, res, origin, _ = band_track()
    act = GR.dilate(img == 0, GR.inflate_thr(LOOP["inflate"], res))
    return (W.from_image(np.asarray(act, np.uint8)), res, origin)


def loop_start():
    return np.array([[x, y, 0.0, LOOP["v"], yaw, 0.0, 0.0] for x, y, yaw in LOOP["starts"]])


def loop_check(s, ref, prev, grid, walls_on, T):
    """the yardstick's solution of one dynamic-branch plan of the loop: prev = (oa, odv) or None -> W.solve's dict"""
    p = SQ.default_params(T)
    oa, odv = (np.zeros(T), np.zeros(T)) if prev is None else prev
    return W.solve(s, ref, oa, odv, None, grid, p, LOOP["n_samples"] if walls_on else 1, wall_margin=LOOP["margin"])
