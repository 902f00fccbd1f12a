"""The scenes of the wall-row tests (tests/test_kmpc_qp_walls_host.py, tests/test_gpu_kmpc_qp_walls.py), built and solved on the CPU with
tests/kmpc_qp_walls_ref.py: a hand-made grid and a batch of 65 egos whose states cover every family of rows.  A helper module, not a conftest;
nothing here touches a GPU.

The grid: 96 x 64 cells of 0.1 m, origin (-1.23, 0.57).  Occupied everywhere but
  the corridor        gx 4..59,  gy 24..35: 1.2 m wide, along +x;
  the notch           gx 24..35, gy 36..43: the corridor's left wall set back by 0.8 m for 1.2 m;
  the free region     gx 64..95, gy 0..63: 3.2 m wide -- wider than twice the scenes' reach of 1.0 m -- and touching the image's right, top and
                      bottom borders.
The egos are slow enough for the previous solution's path to stay within ~1.2 m of where it starts, whatever the horizon.
"""
import functools
import math
import os

import numpy as np

import kmpc_qp_ref as Q
import kmpc_qp_walls_ref as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_FILE = "g23_kmpc_qp_walls.npz"       # tools/gen_golden_kmpc_qp_walls.py: solve_scene() of the T = 31 shape

RES, ORIGIN, GW, GH = 0.1, (-1.23, 0.57), 96, 64
N_SAMPLES = 20                              # the scenes' reach: 20 x 0.05 m = 1.0 m
E = 65                                      # the last wave group of a launch is half full (two egos per wave) or one more block (one per wave)
SHAPES = ((2, 0), (8, 0), (8, 4), (31, 16))
FAMILIES = ("no_wall", "one_side", "both_sides", "disc_and_wall", "two_discs", "exact_reach", "leaves_image", "inside_wall", "outside_image",
            "v0_out", "nan_state")


def family_of(e):
    return FAMILIES[e % len(FAMILIES)]


@functools.lru_cache(maxsize=None)
def grid_image():
    """the map image u8 [h][w], row 0 at the top, 0 = occupied, 255 = free (f1p_set_grid with occupied_below = 128)"""
    cells = np.ones((GH, GW), np.uint8)                          # gy order, 1 = occupied
    cells[24:36, 4:60] = 0
    cells[36:44, 24:36] = 0
    cells[:, 64:96] = 0
    img = np.where(cells[::-1] == 1, 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


def grid_of(active_image_cells=None):
    """the yardstick's grid: of the hand-made image as it is, or of the cells Context.grid_debug_read(1) returned (image row order)"""
    cells = (grid_image() == 0) if active_image_cells is None else active_image_cells
    return (W.from_image(np.asarray(cells, dtype=np.uint8)), RES, ORIGIN)


def wx(gx):
    return ORIGIN[0] + gx * RES


def wy(gy):
    return ORIGIN[1] + gy * RES


def _beside(path, t, lat, r):
    """a parked disc whose centre is `lat` metres left of the path's point at step t"""
    x, y, yaw = path[0, t], path[1, t], path[3, t]
    return [x - lat * math.sin(yaw), y + lat * math.cos(yaw), 0.0, 0.0, r]


@functools.lru_cache(maxsize=None)
def scene(T, M):
    """-> x0 [E, 4], ref [E, 4, T+1], oa, od [E, T] (a non-zero previous solution), obs [E, M, 5], fam {family: egos}.  What a family promises
    is asserted from the yardstick's output (assert_families), not assumed."""
    p = Q.default_params(T)
    rng = np.random.default_rng(7000 * T + M)
    horizon = T * p["DTK"]
    x0 = np.zeros((E, 4))
    oa = rng.normal(0.0, min(0.5, 0.1 / horizon), (E, T))
    od = rng.normal(0.0, 0.02, (E, T))
    obs = np.zeros((E, M, 5))
    obs[:, :, 4] = -1.0
    ref = np.zeros((E, 4, T + 1))
    fam = {f: [] for f in FAMILIES}
    tm = max(1, T // 2)
    for e in range(E):
        f, j = family_of(e), e // len(FAMILIES)
        fam[f].append(e)
        v = min(3.0, rng.uniform(0.7, 1.2) / horizon)
        along_x = (wx(5) + rng.uniform(0.0, 0.4), 0.0 + rng.normal(0.0, 0.03))          # in the corridor before the notch, heading +x
        x, y, yaw = along_x[0], wy(30) + rng.uniform(-0.25, 0.25), along_x[1]
        if f == "no_wall":                                       # the middle of the free region, heading +y: 1.6 m to either side
            x, y, yaw = wx(80) + rng.uniform(-0.3, 0.3), wy(10) + rng.uniform(0.0, 2.0), math.pi / 2 + rng.normal(0.0, 0.03)
        elif f == "one_side":                                    # in the notch, 0.25 .. 0.45 m from the right wall: the left one is 1.5 m away
            x, y = wx(25) + rng.uniform(0.0, 0.1), wy(24) + rng.uniform(0.25, 0.45)
            v = min(v, 0.7 / horizon)
        elif f == "disc_and_wall" or f == "two_discs":
            y = wy(30) + rng.uniform(0.05, 0.2)                  # nearer to the left wall
        elif f == "exact_reach":                                 # heading exactly +x, no steering: the left wall's first occupied sample is
            yaw, od[e] = 0.0, 0.0                                # number N_SAMPLES (j even) or N_SAMPLES + 1 (j odd) at every step
            # (in the notch, whose back wall is at gy 44; the path stays inside the notch's 1.2 m)
            x, y = wx(26) + rng.uniform(0.0, 0.05), wy(44) - (N_SAMPLES * 0.05 - 0.02 if j % 2 == 0 else N_SAMPLES * 0.05 + 0.03)
            v = min(v, 0.6 / horizon)
        elif f == "leaves_image":                                # 0.2 .. 0.4 m from the image's right border, heading +y
            x, y, yaw = wx(96) - rng.uniform(0.2, 0.4), wy(10) + rng.uniform(0.0, 2.0), math.pi / 2 + rng.normal(0.0, 0.02)
        elif f == "inside_wall":                                 # in the occupied band below the corridor
            y = wy(24) - rng.uniform(0.2, 0.45)
        elif f == "outside_image":
            x, y = ORIGIN[0] - rng.uniform(1.0, 3.0), ORIGIN[1] - rng.uniform(1.0, 3.0)
        elif f == "v0_out":
            v = [6.2, -0.1][j % 2]
        x0[e] = (x, y, v, yaw)
        path = Q.predict_motion(x0[e], oa[e], od[e], p)
        # the reference: straight on at the ego's speed, pulled up to 0.5 m to one side -- so the optimum leans on a wall's rows
        lat = rng.uniform(-0.5, 0.5)
        tt = np.arange(T + 1) * p["DTK"]
        vr = min(max(v, 0.0), 6.0)
        ref[e] = (x + vr * tt * math.cos(yaw) - lat * math.sin(yaw), y + vr * tt * math.sin(yaw) + lat * math.cos(yaw), np.full(T + 1, vr),
                  np.full(T + 1, yaw))
        if f == "disc_and_wall" and M >= 1:                      # one disc 0.15 m off the path in the middle of the horizon: nearer than both walls
            obs[e, M - 1] = _beside(path, tm, -(0.15 + 0.30), 0.30)
        elif f == "two_discs" and M >= 2:                        # two of them, clearances 0.10 and 0.20 m
            obs[e, 0] = _beside(path, tm, -(0.20 + 0.30), 0.30)
            obs[e, M - 1] = _beside(path, tm, 0.10 + 0.25, 0.25)
        elif f == "nan_state":
            x0[e, j % 4] = [np.nan, np.inf, -np.inf][j % 3]
        elif M >= 1 and f == "both_sides":                       # a far disc: a live slot that never gets a row, both walls are nearer
            obs[e, 0] = _beside(path, 1, 3.0, 0.3)
    for a in (x0, ref, oa, od, obs):
        a.setflags(write=False)
    return x0, ref, oa, od, obs, fam


def solve_scene(T, M, grid=None):
    """the yardstick's solution per ego; None where the GPU reports a status instead (nan_state: 3, v0_out: 1)"""
    x0, ref, oa, od, obs, _ = scene(T, M)
    p = Q.default_params(T)
    g = grid_of() if grid is None else grid
    return tuple(W.solve(x0[e], ref[e], oa[e], od[e], obs[e], g, p, N_SAMPLES) for e in range(E))


@functools.lru_cache(maxsize=None)
def solutions(T, M):
    """solve_scene(T, M) on the hand-made grid.  T = 31: the points and multipliers recorded in the golden file, re-certified on the problems
    rebuilt here (a record that is not the optimum of THIS problem does not certify); the short horizons are solved outright."""
    if T < 31:
        return solve_scene(T, M)
    x0, ref, oa, od, obs, _ = scene(T, M)
    p = Q.default_params(T)
    g = np.load(os.path.join(GOLDEN, GOLDEN_FILE), allow_pickle=False)
    k, n, grid = f"T{T}_M{M}_", 2 * T, grid_of()
    out = []
    for e in range(E):
        if not g[k + "solved"][e]:
            out.append(None)
            continue
        b = W.build(x0[e], ref[e], oa[e], od[e], obs[e], grid, p, N_SAMPLES)
        w, al = g[k + "w"][e], g[k + "avoid_lam"][e]
        lam = W.lam_full(b, g[k + "lam"][e], al)
        out.append(dict(u=w[:n].reshape(T, 2), eps=float(w[n]), w=w, lam=lam, avoid_lam=al, degenerate=bool(g[k + "degenerate"][e]),
                        planes=b["planes"], cert=W.cert(b, w, lam), steer=float(w[1]), speed=float(x0[e, 2] + w[0] * p["DTK"]), build=b,
                        edge=b["edge"]))
    return tuple(out)


# The feasible egos on which the interior point stops at its last iterate (status 2: its Cholesky factorisation breaks down before the
# absolute gap reaches 1e-10, DESIGN.md 5s "Status 2"), as recorded on an MI355X.  The kernel's arithmetic does not depend on an ego's
# neighbours, so the record is exact; every other feasible ego must converge.  An ego listed here is held to every bar of a converged one.
NOT_CONVERGED = {(8, 0): (62,)}


def expected_status(T, M):
    fam = scene(T, M)[5]
    st = np.zeros(E, np.int32)
    st[list(NOT_CONVERGED.get((T, M), ()))] = 2
    st[fam["nan_state"]] = 3
    st[fam["v0_out"]] = 1
    return st


def assert_families(T, M, sols):
    """every family is populated with what it promises, read from the yardstick's planes"""
    x0, ref, oa, od, obs, fam = scene(T, M)
    p = Q.default_params(T)
    grid = grid_of()
    assert all(len(v) >= 5 for v in fam.values())
    slots = lambda e: sols[e]["planes"][:, :, 3]               # noqa: E731
    walls = lambda e: np.isin(slots(e), (W.SLOT_L, W.SLOT_R))  # noqa: E731
    for e in fam["no_wall"]:
        assert not walls(e).any() and (slots(e) == -1).all()
    for e in fam["one_side"]:
        assert (walls(e).sum(axis=1) == 1).all() and (slots(e)[:, 0] == W.SLOT_R).all()
    for e in fam["both_sides"]:
        assert (walls(e).sum(axis=1) == 2).all()
        assert {tuple(r) for r in slots(e)} <= {(W.SLOT_L, W.SLOT_R), (W.SLOT_R, W.SLOT_L)}
    assert len({tuple(r) for e in fam["both_sides"] for r in slots(e)}) == 2                   # nearer left and nearer right both occur
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
            k, _ = W.march(grid, path[0, t], path[1, t], -math.sin(path[3, t]), math.cos(path[3, t]), N_SAMPLES)
            k1, _ = W.march(grid, path[0, t], path[1, t], -math.sin(path[3, t]), math.cos(path[3, t]), N_SAMPLES + 1)
            assert (k, k1) == ((N_SAMPLES, N_SAMPLES) if j % 2 == 0 else (0, N_SAMPLES + 1)), (e, t, k, k1)
        assert (W.SLOT_L in slots(e)) == (j % 2 == 0)
    assert {e // len(FAMILIES) % 2 for e in fam["exact_reach"]} == {0, 1}
    for e in fam["leaves_image"]:
        s = sols[e]
        assert (slots(e)[:, 0] == W.SLOT_R).all() and (slots(e)[:, 1] == -1).all()
        path = s["build"]["data"]["path"]
        for t in range(1, T + 1):                                # the contact is inside the image, the sample after it is not
            k, _ = W.march(grid, path[0, t], path[1, t], math.sin(path[3, t]), -math.cos(path[3, t]), N_SAMPLES)
            q = W.sample(grid, path[0, t], path[1, t], math.sin(path[3, t]), -math.cos(path[3, t]), k)
            assert W.cell(grid, *q) is None and k >= 2
    for e in fam["inside_wall"]:
        s = sols[e]
        assert occupied_path(grid, s) and (np.sort(slots(e), axis=1) == (W.SLOT_L, W.SLOT_R)).all()
        pl = s["planes"]
        assert np.array_equal(pl[:, 0, :2], -pl[:, 1, :2])     # pinned between two contacts that coincide: opposite normals
    for e in fam["outside_image"]:
        assert (slots(e) == (W.SLOT_L, W.SLOT_R)).all()
        path = sols[e]["build"]["data"]["path"]
        assert all(W.cell(grid, path[0, t], path[1, t]) is None for t in range(T + 1))
    for e in fam["v0_out"] + fam["nan_state"]:
        assert sols[e] is None
    assert not Q.feasible(x0[fam["v0_out"][0]], p) and not np.isfinite(x0[fam["nan_state"]]).all(axis=1).any()


def occupied_path(grid, sol):
    path = sol["build"]["data"]["path"]
    return all(W.occupied(grid, path[0, t], path[1, t]) for t in range(1, path.shape[1]))
