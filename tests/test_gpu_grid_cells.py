"""The three bit-packed occupancy maps on the device, CELL BY CELL against the plain numpy reference tests/grid_ref.py (validated on the
CPU by tests/test_grid_ref_host.py): the uploaded grid (k_pack_grid), the active bitmap (k_edt_rows' ballot-packed output through
f1p_inflate_grid / f1p_set_footprint), the clearance map the f32 filters trust (ensure_clear_map, built by a KMPC plan and by lattice plans)
and the point test (cell_of + the bit) -- read through the two test hooks f1p_grid_debug_read and f1p_grid_occupied_batch.  Every
expected value is a boolean or an exact integer: every comparison is assert_array_equal.  The distance image's edge cases are at the end."""
import math

import numpy as np
import pytest

import grid_ref as G
from f1tenth_planning_amd import _abi, synth

pytestmark = pytest.mark.gpu

UPLOADED, ACTIVE, CLEARANCE = 0, 1, 2


@pytest.fixture(scope="module")
def ctx():
    from f1tenth_planning_amd.runtime import Context
    with Context(0) as c:
        yield c


def _read(ctx, which):
    """the map as bool [h][w]; its padding bits are all set (k_pack_grid's rule, kept by every kernel that writes a map)"""
    cells, pad_set, dist = ctx.grid_debug_read(which)
    assert pad_set, f"map {which}: a padding bit beyond column w is clear"
    return cells


def _rejected(ctx, which, code=_abi.F1P_ESTATE):
    from f1tenth_planning_amd.runtime import F1PError
    with pytest.raises(F1PError) as ei:
        ctx.grid_debug_read(which)
    assert ei.value.code == code
    return str(ei.value)


# ---- pack -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", G.HEIGHTS)
@pytest.mark.parametrize("w", G.WIDTHS)
def test_pack_every_width_around_the_word_and_block_sizes(ctx, h, w):
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.05)
    ctx.set_grid(img, G.RES, (-3.0, 2.0), 128)
    want = G.pack(img, 128)
    np.testing.assert_array_equal(_read(ctx, UPLOADED), want)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), want)
    if h * w >= 64:
        assert want.any() and not want.all()


@pytest.mark.parametrize("occupied_below", [0, 1, 128, 255, 256])
@pytest.mark.parametrize("h,w", [(7, 33), (40, 257)])
def test_pack_thresholds_at_the_ends_of_the_u8_range(ctx, h, w, occupied_below):
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.05)
    assert set(G.SPECIAL) <= set(np.unique(img).tolist())
    ctx.set_grid(img, G.RES, (0.0, 0.0), occupied_below)
    want = G.pack(img, occupied_below)
    assert want.sum() == (img.astype(int) < occupied_below).sum() and (occupied_below > 0 or not want.any()) and (occupied_below < 256 or want.all())
    np.testing.assert_array_equal(_read(ctx, UPLOADED), want)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), want)


# ---- lookup -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [G.RES, G.RES_POW2])
@pytest.mark.parametrize("origin", [(-3.0, 2.0), (0.0, 0.0)])
def test_point_test_on_centres_corners_their_fp64_neighbours_outside_and_non_finite(ctx, res, origin):
    img = G.cell_map(40, 65, seed=40065, p=0.02)
    ctx.set_grid(img, res, origin, 128)
    active = G.pack(img, 128)
    pts = G.probe_points(active, res, *origin)
    want = G.occupied(active, res, origin[0], origin[1], pts)
    got = ctx.grid_occupied(pts)
    np.testing.assert_array_equal(got, want)
    assert want[-35:].all() and not want.all()
    # the same per-point answers at every batch size (one point, one wave less / exactly / more than one, more than a block)
    order = np.random.default_rng(5).permutation(len(pts))
    for E in (1, 63, 64, 65, 257):
        sel = order[:E] if E > 1 else order[np.flatnonzero(~want[order])[:1]]
        np.testing.assert_array_equal(ctx.grid_occupied(pts[sel]), want[sel], err_msg=f"E = {E}")
    assert ctx.grid_occupied(np.zeros((0, 2))).shape == (0,)
    # the test reads the ACTIVE bitmap
    ctx.inflate_grid(2.0 * res)
    act2 = G.dilate(active, G.inflate_thr(2.0 * res, res))
    np.testing.assert_array_equal(_read(ctx, ACTIVE), act2)
    np.testing.assert_array_equal(ctx.grid_occupied(pts), G.occupied(act2, res, origin[0], origin[1], pts))
    assert (act2 != active).any()


# ---- inflate ----------------------------------------------------------------------------------------------------------------------------
def _inflate_and_compare(ctx, img, res, radius, note):
    occ = G.pack(img, 128)
    thr = G.inflate_thr(radius, res)
    ctx.inflate_grid(radius)
    want = G.dilate(occ, thr)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), want, err_msg=f"{note}: radius {radius!r} at {res} (thr {thr})")
    np.testing.assert_array_equal(_read(ctx, UPLOADED), occ, err_msg=f"{note}: the upload changed")
    return want


@pytest.mark.parametrize("w", G.WIDTHS)
def test_inflate_equals_the_disc_dilation_cell_by_cell(ctx, w):
    h = 40
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.002)
    occ = G.pack(img, 128)
    ctx.set_grid(img, G.RES, (-3.0, 2.0), 128)
    free = {}
    for q in G.Q_CELLS:
        free[q] = (~_inflate_and_compare(ctx, img, G.RES, q * G.RES, f"{h} x {w}, q = {q!r}")).sum()
    assert _inflate_and_compare(ctx, img, G.RES, G.q_beyond(h, w) * G.RES, f"{h} x {w}, q beyond the map").all()
    assert free[40.0] == 0 and free[0.3] == (~occ).sum()                        # (h = 40: nothing is 40 cells from the outside)
    if w >= 31:
        assert free[0.3] > free[1.5] > free[7.3] > 0
        s2 = math.sqrt(2.0)
        assert free[s2 * (1.0 - 1e-12)] > free[s2 * (1.0 + 1e-12)]            # the diagonal neighbour: d2 = 2 on either side of q^2


@pytest.mark.parametrize("w", G.WIDTHS)
def test_inflate_is_strict_at_integer_radii(ctx, w):
    """res = 1 / 16: radius k res gives q = k exactly, and a cell at exactly d2 = k^2 from the nearest occupied cell stays free"""
    h = 40
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.002)
    occ = G.pack(img, 128)
    ctx.set_grid(img, G.RES_POW2, (0.0, 0.0), 128)
    for k in G.K_EXACT:
        assert G.inflate_thr(k * G.RES_POW2, G.RES_POW2) == k * k
        got = _inflate_and_compare(ctx, img, G.RES_POW2, k * G.RES_POW2, f"{h} x {w}, k = {k}")
        on_the_rim = G.dilate(occ, k * k + 1) & ~got                            # d2 == k^2 exactly
        assert on_the_rim.any() or w < 2 * k + 2


def test_inflate_by_forty_cells_on_a_two_block_map(ctx):
    h, w = 130, 257
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.0)
    ctx.set_grid(img, G.RES, (-3.0, 2.0), 128)
    want = _inflate_and_compare(ctx, img, G.RES, 40.0 * G.RES, "130 x 257")
    assert 0 < (~want).sum() < want.size // 4                                  # a free pocket is left, on both sides of column 256 or not


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def test_inflations_do_not_compound_and_the_footprint_adds(ctx):
    h, w, res = 40, 257, G.RES
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.002)
    occ = G.pack(img, 128)
    ctx.set_grid(img, res, (-3.0, 2.0), 128)
    r1, r2, rho = 0.36, 0.11, 0.17
    _inflate_and_compare(ctx, img, res, r1, "r1")
    small = _inflate_and_compare(ctx, img, res, r2, "r2 after r1: a fresh inflation of r2")
    assert (small != G.dilate(occ, G.inflate_thr(r1, res))).any()
    ctx.inflate_grid(0.0)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), occ)                      # 0 restores the upload
    ctx.inflate_grid(r2)
    ctx.set_footprint([-0.1, 0.2], rho)                                         # one dilation by r + rho
    both = G.dilate(occ, G.inflate_thr(r2 + rho, res))
    np.testing.assert_array_equal(_read(ctx, ACTIVE), both)
    assert (both != small).any()
    ctx.inflate_grid(r1)                                                        # a new inflation under the footprint: r1 + rho
    np.testing.assert_array_equal(_read(ctx, ACTIVE), G.dilate(occ, G.inflate_thr(r1 + rho, res)))
    ctx.inflate_grid(r2)
    ctx.set_footprint((), 0.0)                                                  # n_discs = 0: back to r
    np.testing.assert_array_equal(_read(ctx, ACTIVE), small)
    np.testing.assert_array_equal(_read(ctx, UPLOADED), occ)


def test_a_radius_beyond_the_cap_is_rejected_and_changes_nothing(ctx):
    h, w, res = 7, 33, G.RES
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.0)
    ctx.set_grid(img, res, (0.0, 0.0), 128)
    before = _inflate_and_compare(ctx, img, res, 0.06, "q = 1.2")
    assert not before.all()
    for radius in (8191.5 * res, 8192.0 * res, 1e6):                            # cap = ceil(q) + 1 > 8192 cells
        assert math.ceil(radius * (1.0 / res)) + 1 > 8192
        with pytest.raises(ValueError):
            ctx.inflate_grid(radius)
        np.testing.assert_array_equal(_read(ctx, ACTIVE), before)
    with pytest.raises(ValueError):
        ctx.set_footprint([0.0], 8192.0 * res)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), before)
    assert math.ceil(8190.5 * res * (1.0 / res)) + 1 == 8192                    # the largest cap: accepted, everything occupied
    assert _inflate_and_compare(ctx, img, res, 8190.5 * res, "cap 8192").all()


def test_a_new_grid_drops_the_inflation_and_the_clearance_map(ctx):
    img = G.cell_map(40, 65, seed=1, p=0.002)
    ctx.set_grid(img, G.RES, (0.0, 0.0), 128)
    ctx.inflate_grid(0.2)
    img2 = G.cell_map(7, 300, seed=2, p=0.002)
    ctx.set_grid(img2, G.RES, (0.0, 0.0), 128)
    np.testing.assert_array_equal(_read(ctx, ACTIVE), G.pack(img2, 128))
    np.testing.assert_array_equal(_read(ctx, UPLOADED), G.pack(img2, 128))
    assert "clearance" in _rejected(ctx, CLEARANCE)


def test_the_hooks_reject_what_they_cannot_answer():
    from f1tenth_planning_amd.runtime import Context, F1PError
    with Context(0) as c:
        for which in (UPLOADED, ACTIVE, CLEARANCE):
            assert "grid not set" in _rejected(c, which)
        with pytest.raises(F1PError) as ei:
            c.grid_occupied(np.zeros((3, 2)))
        assert ei.value.code == _abi.F1P_ESTATE
        assert c.grid_occupied(np.zeros((0, 2))).shape == (0,)                  # E = 0: a no-op, with or without a grid
        c.set_grid(G.cell_map(7, 33, seed=3), G.RES, (0.0, 0.0), 128)
        for which in (-1, 3):
            with pytest.raises(ValueError):
                c.grid_debug_read(which)
        assert c.lib.f1p_grid_debug_read(c.h, 1, None, None, None) == _abi.F1P_EINVAL
        out = np.empty(1, np.uint8)
        assert c.lib.f1p_grid_occupied_batch(c.h, None, 1, out.ctypes.data) == _abi.F1P_EINVAL
        assert c.lib.f1p_grid_occupied_batch(c.h, None, -1, None) == _abi.F1P_EINVAL
        cells = np.empty((7, 33), np.uint8)                                     # the two extra outputs are optional
        assert c.lib.f1p_grid_debug_read(c.h, 0, cells.ctypes.data, None, None) == _abi.F1P_OK
        np.testing.assert_array_equal(cells.astype(bool), c.grid_debug_read(0)[0])
        assert c.grid_debug_read(1)[2] == 0.0                                   # no clearance map yet: distance 0
        assert "clearance" in _rejected(c, CLEARANCE)


# ---- clearance --------------------------------------------------------------------------------------------------------------------------
_scene_cache = {}


def _corridor():
    """a closed 24 m raceline in a 1 m corridor on a 170 x 187 map (w no multiple of 32, five and a bit words per row)"""
    if not _scene_cache:
        rl = synth.make_raceline(seed=0, n_pts=121, spacing=0.2)
        rl[:, 2] = np.minimum(rl[:, 2], 4.0)
        img, origin = synth.make_grid(rl[:, :2], size=(170, 187), resolution=G.RES, half_width=0.5, wall_px=3)
        _scene_cache.update(rl=rl, img=img, origin=origin, occ=G.pack(img, 128))
    s = _scene_cache
    return s["rl"], s["img"], s["origin"], s["occ"]


def _install(c):
    rl, img, origin, occ = _corridor()
    c.set_waypoints(rl)
    c.set_grid(img, G.RES, origin, 128)
    return rl, occ


def _clear_equals_reference(c, active, note):
    """the clearance map, its distance D and the active bitmap it belongs to: map == clearance(active, D), cell by cell"""
    np.testing.assert_array_equal(_read(c, ACTIVE), active, err_msg=note)
    cells, pad_set, dist = c.grid_debug_read(CLEARANCE)
    assert pad_set and dist > 0.0
    want = G.clearance(active, dist)
    np.testing.assert_array_equal(cells, want, err_msg=f"{note}: D = {dist!r}")
    assert not (active & ~cells).any() and (cells != active).any() and not cells.all()
    return cells, dist


def _kmpc_plan(c, rl, E=16):
    p = synth.make_egos(rl, E, seed=4, pos_sigma=0.1)
    x0 = np.ascontiguousarray(np.column_stack([p[:, 0], p[:, 1], np.minimum(p[:, 3], 3.0), p[:, 2]]))
    c.kmpc_warm_reset()
    return c.kmpc_plan(x0, _abi.kmpc_cfg(horizon=8, n_rollouts=128), _abi.kmpc_sampler(seed=11, call=3, use_warm=True, sigma_accel=1.5, sigma_steer=0.15))


def test_clearance_map_of_a_kmpc_plan(ctx):
    rl, occ = _install(ctx)
    _rejected(ctx, CLEARANCE)
    ctx.kmpc_set_collision(True, 2)
    try:
        ctx.kmpc_set_mode(True)
        _kmpc_plan(ctx, rl)
        _, dist = _clear_equals_reference(ctx, occ, "kmpc, plain grid")
        assert dist >= 2.0                                                      # F1P_K4_CLEAR_CELLS: what the filter's proof needs
        r = 0.12
        ctx.inflate_grid(r)
        assert "stale" in _rejected(ctx, CLEARANCE)                             # the active bitmap changed under the map
        assert ctx.grid_debug_read(ACTIVE)[2] == 0.0
        _kmpc_plan(ctx, rl)
        _, dist = _clear_equals_reference(ctx, G.dilate(occ, G.inflate_thr(r, G.RES)), "kmpc, inflated grid")
        assert dist >= 2.0
    finally:
        ctx.kmpc_set_collision(False)


def _lattice_bound(cfg, r, res):
    """f1p_lattice_set_clearance's documented distance: r ds_cap + (sqrt 2 + 1) cells, ds_cap = 1.2 hypot(max look-ahead, max width) / (S - 1)"""
    la = max(abs(v) for v in cfg.lookahead[:cfg.n_lookahead]); wd = max(abs(v) for v in cfg.width[:cfg.n_width])
    return r * 1.2 * math.hypot(la, wd) / (cfg.n_stations - 1) / res + math.sqrt(2.0) + 1.0


def test_clearance_map_of_lattice_plans(ctx):
    rl, occ = _install(ctx)
    cfg = synth.bench_lattice_cfg(n_cand=64, n_stations=50)
    poses = synth.make_egos(rl, 64, seed=9, pos_sigma=0.1)
    try:
        ctx.lattice_set_mode(2)
        dists = {}
        for r in (1, 2):
            ctx.lattice_set_clearance(r)
            ctx.lattice_plan(poses, cfg)
            assert ctx.lattice_debug_queue(len(poses)).shape == (len(poses),)   # (the mixed schedule took the plan)
            _, dists[r] = _clear_equals_reference(ctx, occ, f"lattice, r = {r}")
            assert dists[r] >= _lattice_bound(cfg, r, G.RES)
        assert dists[2] > dists[1]                                              # (the map was rebuilt for the larger distance)
        rad = 0.1
        ctx.inflate_grid(rad)
        assert "stale" in _rejected(ctx, CLEARANCE)
        ctx.lattice_plan(poses, cfg)
        _, d = _clear_equals_reference(ctx, G.dilate(occ, G.inflate_thr(rad, G.RES)), "lattice, inflated grid")
        assert d >= _lattice_bound(cfg, 2, G.RES)
    finally:
        ctx.lattice_set_mode(1); ctx.lattice_set_clearance()


def test_clearance_maps_of_two_replicas_are_identical():
    from f1tenth_planning_amd.runtime import MultiContext
    rl, img, origin, occ = _corridor()
    cfg = synth.bench_lattice_cfg(n_cand=64, n_stations=50)
    poses = synth.make_egos(rl, 64, seed=9, pos_sigma=0.1)
    with MultiContext([0, 0]) as mc:
        mc.set_waypoints(rl); mc.set_grid(img, G.RES, origin, 128); mc.inflate_grid(0.1)
        for c in mc.ctxs:
            c.lattice_set_mode(2)
        mc.lattice_plan(poses, cfg)
        active = G.dilate(occ, G.inflate_thr(0.1, G.RES))
        maps = [_clear_equals_reference(c, active, f"replica {g}") for g, c in enumerate(mc.ctxs)]
        assert maps[0][1] == maps[1][1]
        np.testing.assert_array_equal(maps[0][0], maps[1][0])


# ---- the distance image's edges -----------------------------------------------------------------------------------------------------------
def _edt_case(name):
    if name == "cap 1":
        return G.cell_map(40, 65, seed=7, p=0.01), 1
    if name == "cap 8192 on 5 x 300":
        return G.cell_map(5, 300, seed=8, p=0.01), 8192
    if name == "300 x 1":
        return G.cell_map(300, 1, seed=9, p=0.02), 64
    if name == "1 x 300":
        return G.cell_map(1, 300, seed=10, p=0.02), 64
    if name == "all free":
        return np.full((40, 65), 254, np.uint8), 64
    assert name == "all occupied"
    return np.zeros((40, 65), np.uint8), 64


@pytest.mark.parametrize("name", ["cap 1", "cap 8192 on 5 x 300", "300 x 1", "1 x 300", "all free", "all occupied"])
def test_distance_image_edge_cases_bit_exact_vs_oracle(ctx, orc, name):
    img, cap = _edt_case(name)
    h, w = img.shape
    ctx.set_grid(img, G.RES, (-3.0, 2.0), 128)
    got = ctx.grid_distance(cap)
    # (the outside is occupied: no cell is farther than min(h, w) / 2 + 1 from it, so a cap beyond the map saturates nothing)
    want = orc.grid_distance(img, G.RES, 128, min(cap, max(h, w) + 1), nthreads=8)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.float32 and got.shape == (h, w) and (got[img < 128] == 0).all()
    if name == "cap 1":
        np.testing.assert_array_equal(got, np.where(img < 128, np.float32(0), np.float32(G.RES * 1.0)))
    if name == "all occupied":
        assert (got == 0).all()
    if name == "all free":                                                      # the distance to the outside: min(x + 1, w - x, y + 1, h - y) cells
        yy, xx = np.mgrid[0:h, 0:w]
        cells = np.minimum(np.minimum(xx + 1, w - xx), np.minimum(yy + 1, h - yy))
        np.testing.assert_array_equal(got, (G.RES * np.sqrt(cells.astype(np.float64) ** 2)).astype(np.float32))
