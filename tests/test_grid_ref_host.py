"""tests/grid_ref.py, the plain numpy reference of the occupancy bitmaps, validated on the CPU before tests/test_gpu_grid_cells.py holds
the device's maps against it: its dilation against the oracle's exhaustive search (orc.inflate_image) on the maps and radii of the device
test, the distances its thresholds imply against scipy's EDT, its point test against orc.cell_occupied."""
import math

import numpy as np
import pytest

import grid_ref as G


def _radii(h, w):
    """(res, radius) of the device test's inflations on an h x w map"""
    out = [(G.RES, q * G.RES) for q in G.Q_CELLS + (G.q_beyond(h, w),)]
    return out + [(G.RES_POW2, k * G.RES_POW2) for k in G.K_EXACT]


@pytest.mark.parametrize("h,w", [(40, w) for w in G.WIDTHS] + [(130, 257)])
def test_dilate_equals_the_oracles_exhaustive_search(orc, h, w):
    img = G.cell_map(h, w, seed=h * 1000 + w, p=0.002 if h == 40 else 0.0)
    occ = G.pack(img, 128)
    for res, radius in _radii(h, w) if h == 40 else [(G.RES, 40.0 * G.RES)]:
        thr = G.inflate_thr(radius, res)
        want = orc.inflate_image(img, res, 128, radius, nthreads=8) == 0
        np.testing.assert_array_equal(G.dilate(occ, thr), want, err_msg=f"{h} x {w}, radius {radius!r} at {res}: thr {thr}")


def test_thresholds_of_the_radii():
    """the strict rule in numbers: q = k exactly leaves d2 = k^2 free; sqrt 2 on either side decides the diagonal neighbour"""
    for k in G.K_EXACT:
        assert G.inflate_thr(k * G.RES_POW2, G.RES_POW2) == k * k
    thr = [G.inflate_thr(q * G.RES, G.RES) for q in G.Q_CELLS]
    assert thr == [1, 1, 3, 2, 3, 54, 1600]
    occ = np.zeros((15, 15), bool); occ[7, 7] = True
    inner = lambda m: m[4:-4, 4:-4]                                     # noqa: E731  (beyond the reach of the outside: d2 >= 25 there)
    assert inner(G.dilate(occ, 1)).sum() == 1 and inner(G.dilate(occ, 2)).sum() == 5 and inner(G.dilate(occ, 3)).sum() == 9
    assert inner(G.dilate(occ, 9)).sum() == 25 and inner(G.dilate(occ, 10)).sum() == 29       # d2 = 9: (+-3, 0), (0, +-3)
    # clearance is inclusive: D = 2 takes d2 = 4 in, D = 2.3 also d2 = 5
    assert inner(G.clearance(occ, 2.0)).sum() == 13 and inner(G.clearance(occ, 2.3)).sum() == 21
    np.testing.assert_array_equal(G.clearance(occ, 2.0), G.dilate(occ, 5))


@pytest.mark.parametrize("h,w,p", [(40, 65, 0.002), (7, 33, 0.0), (40, 257, 0.002), (1, 31, 0.0), (130, 257, 0.0)])
def test_implied_distances_equal_scipys_edt(h, w, p):
    """d2 < thr for every integer thr up to 12^2 + 1 <=> the dilation at thr: the distance each cell takes from the family of dilations is
    scipy's exact EDT of the mask padded with occupied cells"""
    from scipy import ndimage
    occ = G.pack(G.cell_map(h, w, seed=h * 1000 + w, p=p), 128)
    ring = 13                                                            # outside cells up to the largest distance looked at
    pad = np.zeros((h + 2 * ring, w + 2 * ring), bool)
    pad[ring:-ring, ring:-ring] = ~occ
    edt = ndimage.distance_transform_edt(pad)[ring:-ring, ring:-ring]
    d2 = np.rint(edt * edt).astype(np.int64)
    assert np.abs(edt - np.sqrt(d2)).max() < 1e-9
    implied = np.full((h, w), 12 * 12 + 1, np.int64)                     # the smallest thr - 1 at which the cell is taken, saturated
    for thr in range(12 * 12 + 1, 0, -1):
        implied[G.dilate(occ, thr)] = thr - 1
    np.testing.assert_array_equal(implied, np.minimum(d2, 12 * 12 + 1))
    np.testing.assert_array_equal(np.sqrt(implied)[implied <= 144], edt[implied <= 144])
    for dist in (1.0, 2.0, 2.5, 3.96, 5.51, 12.0):
        np.testing.assert_array_equal(G.clearance(occ, dist), edt <= dist)


@pytest.mark.parametrize("res", [G.RES, G.RES_POW2])
@pytest.mark.parametrize("origin", [(-3.0, 2.0), (0.0, 0.0)])
def test_occupied_equals_the_oracles_cell_rule(orc, res, origin):
    img = G.cell_map(40, 65, seed=40065, p=0.02)
    active = G.pack(img, 128)
    pts = G.probe_points(active, res, *origin)
    got = G.occupied(active, res, origin[0], origin[1], pts)
    g, keep = orc.make_grid(img, res, origin[0], origin[1], 128)
    want = np.array([orc.cell_occupied(g, float(x), float(y)) for x, y in pts])
    del keep
    np.testing.assert_array_equal(got, want)
    assert got[-35:].all()                                               # not finite or 1e300 away: occupied
    n_c = 67 * 42
    inside = got[:n_c].reshape(67, 42)[1:-1, 1:-1]                       # the centres come back as the image, transposed and flipped
    np.testing.assert_array_equal(inside.T[::-1], active)
    assert got[:n_c].reshape(67, 42)[0].all() and got[:n_c].reshape(67, 42)[-1].all() and got[:n_c].reshape(67, 42)[:, 0].all()
    assert not got.all() and math.isfinite(pts[0, 0])
