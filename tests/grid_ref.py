"""Plain numpy reference of the three bit-packed occupancy maps ("The maps, cell by cell"): the uploaded grid, its disc
dilation (the active bitmap), the clearance map of the active bitmap and the point test on it.  By definition, not by the two-pass scheme
of the kernels or of the oracle: a cell of a dilated map is the OR of the input over every integer offset inside the disc.  Validated on the
CPU by tests/test_grid_ref_host.py (against the oracle's exhaustive search and scipy's EDT) before tests/test_gpu_grid_cells.py holds
the device's maps against it.

Every map here is a bool array [h][w] in the IMAGE's row order (row 0 = top), True = occupied / bit set.  A disc is symmetric, so the
row order does not matter to the dilations; `occupied` applies the row flip."""
import math

import numpy as np

SPECIAL = (0, 1, 127, 128, 254, 255)              # the pixel values on either side of every threshold the tests use


def pack(img, occupied_below):
    """a cell is occupied iff its pixel value < occupied_below"""
    return np.asarray(img).astype(np.int64) < int(occupied_below)


def _or_of_shifts(occ, limit):
    """out(x, y) = OR of occ(x + dx, y + dy) over every integer (dx, dy) with dx^2 + dy^2 <= limit; cells outside the image are
    occupied.  One ring of occupied cells around the image stands for all of them: clamping an outside cell's coordinates to
    [-1, w] x [-1, h] gives a ring cell that is no farther from any cell of the image -- so |dx| <= w and |dy| <= h are enough."""
    occ = np.asarray(occ, bool)
    h, w = occ.shape
    pad = np.ones((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = occ
    out = np.zeros((h, w), bool)
    r = math.isqrt(limit) if limit >= 0 else -1
    for dy in range(-min(r, h), min(r, h) + 1):
        for dx in range(-min(r, w), min(r, w) + 1):
            if dx * dx + dy * dy > limit:
                continue
            y0, y1 = max(0, -1 - dy), min(h, h + 1 - dy)          # rows y of the image with 0 <= 1 + y + dy <= h + 1
            x0, x1 = max(0, -1 - dx), min(w, w + 1 - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] |= pad[1 + y0 + dy:1 + y1 + dy, 1 + x0 + dx:1 + x1 + dx]
    return out


def dilate(occ, thr):
    """occupied iff an occupied (or outside) cell lies at squared centre distance d2 < thr (STRICT), thr an integer"""
    thr = int(thr)
    return _or_of_shifts(occ, thr - 1)


def inflate_thr(radius, res):
    """the threshold of f1p_inflate_grid(radius): q = radius * (1.0 / res) in fp64, then d2 < q^2 <=> d2 < ceil(q^2) for integer d2"""
    q = float(radius) * (1.0 / float(res))
    return int(math.ceil(q * q))


def clearance(active, dist_cells):
    """bit set iff an occupied (or outside) cell of `active` lies at squared centre distance d2 <= floor(D^2) (INCLUSIVE)"""
    d = float(dist_cells)
    return _or_of_shifts(active, int(math.floor(d * d)))


def occupied(active, res, ox, oy, pts):
    """the point test: cell (floor((x - ox) * (1.0 / res)), floor((y - oy) * (1.0 / res))) in fp64, row gy counted from the BOTTOM
    of the image; a point outside the image or with a non-finite coordinate is occupied"""
    active = np.asarray(active, bool)
    h, w = active.shape
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    inv = 1.0 / float(res)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((pts[:, 0] - float(ox)) * inv)
        fy = np.floor((pts[:, 1] - float(oy)) * inv)
        inside = (fx >= 0.0) & (fy >= 0.0) & (fx < float(w)) & (fy < float(h))          # a NaN compares false: outside
    out = np.ones(len(pts), bool)
    gx, gy = fx[inside].astype(np.int64), fy[inside].astype(np.int64)
    out[inside] = active[h - 1 - gy, gx]
    return out


def cell_map(h, w, seed, p=0.01):
    """test image [h][w] u8: mostly free (254), a fraction p of single occupied cells (0) and as many "unknown" ones (205, free at 128),
    a wall from the left edge and one that TOUCHES THE RIGHT EDGE, and -- where the image has the room -- each of SPECIAL at least once"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 254, np.uint8)
    img[rng.random((h, w)) < p] = 0
    img[rng.random((h, w)) < p] = 205
    img[h // 3, : w // 4] = 0
    img[(2 * h) // 3, w - max(1, w // 4):] = 1
    n = min(len(SPECIAL), h * w)
    flat = img.reshape(-1)
    flat[rng.choice(h * w, n, replace=False)] = np.array(SPECIAL[:n], np.uint8)
    return img


def _probe_points(h, w, res, ox, oy, free_xy):
    kx, ky = np.arange(w + 1), np.arange(h + 1)
    cx, cy = ox + kx * res, oy + ky * res
    xs = np.concatenate([cx, np.nextafter(cx, np.inf), np.nextafter(cx, -np.inf)])
    ys = np.concatenate([cy, np.nextafter(cy, np.inf), np.nextafter(cy, -np.inf)])
    corners = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    mx, my = ox + (np.arange(-1, w + 1) + 0.5) * res, oy + (np.arange(-1, h + 1) + 0.5) * res    # centres, one cell beyond every side included
    centres = np.stack(np.meshgrid(mx, my, indexing="ij"), -1).reshape(-1, 2)
    odd = [1e300, -1e300, np.inf, -np.inf, np.nan]
    fx, fy = free_xy
    wild = [(v, fy) for v in odd] + [(fx, v) for v in odd] + [(a, b) for a in odd for b in odd]
    return np.concatenate([centres, corners, np.array(wild)])


def probe_points(active, res, ox, oy):
    """the lookup test's points on an h x w map: every cell centre and the centres one cell outside each side, every cell corner
    ox + k res and its two neighbours in fp64 (in each coordinate, all combinations), +-1e300 / +-inf / NaN in either coordinate"""
    h, w = active.shape
    free = np.argwhere(~np.asarray(active, bool))
    iy, ix = free[len(free) // 2]                                        # the centre of a free cell for the other coordinate
    return _probe_points(h, w, res, ox, oy, (ox + (ix + 0.5) * res, oy + (h - 1 - iy + 0.5) * res))


# the cases tests/test_grid_ref_host.py (CPU) and tests/test_gpu_grid_cells.py (device) share
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 513)
HEIGHTS = (1, 2, 7, 40)
RES = 0.05
RES_POW2 = 0.0625                                 # 1 / 16: radius k * res gives q = k exactly
Q_CELLS = (0.3, 0.5, 1.5, math.sqrt(2.0) * (1.0 - 1e-12), math.sqrt(2.0) * (1.0 + 1e-12), 7.3, 40.0)
K_EXACT = (1, 2, 3, 5)


def q_beyond(h, w):
    """a radius in cells larger than the map: everything is occupied"""
    return float(max(h, w)) + 2.5
