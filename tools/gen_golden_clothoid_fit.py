#!/usr/bin/env python3
"""tests/golden/g21_clothoid_fit.npz: goals for the G1 clothoid fit with the 50-digit answers of tests/clothoid_fit_ref.py.

Families (FAMILIES of clothoid_fit_ref; every goal is followed by its mirror (x, -y, -theta), whose answers are the original's negated):
  square         a 33 x 33 grid over the normalised square (phi0, phi1) in [-pi_d, pi_d]^2 at r = 1, edges included (one half of the grid as
                 originals, the other half as their mirrors).  phi0 = +-pi_d is a goal straight behind the ego with y = -+0.0; phi1 = +-pi_d
                 is kept exact where the chord angle is 0 or +-pi_d and moved 1e-9 inside elsewhere (there the seam would hang on the last
                 bit of the device's atan2, which the fit does not promise).  The corner phi0 = phi1 = +-pi_d is flagged ambiguous, the
                 corners (-+pi_d, +-pi_d) -- a full circle, L unbounded -- singular (clothoid_fit_ref.solve).
  worst-guess    the 64 goals of largest |A* - A_guess| in a 241 x 241 scan of the square (float64 continuation, clothoid_fit_ref.scan_roots)
  rule-switch    goals on rays of the square placed by bisection so that the phase excursion of the guess lies within 1e-6 either side of
                 fit_moments' thresholds 8, 14, 21, 29 (40 rays for the outer two, 20 for the inner two: every rule gets 40 goals or more)
  scale          8 angle pairs at r = 1e-11 .. 1e150 (1e101 and 1e150 take g1_begin's hypot path), one pair small enough for a subnormal kappa'
  small-r        the same pairs at r = 1e-100 .. 1e-300: below the fit's 1e-12 m, rejected
  heading        theta + 2 pi_d k, |theta| past 1e6 (remainder_2pi's library path), theta = +-pi_d and its neighbours, goals behind the ego
                 with y = +-0, +-5e-324, +-1e-300, +-1e-12 |x|, and differences within an ulp of an odd multiple of pi_d (the seam correction)
  near-straight  (r, 0, 0) and three goals a hair off it
  reject         r <= 1e-12, NaN / inf in each slot
  class          the goals Clothoid.G1Hermite forms in the start frame for 6 pairs of poses off the origin (class_start, class_end)
Byte-for-byte reproducible; a few minutes of mpmath."""
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clothoid_fit_ref as F  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_clothoid_fit.npz")
PI = F.PI_D
FAM = {n: i for i, n in enumerate(F.FAMILIES)}


def from_angles(r, p0, p1):
    """the goal whose normalisation gives (p0, p1) up to rounding: chord angle -p0 (y = a signed zero straight behind), heading p1 - p0"""
    phi = -p0
    if abs(p0) == PI:
        x, y = -r, math.copysign(0.0, phi)
    else:
        x, y = r * math.cos(phi), r * math.sin(phi)
        if phi == 0.0:
            y = 0.0
    if abs(p1) == PI and phi not in (0.0, PI, -PI):
        p1 = math.copysign(PI - 1e-9, p1)
    return x, y, p1 + phi


def exc_of(goal):
    n = F.normalise(*goal)
    ag = float(F.guess_np(n[1], n[2]))
    return abs(ag) + abs((n[2] - n[1]) - ag)


def square():
    grid = np.linspace(-PI, PI, 33)
    grid[16] = 0.0
    out = []
    for i, p0 in enumerate(grid):
        for k, p1 in enumerate(grid):
            if (i, k) > (16, 16) or (i, k) == (16, 16):        # this half and the centre; the mirrors are the other half
                out.append(from_angles(1.0, float(p0), float(p1)))
    return out


def worst_guess():
    g = np.linspace(-PI, PI, 241)
    P0, P1 = np.meshgrid(g, g, indexing="ij")
    err = np.abs(F.scan_roots(P0, P1) - F.guess_np(P0, P1))
    order = np.argsort(-err, axis=None, kind="stable")[:64]
    i, k = np.unravel_index(order, err.shape)
    print(f"241 x 241 scan: largest |A* - A_guess| {err.max():.6f} at (phi0, phi1) = ({P0[i[0], k[0]]:.4f}, {P1[i[0], k[0]]:.4f}); "
          f"the 64th largest {err[i[-1], k[-1]]:.6f}")
    return [from_angles(1.0, float(P0[a, b]), float(P1[a, b])) for a, b in zip(i, k)]


def rule_switch():
    out = []
    for thr, want in zip(F.RULE_EDGES, (40, 20, 20, 40)):
        got, j = 0, 0
        while got < want:
            psi = 2.0 * math.pi * ((j * 0.6180339887498949) % 1.0)
            j += 1
            cs, sn = math.cos(psi), math.sin(psi)
            tmax = (PI - 1e-3) / max(abs(cs), abs(sn))
            goal = lambda t: from_angles(1.0, t * cs, t * sn)       # noqa: E731
            ts = np.linspace(0.0, tmax, 400)
            ex = np.array([exc_of(goal(t)) for t in ts])
            cross = np.nonzero((ex[:-1] < thr) & (ex[1:] > thr))[0]
            if len(cross) == 0:
                continue
            lo, hi = float(ts[cross[0]]), float(ts[cross[0] + 1])
            while max(exc_of(goal(hi)) - thr, thr - exc_of(goal(lo))) > 5e-7:
                mid = 0.5 * (lo + hi)
                if abs(exc_of(goal(mid)) - thr) < 1e-9:          # too near the threshold for either side: cut elsewhere
                    mid = lo + 0.3 * (hi - lo)
                if exc_of(goal(mid)) < thr:
                    lo = mid
                else:
                    hi = mid
            for t in (lo, hi):
                assert 1e-10 < abs(exc_of(goal(t)) - thr) < 1e-6
                out.append(goal(t))
            got += 1
    return out


PAIRS = ((0.3, -0.2), (1.2, 0.9), (-2.0, 1.5), (2.8, -2.9), (0.01, 0.02), (-1.0, -3.0), (0.5, 2.5), (1e-9, -3e-9))


def scale(rs):
    return [from_angles(r, p0, p1) for r in rs for p0, p1 in PAIRS]


def heading():
    out = []
    bases = ((1.5, 0.0), (0.0, 2.0), (1.0, 0.7), (-0.8, 0.5))
    for x, y in bases:
        for th in (0.3, -2.9):
            for k in (1, -1, 3, -3, 20, -20, 100000, -100000):
                out.append((x, y, th + F.TWO_PI_D * k))
        for th in (1e6 + 0.3, -(1e6 + 0.3), 1.234567e7, -1.234567e7, 1e9 + 0.5, 1e15, -1e15, 1e300):
            out.append((x, y, th))
    up = lambda v, n: v if n == 0 else up(math.nextafter(v, math.copysign(math.inf, n)), n - (1 if n > 0 else -1))   # noqa: E731
    for s in (1.0, -1.0):                                          # theta = +-pi_d and its two neighbours, the chord along +x
        for n in (-1, 0, 1):
            out.append((1.5, 0.0, up(s * PI, n)))
    for x in (-2.0,):                                              # straight behind the ego: the sign of a zero (or vanishing) y picks the side
        for th in (0.3, 2.5):
            for y in (0.0, 5e-324, 1e-300, 1e-12 * abs(x)):
                out += [(x, y, th), (x, -y, th)]
    for k in (1, -2, 20, 1000, -3001):                             # th - phi within an ulp of an odd multiple of pi_d: n = rint(.) may go either way
        for n in (-1, 0, 1):
            out.append((1.5, 0.0, up((2 * k + 1) * PI, n)))
            out.append((-1.5, 0.0, up(2 * k * PI, n) + 0.0))
            out.append((-1.5, -0.0, up(2 * k * PI, n) + 0.0))
    keep = []
    for g in out:                                                  # an exact tie of the remainder has no side to pin: none is kept
        phi = F.chord_angle(g[0], g[1])
        _, p0, p1 = F.normalise(*g)
        if abs(p1) == PI and abs(g[2] - phi) > PI:
            print("dropped (tie of the remainder):", g)
            continue
        keep.append(g)
    return keep


CLASS_START = ((1.0, 2.0, 0.5), (-3.0, 0.7, -2.0), (10.0, -4.0, 3.0), (0.3, 0.3, -0.4), (-50.0, 20.0, 1.2), (2.5, -1.5, 2.9))
CLASS_END = ((2.5, 2.4, 1.4), (-3.5, 2.0, 1.0), (8.0, -4.5, -2.5), (0.35, 0.1, 0.2), (-48.0, 25.0, -1.0), (1.0, -1.0, -3.0))


def class_goals():
    """utils/clothoid.py G1Hermite's own expression for the goal in the start frame"""
    out = []
    for (x0, y0, theta0), (x1, y1, theta1) in zip(np.array(CLASS_START), np.array(CLASS_END)):
        c, s = np.cos(theta0), np.sin(theta0)
        dx, dy = x1 - x0, y1 - y0
        out.append((c * dx + s * dy, -s * dx + c * dy, theta1 - theta0))
    return out


def main():
    fam, goals = [], []

    def add(name, gs):
        for g in gs:
            fam.append(FAM[name]); goals.append(tuple(float(v) for v in g))
    add("square", square())
    add("worst-guess", worst_guess())
    add("rule-switch", rule_switch())
    add("scale", scale((1e-11, 1e-9, 1e-6, 1e-3, 1e3, 1e6, 1e99, 1e101, 1e150)) + [(1.1e-12, 0.0, 0.2)])
    add("small-r", scale((1e-100, 1e-150, 1e-160, 1e-200, 1e-300)))
    add("heading", heading())
    add("near-straight", [(r, 0.0, 0.0) for r in (2.0, 0.084, 5.0, 1e-11, 1e101)] + [(2.0, 1e-300, 0.0), (2.0, 1e-17, 1e-17), (2.0, 1e-8, -1e-8)])
    nan, inf = math.nan, math.inf
    add("reject", [(0.0, 0.0, 0.3), (1e-12, 0.0, 0.0), (1e-13, 0.0, 0.1), (6e-13, 6e-13, 0.1), (nan, 1.0, 0.0), (1.0, nan, 0.0), (1.0, 1.0, nan),
                   (inf, 1.0, 0.0), (-inf, 1.0, 0.0), (1.0, inf, 0.0), (1.0, -inf, 0.0), (1.0, 1.0, inf), (1.0, 1.0, -inf), (inf, inf, 0.0)])
    add("class", class_goals())
    keys = ("expect_ok", "ambiguous", "singular", "rule", "phi0", "phi1", "A", "k0", "dk", "L", "dg", "guess_err", "exc")
    rows = {k: [] for k in keys}
    G, family, mirror_of = [], [], []
    for i, (f, g) in enumerate(zip(fam, goals)):
        s = F.solve(*g)
        if i % 200 == 0:
            print(f"{i} / {len(goals)}", flush=True)
        for sign, src in ((1.0, -1), (-1.0, len(G))):
            G.append((g[0], sign * g[1], sign * g[2])); family.append(f); mirror_of.append(src)
            for k in keys:
                rows[k].append(sign * s[k] if k in ("phi0", "phi1", "A", "k0", "dk") else s[k])
    a = {k: np.array(v, dtype=np.int32 if k in ("expect_ok", "ambiguous", "singular", "rule") else np.float64) for k, v in rows.items()}
    ok = a["expect_ok"] == 1
    assert (np.array(family)[~ok] >= FAM["small-r"]).all() and ok[np.array(family) < FAM["small-r"]].all()
    sq = np.array(family) == FAM["square"]
    assert sq.sum() == 33 * 33 + 1 and a["ambiguous"].sum() >= 2
    print(f"{len(G)} goals, {int(ok.sum())} with a fit, {int(a['ambiguous'].sum())} ambiguous, {int(a['singular'].sum())} singular; per rule {np.bincount(a['rule'][ok], minlength=5).tolist()}; "
          f"largest guess_err {a['guess_err'].max():.6f}, largest exc {a['exc'].max():.3f}, smallest |g'| {a['dg'][ok].min():.4f}")
    np.savez_compressed(OUT, goals=np.array(G), family=np.array(family, np.int32), mirror_of=np.array(mirror_of, np.int32),
                        class_start=np.array(CLASS_START), class_end=np.array(CLASS_END),
                        phi=np.column_stack([a.pop("phi0"), a.pop("phi1")]), **a)
    print("written", os.path.normpath(OUT), os.path.getsize(OUT))


if __name__ == "__main__":
    main()
