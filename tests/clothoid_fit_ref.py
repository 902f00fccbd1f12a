"""High-precision reference of the G1 clothoid fit (csrc/lattice_device.h g1_fit).

mpmath at 50 digits at generation time and in the host test; the GPU tests read tests/golden/g21_clothoid_fit.npz and need numpy only
(everything below `load_fixture` is numpy).  Nothing here shares a quadrature rule, a Taylor model or a starting point with the fit.

  normalise(x, y, th)      the library's normalisation taken literally: phi = atan2(y, x) rounded to double, the two differences 0 - phi
                           and th - phi formed in doubles, each reduced by whole multiples of the DOUBLE 2 pi evaluated exactly (the IEEE
                           remainder: an angle already in [-pi_d, pi_d] is left alone, atan2 = +-pi_d stays) -> (r, phi0, phi1)
  gh(A, phi0, delta)       g = int_0^1 sin(phi), h = int_0^1 cos(phi), g' = int_0^1 (tau^2 - tau) cos(phi), phi = A tau^2 + (delta - A) tau
                           + phi0: h + j g = exp(j phi0) xy(delta - A, 2 A, 1) with clothoid_ref.xy (Fresnel closed form, checked against
                           mpmath.quad to 1e-40), g' from the same closed form by two integrations by parts (central difference for small |A|)
  principal_root(phi0, phi1)  the branch, by a property no code under test shares: continue the root A = 0 of (0, 0) along the straight segment
                           to (phi0, phi1) in fixed steps with mp Newton, then polish to |g| < 1e-45 (times the larger angle where that is below 1).  The guess polynomial is never used.
  guess(phi0, phi1)        the published initial guess evaluated in mp: recorded as data (guess_err, the rule fit_moments picks at it)
  solve(x, y, th)          everything the fixture stores for one goal
"""
import math

DPS = 50
PI_D = math.pi
TWO_PI_D = 2.0 * math.pi
N_STEPS = 48
RULE_EDGES = (8.0, 14.0, 21.0, 29.0)          # fit_moments: 16 / 20 / 24 / 28 / 32 nodes; panels of the 32-node rule past 36
R_MIN = 1e-12


def _mp():
    import mpmath
    return mpmath


def reduce_angle(a):
    """IEEE remainder of the double a by the double 2 pi: exact, |result| <= pi_d, an angle in [-pi_d, pi_d] comes back unchanged"""
    return math.remainder(a, TWO_PI_D)


def chord_angle(x, y):
    """atan2(y, x) correctly rounded to double (it keeps the sign of a zero y: +-pi_d straight behind the ego)"""
    if y == 0.0:                                          # (mpf has no signed zero)
        return math.copysign(PI_D if math.copysign(1.0, x) < 0 else 0.0, y)
    mp = _mp()
    with mp.workdps(DPS):
        return float(mp.atan2(mp.mpf(y), mp.mpf(x)))


def normalise(x, y, th):
    """-> (r: mpf, the exact chord of the doubles; phi0, phi1: doubles) or None where the fit rejects (r <= 1e-12, anything not finite)"""
    mp = _mp()
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(th)):
        return None
    with mp.workdps(DPS):
        r = mp.sqrt(mp.mpf(x) ** 2 + mp.mpf(y) ** 2)
        if not r > mp.mpf(R_MIN):
            return None
    phi = chord_angle(x, y)
    return r, reduce_angle(0.0 - phi), reduce_angle(th - phi)


SMALL = 1e-6             # all of |A|, |phi0|, |delta| below this: the phase is small on the whole of [0, 1] and the series branch takes over


def _gh_series(mp, A, phi0, delta):
    """gh for a small phase, good to 1e-70 RELATIVE to the phase (the closed form is good to 1e-50 absolute, which near a straight goal says
    nothing about kappa0 and kappa'): sin and cos as Taylor polynomials in phi (up to phi^13: the next term is below 1e-84 of phi), phi a
    quadratic in tau, every power integrated over [0, 1] exactly"""
    def mul(p, q):
        out = [mp.mpf(0)] * (len(p) + len(q) - 1)
        for i, a in enumerate(p):
            for k, b_ in enumerate(q):
                out[i + k] += a * b_
        return out
    integ = lambda p: sum(c / (i + 1) for i, c in enumerate(p))   # noqa: E731
    phi, u = [phi0, delta - A, A], [mp.mpf(0), mp.mpf(-1), mp.mpf(1)]
    g = h = dg = mp.mpf(0)
    pw = [mp.mpf(1)]                                      # phi^n
    for n in range(14):
        c = (-1) ** (n // 2) / mp.factorial(n)
        if n % 2:
            g += c * integ(pw)
        else:
            h += c * integ(pw)
            dg += c * integ(mul(pw, u))
        pw = mul(pw, phi)
    return g, h, dg


def gh(A, phi0, delta):
    """(g, h, g') at A (mpf), phi0 and delta the exact values handed in"""
    import clothoid_ref as C
    mp = _mp()
    with mp.workdps(DPS + 30):
        A, phi0, delta = mp.mpf(A), mp.mpf(phi0), mp.mpf(delta)
        if max(abs(A), abs(phi0), abs(delta)) < SMALL:
            return _gh_series(mp, A, phi0, delta)
        b = delta - A

        def i0(a_):
            x, y = C.xy(delta - a_, 2 * a_, 1.0)
            return mp.expj(phi0) * mp.mpc(x, y)
        z = i0(A)
        if abs(A) >= mp.mpf("0.01"):
            # d/dtau e^{j phi} = j (2 A tau + b) e^{j phi}:  I1 = int tau e^{j phi}, I2 = int tau^2 e^{j phi} by parts
            e0, e1 = mp.expj(phi0), mp.expj(phi0 + delta)
            i1 = ((e1 - e0) / 1j - b * z) / (2 * A)
            i2 = ((e1 - z) / 1j - b * i1) / (2 * A)
            dg = (i2 - i1).real                              # d/dA (h + j g) = j (I2 - I1)
        else:
            hh = mp.mpf(10) ** -18
            dg = (i0(A + hh).imag - i0(A - hh).imag) / (2 * hh)
        return z.imag, z.real, dg


def gh_quad(A, phi0, delta):
    """(g, h, g') by mpmath.quad of the defining integrals: the host test's second opinion"""
    mp = _mp()
    with mp.workdps(DPS):
        A, phi0, delta = mp.mpf(A), mp.mpf(phi0), mp.mpf(delta)
        ph = lambda t: A * t * t + (delta - A) * t + phi0   # noqa: E731
        cuts = mp.linspace(0, 1, max(2, int(abs(A) + abs(delta - A)) + 2))
        sc = min(mp.mpf(1), max(abs(A), abs(phi0), abs(delta), mp.mpf(10) ** -400))   # (quad stops on an absolute error: keep the integrand O(1))
        return (sc * mp.quad(lambda t: mp.sin(ph(t)) / sc, cuts), mp.quad(lambda t: mp.cos(ph(t)), cuts),
                mp.quad(lambda t: (t * t - t) * mp.cos(ph(t)), cuts))


def principal_root(phi0, phi1, steps=N_STEPS):
    """A* (mpf): the root of g that continues A = 0 at (0, 0) along the segment t (phi0, phi1), t = k / steps"""
    mp = _mp()
    with mp.workdps(DPS + 30):
        p0, p1 = mp.mpf(phi0), mp.mpf(phi1)
        scale = min(mp.mpf(1), max(abs(p0), abs(p1)))       # tolerances relative to the angles: a nearly straight goal keeps its digits
        if scale == 0:
            return mp.mpf(0)
        A, last = mp.mpf(0), mp.mpf(0)
        for k in range(1, steps + 1):
            t = mp.mpf(k) / steps
            a, d = p0 * t, (p1 - p0) * t
            A, last = 2 * A - last, A                      # predictor: the secant through the last two roots
            for _ in range(30):
                g, _, dg = gh(A, a, d)
                step = g / dg
                A -= step
                if abs(step) < scale * mp.mpf(10) ** (-12 if k < steps else -30):
                    break
            else:
                raise ArithmeticError("continuation did not converge")
        for _ in range(4):
            g, _, dg = gh(A, p0, p1 - p0)
            if abs(g) < scale * mp.mpf(10) ** -45:
                break
            A -= g / dg
        else:
            raise ArithmeticError("polish did not reach 1e-45")
        return A


GUESS = (2.989696028701907, 0.716228953608281, -0.458969738821509, -0.502821153340377, 0.261062141752652, -0.045854475238709)


def guess(phi0, phi1):
    """the published initial guess (Bertolazzi & Frego 2015, table 1) in mp, X = phi0 / pi_d, Y = phi1 / pi_d as the fit scales them"""
    mp = _mp()
    with mp.workdps(DPS):
        c = [mp.mpf(v) for v in GUESS]
        p0, p1 = mp.mpf(phi0), mp.mpf(phi1)
        X, Y = p0 / mp.mpf(PI_D), p1 / mp.mpf(PI_D)
        xy = X * Y
        return (p0 + p1) * (c[0] + xy * (c[1] + xy * c[2]) + (c[3] + xy * c[4]) * (X * X + Y * Y) + c[5] * (X ** 4 + Y ** 4))


def rule_of(exc):
    """index of the Gauss-Legendre rule fit_moments picks at phase excursion exc: 0..4 (16, 20, 24, 28, 32 nodes), 5 = panels"""
    for i, e in enumerate(RULE_EDGES):
        if exc <= e:
            return i
    return 4 if exc <= 36.0 else 5


def solve(x, y, th):
    """one goal -> dict(expect_ok, phi0, phi1, A, k0, dk, L: doubles; dg = |g'(A*)|, guess_err, exc (of the guess), rule, ambiguous, singular).
    ambiguous: both angles within 1e-9 of the seam with the same sign -- the corner phi0 = phi1 = +-pi_d, where two mirrored roots have the
    same |A| and the last bit of an angle picks one.  singular: both within 1e-6 of it with opposite signs -- the corners (-+pi, +-pi), a full
    circle back through the start: h -> 0, L = r / h is unbounded and neither L nor ok is pinned by anything but rounding."""
    mp = _mp()
    out = dict(expect_ok=0, phi0=0.0, phi1=0.0, A=0.0, k0=0.0, dk=0.0, L=0.0, dg=0.0, guess_err=0.0, exc=0.0, rule=-1, ambiguous=0, singular=0)
    n = normalise(x, y, th)
    if n is None:
        return out
    r, phi0, phi1 = n
    with mp.workdps(DPS + 30):
        delta = mp.mpf(phi1) - mp.mpf(phi0)
        A = principal_root(phi0, phi1)
        _, h, dg = gh(A, phi0, delta)
        if not h > 0:
            raise ArithmeticError("the continued root has no positive length")
        L = r / h
        Ag = guess(phi0, phi1)
        exc = abs(Ag) + abs(delta - Ag)
        out.update(expect_ok=1, phi0=phi0, phi1=phi1, A=float(A), k0=float((delta - A) / L), dk=float(2 * A / (L * L)), L=float(L),
                   dg=float(abs(dg)), guess_err=float(abs(A - Ag)), exc=float(exc), rule=rule_of(float(exc)),
                   ambiguous=int(min(abs(phi0), abs(phi1)) >= PI_D - 1e-9 and phi0 * phi1 > 0),
                   singular=int(min(abs(phi0), abs(phi1)) >= PI_D - 1e-6 and phi0 * phi1 < 0))
    return out


# ---- the whole square at once, in doubles: the generator's scan for the goals of largest guess error (numpy) -----------------------------
def scan_roots(P0, P1, steps=N_STEPS):
    """principal_root's continuation in float64 for arrays of (phi0, phi1): an 80-node Gauss-Legendre rule on [0, 1] (exact to rounding for
    the phases of the square), Newton to 1e-13.  Good to ~1e-13: it ranks goals by guess_err, it pins nothing."""
    import numpy as np
    x, w = np.polynomial.legendre.leggauss(80)
    tau, w = 0.5 * (x + 1.0), 0.5 * w
    u = tau * tau - tau
    P0, P1 = np.asarray(P0, dtype=np.float64), np.asarray(P1, dtype=np.float64)
    A, last = np.zeros_like(P0), np.zeros_like(P0)
    for k in range(1, steps + 1):
        t = k / steps
        a, d = (P0 * t)[..., None], ((P1 - P0) * t)[..., None]
        A, last = 2.0 * A - last, A
        for _ in range(12):
            ph = A[..., None] * u + d * tau + a
            step = (np.sin(ph) * w).sum(-1) / (np.cos(ph) * u * w).sum(-1)
            A = A - step
            if np.abs(step).max() < 1e-13:
                break
    return A


def guess_np(P0, P1):
    import numpy as np
    c = GUESS
    X, Y = np.asarray(P0) / PI_D, np.asarray(P1) / PI_D
    xy = X * Y
    return (P0 + P1) * (c[0] + xy * (c[1] + xy * c[2]) + (c[3] + xy * c[4]) * (X * X + Y * Y) + c[5] * (X ** 4 + Y ** 4))


# ---- the fixture and the bars, shared by the host and the GPU tests: numpy only -------------------------------------------
FWD_BAR = 1e-12          # k0 L*, dk L*^2, L / L*, A = dk L^2 / 2: the project's bar for values through the device's sin / cos
BWD_BAR = 1e-14          # |A - A*| |g'(A*)|: 2e-15 claimed model remainder + 32 fma roundings of O(1 / 32) terms + 1 ulp of sincos ~ 6e-15
ORACLE_BAR = 1e-11       # the CPU restatements stop at |g| <= 1e-13: 1e-13 / min |g'| (0.070), doubled for dk L^2 = 2 A
SUBNORMAL = 2.0 ** -1074
FAMILIES = ("square", "worst-guess", "rule-switch", "scale", "small-r", "heading", "near-straight", "reject", "class")


def load_fixture(golden_dir):
    """g21_clothoid_fit.npz -> dict of arrays over the n goals: goals [n, 3], expect_ok, ambiguous, singular, mirror_of (-1: an original), family (index
    into FAMILIES), rule, phi [n, 2], A, k0, dk, L, dg, guess_err, exc; a mirror's A, k0, dk are its original's negated (exactly: every step of
    the normalisation is odd); class_start, class_end [6, 3]: the end poses behind the goals of the family "class", in its order"""
    import os
    import numpy as np
    f = np.load(os.path.join(golden_dir, "g21_clothoid_fit.npz"), allow_pickle=False)
    fx = {k: f[k] for k in f.files}
    fx["expect_ok"] = fx["expect_ok"].astype(bool)
    fx["ambiguous"] = fx["ambiguous"].astype(bool)
    fx["singular"] = fx["singular"].astype(bool)
    return fx


def fit_errors(k0, dk, L, fx, sel=None):
    """device (or oracle) parameters against the fixture on the goals sel (default: expected ok, neither ambiguous nor singular) ->
    (fwd [m, 4]: errors of k0 L*, dk L*^2, L / L*, A in scale-free units, the dk column less the subnormal allowance; bwd [m]: |A - A*| |g'(A*)|;
    idx [m]).  A is recovered from the parameters under test as dk L^2 / 2; long double keeps r = 1e150 (L^2 ~ 1e302) and the
    recovery's own roundings out of the figures."""
    import numpy as np
    ld = np.longdouble
    if sel is None:
        sel = fx["expect_ok"] & ~fx["ambiguous"] & ~fx["singular"]
    idx = np.nonzero(sel)[0]
    k0, dk, L = (np.asarray(v, dtype=np.float64)[idx].astype(ld) for v in (k0, dk, L))
    Ls, k0s, dks, As = (fx[k][idx].astype(ld) for k in ("L", "k0", "dk", "A"))
    A = dk * L * L / 2
    e_dk = np.abs(dk - dks) * Ls * Ls
    sub = (np.abs(fx["dk"][idx]) < 2.0 ** -1022) | (np.abs(np.asarray(dk, dtype=np.float64)) < 2.0 ** -1022)
    e_dk = np.where(sub, np.maximum(e_dk - ld(SUBNORMAL) * Ls * Ls, 0), e_dk)
    e_A = np.abs(A - As)
    e_A = np.where(sub, np.maximum(e_A - ld(SUBNORMAL) * Ls * Ls, 0), e_A)
    fwd = np.stack([np.abs(k0 - k0s) * Ls, e_dk, np.abs(L / Ls - 1), e_A], axis=1).astype(np.float64)
    return fwd, (e_A * fx["dg"][idx]).astype(np.float64), idx


def interleave(fx):
    """an order of the fixture's goals in which neighbours differ: every class (rule 0..4, rejected) is spread evenly over the whole order
    (goal i of a class of m sits at (i + 1/2) / m), so that four consecutive goals -- one wave of the refinement, 16 lanes per entry -- hold
    different quadrature rules, and rejected goals turn up all along -> permutation [n]"""
    import numpy as np
    cls = np.where(fx["expect_ok"], fx["rule"], 5)
    pos = np.empty(len(cls))
    for c in range(6):
        m = np.nonzero(cls == c)[0]
        pos[m] = (np.arange(len(m)) + 0.5) / max(len(m), 1)
    return np.argsort(pos, kind="stable")
