"""High-precision reference of the lattice planner's two candidate generators and of its cost.

Plain functions in mpmath arithmetic (50 digits, more where a closed form cancels); nothing here shares a loop, a series or a table with
csrc/lattice_device.h or oracle/f1p_oracle.c.  tools/gen_golden_clothoid_eval.py evaluates them into tests/golden/g19_clothoid_eval.npz;
the GPU tests read that file.  `cost` and `nsub` are plain arithmetic on whatever numbers they are given and need no mpmath.

  xy(k0, dk, s)             int_0^s exp(j (k0 u + dk u^2 / 2)) du by completing the square into Fresnel C / S
  rows(k0, dk, L, S)        the sample_traj layout (utils/utils.py:286-295): s_i = i * (L / max(S - 1, 1)), (x, y, theta, |kappa|)
  theta_kappa(k0, dk, L, S)  columns 3 and 4 of rows() in exact rational arithmetic (no mpmath)
  nsub(k0, dk, L, S)        pieces per station interval by interval_setup's two rules, WITHOUT its cap (labels only)
  cubic_rows(gx, gy, gth, S)  the cubic generator from its definition (include/f1p.h), with the conditioning terms of |kappa|
  cost(rows, L, cfg, prev)  DESIGN.md 3, item 6
"""
import math
from fractions import Fraction

DPS = 50


def _mp():
    import mpmath
    return mpmath


def _extra_digits(k0, dk, s):
    """digits the Fresnel form loses: its arguments grow like k0 / sqrt(dk) (phase k0^2 / 2 dk) and the two Fresnel values cancel down
    to s sqrt(dk)"""
    lg = lambda v: abs(math.log10(abs(v))) if v != 0.0 else 0.0   # noqa: E731
    return int(2.0 * lg(dk) + 2.0 * lg(k0) + lg(s)) + 20


def _xy_pos(mp, k0, dk, s):
    """dk > 0: k0 u + dk u^2 / 2 = (pi / 2) t^2 - k0^2 / (2 dk) with t = sqrt(dk / pi) (u + k0 / dk)"""
    w = mp.sqrt(dk / mp.pi)
    t0, t1 = w * (k0 / dk), w * (s + k0 / dk)
    z = mp.mpc(mp.fresnelc(t1) - mp.fresnelc(t0), mp.fresnels(t1) - mp.fresnels(t0)) / w
    z *= mp.expj(-k0 * k0 / (2 * dk))
    return z.real, z.imag


def xy(k0, dk, s):
    """(x, y) of the clothoid from pose (0, 0, 0) with curvature k0 + dk u at arc length s: two mpf of DPS digits.  The arguments are
    taken as the exact values of the doubles handed in."""
    mp = _mp()
    if abs(float(dk)) * abs(float(s)) ** 3 / 6.0 < 1e-80:   # |xy(k0, dk, s) - xy(k0, 0, s)| <= |dk| s^3 / 6: far below DPS digits of any table entry
        dk = 0.0
    with mp.workdps(DPS + _extra_digits(float(k0), float(dk), float(s))):
        k0, dk, s = mp.mpf(k0), mp.mpf(dk), mp.mpf(s)
        if s == 0:
            x, y = mp.mpf(0), mp.mpf(0)
        elif dk > 0:
            x, y = _xy_pos(mp, k0, dk, s)
        elif dk < 0:                                   # the conjugate curve: exp(j phase) = conj(exp(j (-phase)))
            x, y = _xy_pos(mp, -k0, -dk, s)
            y = -y
        elif k0 != 0:                                  # a circle: (e^{j k0 s} - 1) / (j k0)
            x, y = mp.sin(k0 * s) / k0, 2 * mp.sin(k0 * s / 2) ** 2 / k0
        else:
            x, y = s, mp.mpf(0)
        with mp.workdps(DPS):
            return +x, +y


def stations(L, S):
    """the doubles s_i = i * (L / max(S - 1, 1)) exactly as sample_traj forms them (one division, one product, both rounded)"""
    ds = float(L) / float(max(int(S) - 1, 1))
    return [float(i) * ds for i in range(int(S))]


def rows(k0, dk, L, S):
    """S rows (x, y, theta, |kappa|) of mpf at the stations s_i; theta = s (k0 + s dk / 2), |kappa| = |k0 + dk s|"""
    mp = _mp()
    out = []
    for s in stations(L, S):
        x, y = xy(k0, dk, s)
        with mp.workdps(DPS + 700):                    # exact for any doubles: products of three 53-bit numbers over 2000 binades
            sm, k0m, dkm = mp.mpf(s), mp.mpf(k0), mp.mpf(dk)
            th, ak = sm * (k0m + sm * dkm / 2), abs(k0m + dkm * sm)
        out.append((x, y, th, ak))
    return out


def theta_kappa(k0, dk, L, S):
    """the rows' last two columns without mpmath: theta = s (k0 + s dk / 2) and |kappa| = |k0 + dk s| in exact rational arithmetic, each
    rounded once to double -> float64 [S, 2].  (The fixture stores x and y only; these two need no transcendental function.)"""
    import numpy as np
    k0, dk = Fraction(float(k0)), Fraction(float(dk))
    out = np.empty((int(S), 2))
    for i, s in enumerate(stations(L, S)):
        s = Fraction(s)
        out[i] = float(s * (k0 + s * dk / 2)), float(abs(k0 + dk * s))
    return out


def nsub_rules(k0, dk, L, S):
    """(curvature rule, kappa' rule): the two piece counts of interval_setup before ceil, max and cap, as exact rationals /
    a correctly rounded square root.  |a| = |kappa| hs / 2 <= 0.15 and |b| = |dk| hs^2 / 8 <= 0.02."""
    k0, dk, L = Fraction(float(k0)), Fraction(float(dk)), Fraction(float(L))
    ds = Fraction(float(L) / float(max(int(S) - 1, 1)))
    kmax = max(abs(k0), abs(k0 + dk * L))
    n1 = kmax * ds / Fraction(3, 10)
    n2sq = ds * ds * abs(dk) * Fraction(25, 4)          # n2 = ds sqrt(6.25 |dk|)
    return n1, n2sq


def nsub(k0, dk, L, S):
    """pieces per station interval, uncapped: max(1, ceil(n1), ceil(n2))"""
    n1, n2sq = nsub_rules(k0, dk, L, S)
    c1 = math.ceil(n1)
    c2 = math.isqrt(math.ceil(n2sq))                    # ceil(sqrt(q)) for a rational q > 0: isqrt(ceil(q)), +1 unless that is exact
    if Fraction(c2 * c2) < n2sq:
        c2 += 1
    return max(1, c1, c2)


def cubic_rows(gx, gy, gth, S):
    """The cubic generator (include/f1p.h F1P_GEN_CUBIC): cubic Hermite from pose (0, 0, 0) to (gx, gy, gth), both tangents of magnitude
    m = chord length, stations at u_i = i / max(S - 1, 1) (the double), theta = atan2(y', x'), |kappa| = |x'y'' - y'x''| / (x'^2 + y'^2)^1.5.
    Returns (rows, sp, cond, m): rows of (x, y, theta, |kappa|), sp = x'^2 + y'^2 and cond = |x'||y''| + |y'||x''| per station, all mpf."""
    mp = _mp()
    gx, gy, gth = mp.mpf(gx), mp.mpf(gy), mp.mpf(gth)
    m = mp.sqrt(gx * gx + gy * gy)
    p0, p1 = (mp.mpf(0), mp.mpf(0)), (gx, gy)
    t0, t1 = (m, mp.mpf(0)), (m * mp.cos(gth), m * mp.sin(gth))
    den = max(int(S) - 1, 1)
    out, sps, conds = [], [], []
    for i in range(int(S)):
        u = mp.mpf(float(i) / float(den))
        # Hermite basis on [0, 1]: p(u) = (2u^3 - 3u^2 + 1) p0 + (u^3 - 2u^2 + u) t0 + (-2u^3 + 3u^2) p1 + (u^3 - u^2) t1
        b = (2 * u ** 3 - 3 * u ** 2 + 1, u ** 3 - 2 * u ** 2 + u, -2 * u ** 3 + 3 * u ** 2, u ** 3 - u ** 2)
        d = (6 * u ** 2 - 6 * u, 3 * u ** 2 - 4 * u + 1, -6 * u ** 2 + 6 * u, 3 * u ** 2 - 2 * u)
        e = (12 * u - 6, 6 * u - 4, -12 * u + 6, 6 * u - 2)
        comb = lambda c, a: c[0] * p0[a] + c[1] * t0[a] + c[2] * p1[a] + c[3] * t1[a]   # noqa: E731
        x, y, xd, yd, xdd, ydd = comb(b, 0), comb(b, 1), comb(d, 0), comb(d, 1), comb(e, 0), comb(e, 1)
        sp = xd * xd + yd * yd
        out.append((x, y, mp.atan2(yd, xd), abs(xd * ydd - yd * xdd) / sp ** mp.mpf(1.5)))
        sps.append(sp)
        conds.append(abs(xd) * abs(ydd) + abs(yd) * abs(xdd))
    return out, sps, conds, m


def chord_sum(rws):
    """polyline length of the rows' (x, y): what stands in for L in the cubic generator's 1 / L term"""
    tot = rws[0][0] * 0
    for a, b in zip(rws[:-1], rws[1:]):
        dx, dy = b[0] - a[0], b[1] - a[1]
        tot = tot + (dx * dx + dy * dy) ** 0.5
    return tot


def cost(rws, L, cfg, prev_theta=None):
    """w_len / L + w_maxk max|kappa| + w_meank sum|kappa| / S + w_sim sum_{j < S - n_shift - n_cull}
    (theta_j - prev_theta_{j + n_shift})^2, in the arithmetic of the numbers handed in (mpf, numpy longdouble, Fraction)"""
    S = len(rws)
    ak = [abs(r[3]) for r in rws]
    c = cfg.w_length * (1 / L) + cfg.w_max_kappa * max(ak) + cfg.w_mean_kappa * (sum(ak) / S)
    if prev_theta is not None:
        sim = 0
        for j in range(S - cfg.n_shift - cfg.n_cull):
            d = rws[j][2] - prev_theta[j + cfg.n_shift]
            sim = sim + d * d
        c = c + cfg.w_similarity * sim
    return c


# ---- the fixture and the bars, shared by the host and the GPU tests: numpy only -----------------------------------------
G_S = (2, 3, 50)


def load_fixture(golden_dir):
    """g19_clothoid_eval.npz (+ the goals and parameters of g14_clothoid_g1.npz it points to) -> (table, goals):
    table: list of dict(label, k0, dk, L, S, nsub, rule, want_nsub, mirror_of, anchor_inside, anchor_on_station, rows [S, 4]);
    goals: dict(goals [m, 3], params [m, 3], rows {S: [m, S, 4]}, cubic {S: (rows [m, S, 4], sp [m, S], cond [m, S])})"""
    import os
    import numpy as np
    f = np.load(os.path.join(golden_dir, "g19_clothoid_eval.npz"), allow_pickle=False)
    g = np.load(os.path.join(golden_dir, "g14_clothoid_g1.npz"), allow_pickle=False)
    table = []
    for i, lab in enumerate(f["t_label"]):
        k0, dk, L = (float(v) for v in f["t_params"][i])
        S, src = int(f["t_S"][i]), int(f["t_mirror_of"][i])
        j = i if src < 0 else src
        xy_ = f["t_xy"][f["t_off"][j]:f["t_off"][j + 1]] * ([1.0, 1.0] if src < 0 else [1.0, -1.0])
        table.append(dict(label=str(lab), k0=k0, dk=dk, L=L, S=S, nsub=int(f["t_nsub"][i]), rule=int(f["t_rule"][i]), want_nsub=int(f["t_want_nsub"][i]),
                          mirror_of=src, anchor_inside=bool(f["t_anchor_inside"][i]), anchor_on_station=bool(f["t_anchor_on_station"][i]),
                          rows=np.column_stack([xy_, theta_kappa(k0, dk, L, S)])))
    idx = f["g_idx"]
    par = np.column_stack([g["k0"][idx], g["dk"][idx], g["L"][idx]])
    goals = dict(goals=g["goals"][idx], params=par, rows={}, cubic={})
    for S in G_S:
        tk = np.stack([theta_kappa(*par[i], S) for i in range(len(idx))])
        goals["rows"][S] = np.concatenate([f[f"g_xy_S{S}"], tk], axis=2)
        goals["cubic"][S] = (f[f"c_rows_S{S}"], f[f"c_sp_S{S}"].astype("f8"), f[f"c_cond_S{S}"].astype("f8"))
    return table, goals


def clothoid_errors(got, want, L):
    """(x, y error / bar, theta and |kappa| error / bar) of rows [..., S, 4] against reference rows; the bars (none of them new):
    x, y 1e-12 max(1, L) absolute (outputs through the device's sin / cos), theta and |kappa| 1e-12 relative + 1e-300"""
    import numpy as np
    L = np.asarray(L, dtype=np.float64)[..., None, None]
    d = np.abs(got - want)
    exy = (d[..., :2] / (1e-12 * np.maximum(1.0, L))).max()
    etk = (d[..., 2:] / (1e-12 * np.abs(want[..., 2:]) + 1e-300)).max()
    return float(exy), float(etk)


def drift_bound(c):
    """what the re-anchored evaluation of csrc/lattice_device.h promises for x, y of a table clothoid c, from its own premises: the heading
    phasor is exact at every 16th piece and drifts by less than 3e-14 rad in between (n^2 / 2 roundings of the recurrence, n <= 16: the
    header's bound), so the position is off by less than 3e-14 L; each piece's P, Q and products add four roundings relative to its length
    (4 * 2^-53 L in all) and each of the (S - 1) nsub accumulations one rounding of the running |x|, |y|"""
    import numpy as np
    return 3e-14 * c["L"] + 2.0 ** -53 * (4.0 * c["L"] + (c["S"] - 1) * c["nsub"] * np.abs(c["rows"][:, :2]).max())


def theta_kappa_rounding(k0, dk, L, S):
    """[S, 2]: what fp64 can promise for theta = s (k0 + s dk / 2) and |kappa| = |k0 + dk s| evaluated in doubles: each of the (at most four)
    roundings is relative to the TERMS |s k0| + |s^2 dk / 2| resp. |k0| + |dk s|, not to a sum that cancels: 4 * 2^-53 of the terms (+ the bars' 1e-300 for subnormal values)"""
    import numpy as np
    s = np.array(stations(L, S))
    return 4.0 * 2.0 ** -53 * np.column_stack([np.abs(s * k0) + np.abs(0.5 * s * s * dk), np.full(len(s), abs(k0)) + np.abs(dk * s)]) + 1e-300


def cubic_errors(got, want, sp, cond, m):
    """(x, y error / bar, theta error / bar, |kappa| error / bar, share of stations left out of the |kappa| check) for cubic rows [n, S, 4]:
    x, y 1e-12 max(1, m); theta 1e-12 absolute; |kappa| 1e-12 |kappa| + 4 * 2^-53 (|x'||y''| + |y'||x''|) / sp^1.5 on the stations with
    sp >= 1e-6 m^4 (m = chord length)"""
    import numpy as np
    m = np.asarray(m, dtype=np.float64)[:, None]
    d = np.abs(got - want)
    exy = (d[..., :2] / (1e-12 * np.maximum(1.0, m))[..., None]).max()
    eth = (d[..., 2] / 1e-12).max()
    use = sp >= 1e-6 * m ** 4
    bar = 1e-12 * np.abs(want[..., 3]) + 4.0 * 2.0 ** -53 * cond / sp ** 1.5
    ek = np.where(d[..., 3] <= bar, d[..., 3] / np.maximum(bar, 1e-300), np.inf)[use].max()     # (a straight goal: error 0 against a bar of 0)
    return float(exy), float(eth), float(ek), float(1.0 - use.mean())


# ---- the plans of the tests: 4 egos x 64 host goals from the fixture's goals --------------------------------------------------------------
PLAN_E, PLAN_C = 4, 64
PLAN_S = (2, 3, 17, 50, 65)


def plan_goals(goals, keep=None):
    """-> (goals [4, 64, 3], src [4, 64]): ego e gets the fixture's goals e, e + 4, ... (src = their index there), the rest of its 64
    candidates are NaN goals (infeasible, src -1).  keep [m] bool: leave the others out as well."""
    import numpy as np
    out = np.full((PLAN_E, PLAN_C, 3), np.nan)
    src = np.full((PLAN_E, PLAN_C), -1)
    for e in range(PLAN_E):
        mine = [i for i in range(e, len(goals), PLAN_E) if keep is None or keep[i]][:PLAN_C]
        out[e, :len(mine)] = goals[mine]
        src[e, :len(mine)] = mine
    return out, src


def cubic_plan_keep(G):
    """[m] bool: the goals whose cubic |kappa| is well conditioned at every station of S = 2, 3, 50 -- no station left out (sp >= 1e-6 m^4) and
    the conditioning term 4 * 2^-53 cond / sp^1.5 at most 1e-12 of the candidate's largest |kappa|, so that the rows' bars keep a cost within
    rtol 1e-10 (the cost is linear in |kappa| with weights below 1)"""
    import numpy as np
    m = np.hypot(G["goals"][:, 0], G["goals"][:, 1])[:, None]
    keep = np.ones(len(m), bool)
    for S in G_S:
        rows_, sp, cond = G["cubic"][S]
        keep &= (sp >= 1e-6 * m ** 4).all(axis=1) & (4.0 * 2.0 ** -53 * cond / sp ** 1.5 <= 1e-12 * rows_[..., 3].max(axis=1, keepdims=True)).all(axis=1)
    return keep


def plan_prev_theta(S):
    """a previous winner's headings [4, S] for the similarity term: smooth, different per ego, nothing special"""
    import numpy as np
    u = np.linspace(0.0, 1.0, S)
    return np.stack([(0.2 + 0.1 * e) * np.sin((1.0 + 0.5 * e) * u) - 0.05 * e * u for e in range(PLAN_E)])


def plan_costs(rows, L, cfg, prev_theta):
    """cost() in numpy's long double over rows [E, C, S, 4] (a row set that is pinned to the reference), L [E, C]; NaN L = infeasible = +inf.
    -> (cost [E, C] float64, excused [E]: the two lowest costs of the ego lie within 1e-9 relative, its argmin is not asserted)"""
    import numpy as np
    E, Cn = L.shape
    c = np.full((E, Cn), np.inf, np.longdouble)
    for e in range(E):
        pt = None if prev_theta is None else prev_theta[e].astype(np.longdouble)
        for k in range(Cn):
            if np.isfinite(L[e, k]):
                c[e, k] = cost(list(rows[e, k].astype(np.longdouble)), np.longdouble(L[e, k]), cfg, pt)
    two = np.sort(c, axis=1)[:, :2]
    return c.astype(np.float64), np.asarray((two[:, 1] - two[:, 0]) <= 1e-9 * np.abs(two[:, 0]))
