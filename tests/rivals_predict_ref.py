"""The rule of the rivals' prediction along their courses (include/f1p.h "Rivals, predicted along the course") in plain numpy, loops and
all: the reference of tests/test_rivals_predict_host.py and tests/test_gpu_rivals_predict.py, and the scene both share.

Selection, slot order, idx, pace and the empty slots are rivals_ref.rivals' (DESIGN.md 5m); only (vx, vy, r) of a live slot are formed here.  The nearest
segment, its parameter and the projection (b, t, q) come from the oracle's nearest_point, which has its own bit-exact tests against the device scan, so a
projection tie cannot split the reference and the device.  Everything else is Python float (IEEE binary64) arithmetic in the header's operation order."""
import math

import numpy as np

import rivals_ref as base

XYVYAW, POSE, ST7 = base.XYVYAW, base.POSE, base.ST7


def arc_table(course):
    """course [n, >= 2] -> (len [n - 1], cum [n], usable): sequential adds; usable: n >= 2, no zero-length segment, L finite and positive"""
    p = np.asarray(course, dtype=np.float64)
    n = p.shape[0]
    lens, cum = [], [0.0]
    with np.errstate(all="ignore"):
        for k in range(n - 1):
            dx = float(p[k + 1, 0]) - float(p[k, 0])
            dy = float(p[k + 1, 1]) - float(p[k, 1])
            q = dx * dx + dy * dy
            ln = math.sqrt(q) if q >= 0.0 else float("nan")
            lens.append(ln)
            cum.append(cum[-1] + ln)
    usable = n >= 2 and all(ln > 0.0 for ln in lens) and math.isfinite(cum[-1]) and cum[-1] > 0.0
    return np.array(lens), np.array(cum), usable


def frenet(orc, course, lens, cum, x, y, v, h):
    """-> (b, s0, d, dir) of a vehicle with a finite state on a usable course"""
    p = np.asarray(course, dtype=np.float64)
    q, _, t, b = orc.nearest_point(np.array([x, y]), np.ascontiguousarray(p[:, :2]))
    ln = float(lens[b])
    ux = (float(p[b + 1, 0]) - float(p[b, 0])) / ln
    uy = (float(p[b + 1, 1]) - float(p[b, 1])) / ln
    s0 = float(cum[b]) + t * ln
    d = (x - float(q[0])) * (-uy) + (y - float(q[1])) * ux
    dr = 1.0 if v * (math.cos(h) * ux + math.sin(h) * uy) >= 0.0 else -1.0
    return int(b), s0, d, dr


def arc_at(cum, s0, dr, av, tau, wrap):
    """-> (s, the value before the wrap and the clamp)"""
    L = float(cum[-1])
    raw = s0 + (dr * av) * tau
    s = raw
    if wrap:
        s = s - L * math.floor(s / L)
    s = min(max(s, 0.0), L)
    return s, raw


def position(course, lens, cum, s, d):
    p = np.asarray(course, dtype=np.float64)
    n = p.shape[0]
    k = min(int(np.searchsorted(cum, s, side="right")) - 1, n - 2)       # the largest k <= n - 2 with cum_k <= s
    ln = float(lens[k])
    ux = (float(p[k + 1, 0]) - float(p[k, 0])) / ln
    uy = (float(p[k + 1, 1]) - float(p[k, 1])) / ln
    w = s - float(cum[k])
    return float(p[k, 0]) + ux * w + (-uy) * d, float(p[k, 1]) + uy * w + ux * d


def predict(orc, states, layout, M, radius, courses, track_ids=None, horizon_s=0.8, horizon_m=0.0, knots=8, inflate=True, wrap=True,
            reach=np.inf, min_speed=0.5, groups=None):
    """courses: list of polylines [n_k, >= 2]; track_ids None: every vehicle follows courses[0] (the context's raceline), else vehicle j follows
    courses[track_ids[j]] -> dict(obs, pace, idx as rivals_ref.rivals, frenet [E, 3] = (s0, d, dir) with NaN rows, b int [E] (-1 where NaN),
    predicted bool [E, M], dev [E, M], knot_s: list of (ego, slot, vehicle, knot, s, raw s) of every evaluated knot)"""
    out = base.rivals(states, layout, M, radius, reach=reach, min_speed=min_speed, groups=groups)
    x, y, v, h = base.columns(states, layout)
    E = x.shape[0]
    K = int(knots)
    tabs = [arc_table(c) for c in courses]
    fr = np.full((E, 3), np.nan)
    bseg = np.full(E, -1)
    course_of = [None] * E
    for j in range(E):
        k = 0 if track_ids is None else int(track_ids[j])
        if not 0 <= k < len(courses):
            continue
        lens, cum, usable = tabs[k]
        if not usable or not all(math.isfinite(float(a)) for a in (x[j], y[j], v[j], h[j])):
            continue
        b, s0, d, dr = frenet(orc, courses[k], lens, cum, float(x[j]), float(y[j]), float(v[j]), float(h[j]))
        fr[j] = (s0, d, dr)
        bseg[j] = b
        course_of[j] = k
    predicted = np.zeros((E, M), bool)
    devs = np.zeros((E, M))
    knot_s = []
    obs = out["obs"]
    for i in range(E):
        H = float(np.float64(horizon_s) + np.float64(horizon_m) * out["pace"][i])
        if not math.isfinite(H) or not H > 0.0:
            continue
        for m in range(M):
            j = int(out["idx"][i, m])
            if j < 0 or course_of[j] is None:
                continue
            av = abs(float(v[j]))
            if not av * H < 1e9:
                continue
            k = course_of[j]
            lens, cum, _ = tabs[k]
            s0, d, dr = (float(a) for a in fr[j])
            c = []
            for q in range(K + 1):
                s, raw = arc_at(cum, s0, dr, av, (H * q) / K, wrap)
                knot_s.append((i, m, j, q, s, raw))
                c.append(position(courses[k], lens, cum, s, d))
            dev = 0.0
            for q in range(1, K):
                f = q / K
                ex = (c[q][0] - c[0][0]) - (c[K][0] - c[0][0]) * f
                ey = (c[q][1] - c[0][1]) - (c[K][1] - c[0][1]) * f
                dev = max(dev, math.sqrt(ex * ex + ey * ey))
            obs[i, m, 2] = (c[K][0] - c[0][0]) / H
            obs[i, m, 3] = (c[K][1] - c[0][1]) / H
            if inflate:
                obs[i, m, 4] = radius + dev
            predicted[i, m] = True
            devs[i, m] = dev
    out.update(frenet=fr, b=bseg, predicted=predicted, dev=devs, knot_s=knot_s)
    return out


def knot_margin(ref, courses, track_ids, wrap):
    """the scene condition: a laterally offset path jumps at a vertex, so the reference and the device may only be compared where no knot's s is
    within rounding of a vertex.  -> the smallest distance of an evaluated knot's s from every cum_k (0 and L among them).  A knot whose s is
    bit-equal to 0 or L is exempt only when that value is exact on both sides: the projection's parameter was clamped (s before the wrap is bit-equal
    to 0 or L), or the clamp of an open course cut a value at least 1e-6 outside [0, L]; any other such knot counts as distance 0."""
    tabs = [arc_table(c) for c in courses]
    worst = np.inf
    for (_, _, j, _, s, raw) in ref["knot_s"]:
        cum = tabs[0 if track_ids is None else int(track_ids[j])][1]
        L = float(cum[-1])
        if s == 0.0 or s == L:
            exact = raw == 0.0 or raw == L or (not wrap and (raw >= L + 1e-6 or raw <= -1e-6))
            if not exact:
                worst = 0.0
            continue
        worst = min(worst, float(np.abs(cum - s).min()))
    return worst


# ---- the courses and the scene of the tests -----------------------------------------------------------------------------------------------------
def circle(radius=2.0, n=257, centre=(0.0, 0.0), clockwise=False, speed=3.0):
    """n points on a circle, the first equal to the last, columns (x, y, v, psi)"""
    a = 2.0 * np.pi * np.arange(n) / (n - 1)
    if clockwise:
        a = -a
    xy = np.column_stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)])
    xy[-1] = xy[0]
    psi = a + (-np.pi / 2 if clockwise else np.pi / 2)
    return np.column_stack([xy, np.full(n, speed), psi])


def open_l():
    """a 5-point open L: 4 m along +x, then 3 m along +y"""
    xy = np.array([[6.0, -1.0], [8.0, -1.0], [10.0, -1.0], [10.0, 0.5], [10.0, 2.0]])
    psi = np.array([0.0, 0.0, 0.0, np.pi / 2, np.pi / 2])
    return np.column_stack([xy, np.full(5, 3.0), psi])


def courses():
    return [circle(), circle(3.0, 193, centre=(1.5, 7.0), clockwise=True), open_l()]


SCENE_E = 70
SCENE_SEED = 26


def on_course(course, seg, frac, d):
    """(x, y, heading of the segment) at the fraction `frac` of segment `seg` of a course, lateral offset d: the foot of the perpendicular is that point
    of that segment, so nearest_point's parameter is frac, not a clamped one"""
    p0, p1 = course[seg, :2], course[seg + 1, :2]
    u = (p1 - p0) / np.hypot(*(p1 - p0))
    p = p0 + (p1 - p0) * frac + np.array([-u[1], u[0]]) * d
    return p[0], p[1], math.atan2(u[1], u[0])


def scene(raceline=False, seed=SCENE_SEED, line=None):
    """70 vehicles in three races (interleaved, so that a race strides past one wave's lanes; uneven sizes) plus two ungrouped -> (states [E, 4] =
    (x, y, v, yaw), groups [E], track_ids [E] or None).  raceline: all on the first course, the context's raceline; else on the three courses with the
    ids mixed; line: another raceline than the first course.  On and off the line (|d| <= 0.4), v = 0, negative v, reversed heading, one vehicle with |v| H > L and (track set) one beyond the L's end."""
    rng = np.random.default_rng(seed + (100 if raceline else 0))
    cs = courses() if line is None else [line]
    E = SCENE_E
    groups = np.array([e % 3 for e in range(E)])
    groups[[7, 40]] = -1
    groups[np.arange(3, 30, 6)] = 0                                  # (uneven sizes)
    tid = np.zeros(E, np.int64) if raceline else rng.integers(0, 3, E)
    st = np.zeros((E, 4))
    for e in range(E):
        c = cs[tid[e]]
        d = 0.0 if e % 5 == 0 else rng.uniform(-0.4, 0.4)
        x, y, hd = on_course(c, int(rng.integers(0, c.shape[0] - 1)), rng.uniform(0.3, 0.7), d)
        st[e] = (x, y, rng.uniform(0.3, 6.0), hd + rng.uniform(-0.3, 0.3))
    st[4, 2] = 0.0                                                   # standing
    st[9, 2] = 0.0
    st[12, 2] = -2.5                                                 # driving backwards
    st[31, 2] = -0.7
    st[17, 3] += np.pi                                               # heading against the course
    st[50, 3] += np.pi
    tid[36] = 0                                                      # |v| H > L on the circle (L = 12.6 m)
    x, y, hd = on_course(cs[0], 67, 0.4, 0.1)
    st[36] = (x, y, 19.0, hd)
    if raceline:
        return st, groups, None
    tid[23] = 2                                                      # beyond the L's end: t is clamped
    st[23] = (10.2, 2.6, 1.5, np.pi / 2)
    return st, groups, tid.astype(np.int32)


def as_layout(st, layout):
    """the scene's (x, y, v, yaw) rows in one of the three layouts (st7: the heading split into yaw and beta)"""
    if layout == XYVYAW:
        return st.copy()
    if layout == POSE:
        return np.ascontiguousarray(st[:, [0, 1, 3, 2]])
    s7 = np.zeros((st.shape[0], 7))
    s7[:, [0, 1, 3]] = st[:, [0, 1, 2]]
    s7[:, 6] = 0.125
    s7[:, 4] = st[:, 3] - 0.125
    return s7
