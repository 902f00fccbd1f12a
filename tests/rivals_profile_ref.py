"""The rule of the rivals' prediction with the course's speed profile (include/f1p.h "Rivals, predicted with the course's speed profile") in
plain Python floats: the reference of tests/test_rivals_profile_host.py and tests/test_gpu_rivals_profile.py.

Built on rivals_predict_ref: selection, slots, pace, the arc table, the Frenet records, the chord, dev and every fallback are that file's; only
the map from tau to a point on the course is formed here.  The scene is that file's 70 vehicles on its three courses, with the speed columns replaced by ones
that vary along the course."""
import math

import numpy as np

import rivals_predict_ref as ref
import rivals_ref as base

XYVYAW, POSE, ST7 = ref.XYVYAW, ref.POSE, ref.ST7
SCENE_E = ref.SCENE_E


def time_table(course, lens, usable, min_speed):
    """course [n, >= 3] with the speed in column 2, lens and usable from ref.arc_table -> (c [n - 1], tim [n], profile-usable): c_k the mean of the two
    |speeds| of segment k floored at min_speed, tim the sequential sum of len_k / c_k"""
    w = [float(a) for a in np.asarray(course, dtype=np.float64)[:, 2]]
    floor = float(min_speed)
    c, tim = [], [0.0]
    with np.errstate(all="ignore"):
        for k in range(len(w) - 1):
            ck = 0.5 * (abs(w[k]) + abs(w[k + 1]))
            if not ck >= floor:
                ck = floor
            c.append(ck)
            tim.append(tim[-1] + float(lens[k]) / ck)
    ok = bool(usable) and all(math.isfinite(a) for a in w) and math.isfinite(tim[-1]) and tim[-1] > 0.0
    return np.array(c), np.array(tim), ok


def time_at(tim, th0, dr, rho, tau, wrap):
    """-> (th, the value before the wrap and the clamp)"""
    Tl = float(tim[-1])
    raw = th0 + (dr * rho) * tau
    th = raw
    if wrap:
        th = th - Tl * math.floor(th / Tl)
    th = min(max(th, 0.0), Tl)
    return th, raw


def position(course, lens, c, tim, th, d):
    p = np.asarray(course, dtype=np.float64)
    n = p.shape[0]
    k = min(int(np.searchsorted(tim, th, side="right")) - 1, n - 2)       # the largest k <= n - 2 with tim_k <= th
    ln = float(lens[k])
    ux = (float(p[k + 1, 0]) - float(p[k, 0])) / ln
    uy = (float(p[k + 1, 1]) - float(p[k, 1])) / ln
    w = (th - float(tim[k])) * float(c[k])
    return float(p[k, 0]) + ux * w + (-uy) * d, float(p[k, 1]) + uy * w + ux * d


def predict(orc, states, layout, M, radius, courses, track_ids=None, horizon_s=0.8, horizon_m=0.0, knots=8, inflate=True, wrap=True,
            reach=np.inf, min_speed=0.5, groups=None):
    """ref.predict's arguments and result with speed = "profile"; courses carry the speed in column 2.  knot_s holds the knots of the vehicles that fall
    back to the constant-speed rule (a course that is usable but not profile-usable), knot_th: list of (ego, slot, vehicle, knot, th, raw th) of every
    knot evaluated in the time coordinate"""
    out = base.rivals(states, layout, M, radius, reach=reach, min_speed=min_speed, groups=groups)
    x, y, v, h = base.columns(states, layout)
    E = x.shape[0]
    K = int(knots)
    tabs = [ref.arc_table(c) for c in courses]
    times = [time_table(c, t[0], t[2], min_speed) if np.asarray(c).shape[1] >= 3 and np.asarray(c).shape[0] >= 2 else (None, None, False)
             for c, t in zip(courses, tabs)]
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
        b, s0, d, dr = ref.frenet(orc, courses[k], lens, cum, float(x[j]), float(y[j]), float(v[j]), float(h[j]))
        fr[j] = (s0, d, dr)
        bseg[j] = b
        course_of[j] = k
    predicted = np.zeros((E, M), bool)
    timed = np.zeros((E, M), bool)
    devs = np.zeros((E, M))
    knot_s, knot_th = [], []
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
            ck, tim, prof = times[k]
            s0, d, dr = (float(a) for a in fr[j])
            c = []
            if prof:
                b = int(bseg[j])
                rho = av / float(ck[b])
                th0 = float(tim[b]) + (s0 - float(cum[b])) / float(ck[b])
                for q in range(K + 1):
                    th, raw = time_at(tim, th0, dr, rho, (H * q) / K, wrap)
                    knot_th.append((i, m, j, q, th, raw))
                    c.append(position(courses[k], lens, ck, tim, th, d))
            else:
                for q in range(K + 1):
                    s, raw = ref.arc_at(cum, s0, dr, av, (H * q) / K, wrap)
                    knot_s.append((i, m, j, q, s, raw))
                    c.append(ref.position(courses[k], lens, cum, s, d))
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
            timed[i, m] = prof
            devs[i, m] = dev
    out.update(frenet=fr, b=bseg, predicted=predicted, timed=timed, dev=devs, knot_s=knot_s, knot_th=knot_th)
    return out


def knot_margin(r, courses, track_ids, wrap, min_speed=0.5):
    """ref.knot_margin in the time coordinate, in metres: the smallest |th - tim_k| * c_k over the evaluated knots, k and k + 1 the vertices of the knot's
    own segment (the nearest ones: the distance along the course to the vertex before it and to the one after it).  A th that is bit-equal to 0 or Tl is
    exempt under knot_margin's condition: the value before the wrap is bit-equal to 0 or Tl, or the clamp of an open course cut a value at least 1e-6 m
    outside [0, Tl]; any other such knot counts as distance 0.  The knots of the vehicles that fell back to the constant-speed rule count with
    ref.knot_margin."""
    tabs = [ref.arc_table(c) for c in courses]
    times = [time_table(c, t[0], t[2], min_speed) for c, t in zip(courses, tabs)]
    worst = ref.knot_margin(r, courses, track_ids, wrap) if r["knot_s"] else np.inf
    for (_, _, j, _, th, raw) in r["knot_th"]:
        ck, tim, _ = times[0 if track_ids is None else int(track_ids[j])]
        Tl = float(tim[-1])
        if th == 0.0 or th == Tl:
            exact = raw == 0.0 or raw == Tl or (not wrap and ((raw - Tl) * float(ck[-1]) >= 1e-6 or raw * float(ck[0]) <= -1e-6))
            if not exact:
                worst = 0.0
            continue
        k = min(int(np.searchsorted(tim, th, side="right")) - 1, len(ck) - 1)
        worst = min(worst, (th - float(tim[k])) * float(ck[k]), (float(tim[k + 1]) - th) * float(ck[k]))
    return worst


# ---- the courses and the scene of the tests -----------------------------------------------------------------------------------------------------
def with_speed(course, speed):
    c = np.array(course, dtype=np.float64)
    c[:, 2] = speed
    return c


def courses():
    """ref.courses() with speed columns that vary along the course: the circle 3.0 + 1.5 sin(3a), the clockwise circle 2.5 + 1.0 cos(2a) (a the
    parameter of ref.circle, the last row equal to the first), the open L slow through its corner"""
    circ, cw, ell = ref.courses()
    a = 2.0 * np.pi * np.arange(circ.shape[0]) / (circ.shape[0] - 1)
    v0 = 3.0 + 1.5 * np.sin(3.0 * a)
    v0[-1] = v0[0]
    a = 2.0 * np.pi * np.arange(cw.shape[0]) / (cw.shape[0] - 1)
    v1 = 2.5 + 1.0 * np.cos(2.0 * a)
    v1[-1] = v1[0]
    return [with_speed(circ, v0), with_speed(cw, v1), with_speed(ell, [3.0, 3.0, 1.2, 1.2, 2.5])]


def scene(raceline=False):
    """ref.scene: the vehicles do not depend on the speed columns"""
    return ref.scene(raceline)


as_layout = ref.as_layout
