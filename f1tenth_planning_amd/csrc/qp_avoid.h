// qp_avoid.h -- the moving-disc avoidance rows of k_kmpc_qp and k_stmpc_qp: what the two kernels' AV variants share.
//
// Per step t = 1..T the two live discs with the least clearance at the linearisation path's point pbar_t give the half-planes
//   -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - (r + margin),   c: the disc's centre at t DT, n: the unit vector from c to pbar_t
// (on the centre itself: minus the direction of travel).  Here: the discs into LDS, the choice of the two, one half-plane, and its
// record in `planes`.  The rows' u-coefficients, the slack and the hooks of qp_ipm.h are each kernel's own (a lane per input with one
// plane and a dense A there, a lane per step with two planes, a packed A and the scaled slack here).  The arguments: QpAvoidArgs
// (f1p_internal.h), the struct the launchers are handed.
#pragma once
#include "qp_ipm.h"

namespace f1p {

// AvArgs of the kernels: none (the plain QP), or one QpAvoidArgs (AV)
__device__ __forceinline__ QpAvoidArgs qp_avoid_args() { return QpAvoidArgs{}; }
__device__ __forceinline__ QpAvoidArgs qp_avoid_args(const QpAvoidArgs& a) { return a; }

// ego e's discs -> ob [M][5], by the G lanes of its group: a live slot (r >= 0) must be finite (-> true if one is not); an empty one is
// kept as r = -1
template <int G>
__device__ __forceinline__ bool qp_avoid_load(const QpAvoidArgs& av, int e, int lane, double* ob) {
    bool bad = false;
    for (int m = lane; m < av.M; m += G) {
        const double* o = av.obs + ((size_t)e * av.M + m) * 5;
        const double ox = o[0], oy = o[1], ovx = o[2], ovy = o[3], r = o[4];
        const bool live = r >= 0.0;
        ob[5 * m] = ox; ob[5 * m + 1] = oy; ob[5 * m + 2] = ovx; ob[5 * m + 3] = ovy; ob[5 * m + 4] = live ? r : -1.0;
        bad |= live && !(isfinite(ox) && isfinite(oy) && isfinite(ovx) && isfinite(ovy) && isfinite(r));
    }
    return bad;
}

// the slots of the two least clearances from (px, py) at time tt, ties to the lower slot; -1: no such disc
struct QpNearest {
    int m0, m1;
};
__device__ __forceinline__ QpNearest qp_avoid_nearest(const double* ob, int M, double px, double py, double tt) {
    double c0 = INFINITY, c1 = INFINITY;
    int m0 = -1, m1 = -1;
    for (int m = 0; m < M; ++m) {
        const double r = ob[5 * m + 4];
        if (!(r >= 0.0)) continue;
        const double dx = px - (ob[5 * m] + ob[5 * m + 2] * tt), dy = py - (ob[5 * m + 1] + ob[5 * m + 3] * tt);
        const double clear = sqrt(dx * dx + dy * dy) - r;
        if (clear < c0) { c1 = c0; m1 = m0; c0 = clear; m0 = m; }
        else if (clear < c1) { c1 = clear; m1 = m; }
    }
    return QpNearest{m0, m1};
}

// one half-plane  n.p >= ... as the row's (n, right-hand side h, slot); absent: zeros and slot -1
struct QpPlane {
    double nx = 0.0, ny = 0.0, h = 0.0;
    int slot = -1;
};

// the half-plane of live slot ms at time tt: (px, py) the path's point, yaw the heading to fall back on there (a reference: read only on
// the disc's centre), (sx, sy) the free response's position at that step
__device__ __forceinline__ QpPlane qp_avoid_plane(const double* ob, int ms, double px, double py, const double& yaw, double tt, double sx,
                                                  double sy, double margin) {
    QpPlane pl;
    const double r = ob[5 * ms + 4];
    const double cx = ob[5 * ms] + ob[5 * ms + 2] * tt, cy = ob[5 * ms + 1] + ob[5 * ms + 3] * tt;
    const double dx = px - cx, dy = py - cy, dist = sqrt(dx * dx + dy * dy);
    if (dist < 1e-9) {                                   // on the disc's centre: stay behind it
        double sn, cs;
        sincos(yaw, &sn, &cs);
        pl.nx = -cs; pl.ny = -sn;
    } else {
        pl.nx = dx / dist; pl.ny = dy / dist;
    }
    pl.h = pl.nx * (sx - cx) + pl.ny * (sy - cy) - (r + margin);
    pl.slot = ms;
    return pl;
}

// the row's record in planes [E][T][2][4]: (n_x, n_y, h, slot), NaN unless ok
__device__ __forceinline__ void qp_avoid_write_plane(double* p, const QpPlane& pl, bool ok) {
    const double NaN = __builtin_nan("");
    p[0] = ok ? pl.nx : NaN; p[1] = ok ? pl.ny : NaN; p[2] = ok ? pl.h : NaN; p[3] = ok ? (double)pl.slot : NaN;
}

}  // namespace f1p
