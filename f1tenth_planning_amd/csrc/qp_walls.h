// qp_walls.h -- the wall rows of k_kmpc_qp's third variant (f1p_kmpc_qp_walls_*): the occupancy bitmap as half-planes of the QP.
//
// Per step t = 1..T two wall candidates compete with the live discs of qp_avoid.h for the step's two rows.  From the linearisation path's
// point pbar_t a side sigma = +1 (left, slot 16) / -1 (right, slot 17) is marched along l = sigma (-sin psibar_t, cos psibar_t) at
// q_k = pbar_t + ((double)k h) l, k = 1 .. n_samples, h = res / 2, on the ACTIVE bitmap with cell_of's rule (outside the image or not finite:
// occupied).  k*: the first occupied sample; the contact c = q_{k* - 1} (q_0 = pbar_t), the clearance (double)(k* - 1) h, the normal -l, the
// row  -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - wall_margin.  Of the (up to) four candidates the two with the least clearance are taken,
// ties to the lower slot.  Here: the march of one side, a candidate from its k*, and the choice among four -- nothing of a kernel's lane
// layout (k_kmpc_qp.hip: a lane per side of a step; a lane-per-step kernel marches both sides itself).  The arguments: QpWallArgs
// (f1p_internal.h).
#pragma once
#include "qp_avoid.h"

namespace f1p {

#define F1P_QP_WALL_SLOT_L 16
#define F1P_QP_WALL_SLOT_R 17

// the kernels' second trailing argument, when there is one
__device__ __forceinline__ QpAvoidArgs qp_avoid_args(const QpAvoidArgs& a, const QpWallArgs&) { return a; }
__device__ __forceinline__ QpWallArgs qp_wall_args() { return QpWallArgs{}; }
__device__ __forceinline__ QpWallArgs qp_wall_args(const QpAvoidArgs&) { return QpWallArgs{}; }
__device__ __forceinline__ QpWallArgs qp_wall_args(const QpAvoidArgs&, const QpWallArgs& w) { return w; }

// sample k of the march from (px, py) along (lx, ly)
__device__ __forceinline__ void qp_wall_sample(const QpWallArgs& w, double px, double py, double lx, double ly, int k, double& qx, double& qy) {
    const double s = (double)k * w.h;
    qx = px + s * lx; qy = py + s * ly;
}

// k*: the first k in 1 .. n_samples whose sample is occupied, 0: none.  The samples' bit tests do not depend on each other: eight words are
// requested before the first of them is looked at, and a group without a hit goes on to the next eight.
__device__ __forceinline__ int qp_wall_march(const QpWallArgs& w, double px, double py, double lx, double ly) {
    constexpr int CH = 8;
    for (int k0 = 1; k0 <= w.n_samples; k0 += CH) {
        uint32_t word[CH];
        int sh[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            double qx, qy;
            qp_wall_sample(w, px, py, lx, ly, k0 + c, qx, qy);
            int gx, gy;
            const bool inside = cell_of(w.g, qx, qy, gx, gy);
            const bool want = inside && k0 + c <= w.n_samples;                 // a load only of a cell of the image
            word[c] = want ? w.g.bits[(size_t)gy * w.g.wwords + (gx >> 5)] : ~0u;
            sh[c] = want ? (gx & 31) : 0;
        }
        int first = 0;
#pragma unroll
        for (int c = CH - 1; c >= 0; --c)
            if (k0 + c <= w.n_samples && ((word[c] >> sh[c]) & 1u)) first = k0 + c;
        if (first) return first;
    }
    return 0;
}

// one candidate for a row: its clearance and slot (-1: absent); a wall's contact point beside them
struct QpCand {
    double clear = 0.0;
    int slot = -1;
};
struct QpWallCand : QpCand {
    double cx = 0.0, cy = 0.0;
};

// the candidate of a side from its k* (0: none): (lx, ly) that side's direction
__device__ __forceinline__ QpWallCand qp_wall_cand(const QpWallArgs& w, double px, double py, double lx, double ly, int kstar, int slot) {
    QpWallCand c;
    if (kstar < 1) return c;
    c.slot = slot;
    c.clear = (double)(kstar - 1) * w.h;
    c.cx = px; c.cy = py;
    if (kstar > 1) qp_wall_sample(w, px, py, lx, ly, kstar - 1, c.cx, c.cy);
    return c;
}

// a live disc's clearance at (px, py) at time tt: the number qp_avoid_nearest ranks by
__device__ __forceinline__ QpCand qp_disc_cand(const double* ob, int m, double px, double py, double tt) {
    QpCand c;
    if (m < 0) return c;
    const double dx = px - (ob[5 * m] + ob[5 * m + 2] * tt), dy = py - (ob[5 * m + 1] + ob[5 * m + 3] * tt);
    c.clear = sqrt(dx * dx + dy * dy) - ob[5 * m + 4];
    c.slot = m;
    return c;
}

// which of four candidates, given in slot order, is the j-th (j = 0, 1) by (clearance, slot); -1: there are fewer
__device__ __forceinline__ int qp_select4(const QpCand& c0, const QpCand& c1, const QpCand& c2, const QpCand& c3, int j) {
    const QpCand* c[4] = {&c0, &c1, &c2, &c3};
    int pick = -1;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int before = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b != a && c[b]->slot >= 0 && (c[b]->clear < c[a]->clear || (c[b]->clear == c[a]->clear && b < a))) ++before;
        if (c[a]->slot >= 0 && before == j) pick = a;
    }
    return pick;
}

// a wall candidate's half-plane: the normal -l, (sx, sy) the free response's position at that step
__device__ __forceinline__ QpPlane qp_wall_plane(const QpWallCand& c, double lx, double ly, double sx, double sy, double margin) {
    QpPlane pl;
    pl.nx = -lx; pl.ny = -ly;
    pl.h = pl.nx * (sx - c.cx) + pl.ny * (sy - c.cy) - margin;
    pl.slot = c.slot;
    return pl;
}

}  // namespace f1p
