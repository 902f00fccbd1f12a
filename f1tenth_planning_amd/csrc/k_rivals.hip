// k_rivals.hip -- each ego's nearest other vehicles of its race as moving discs (include/f1p.h "Rivals"): the [E][M][5] slots the
// three *_set_obstacles_dev borrow, the lattice's pace [E] and the chosen indices [E][M].
//
// One wave per ego, four per workgroup, no LDS.  The race's members are read through the list f1p_rivals_set_groups sorted by (group, ego)
// (none: the identity, one race of all).  Slot m is the (d2, j) argmin -- np.argmin's order: NaN first, then the value, then the index -- over
// the candidates STRICTLY AFTER slot m-1's in that order: M rounds of wave_argmin_2step, each lane proposing the best of the members it strides
// over.  (d2, j) pairs are distinct in j, so the order is total and "strictly after the last one taken" removes exactly the taken ones.  A race
// of up to 64 members computes every distance once (the first stride is kept in registers); a larger one re-evaluates the strides past the
// first in every round: O(M n) distances per ego.  The slot values (one full-range sincos each) are formed once, by lane m for slot m.
#include "f1p_internal.h"

namespace f1p {

#define F1P_RIV_NONE 0x7fffffff

__global__ __launch_bounds__(256) void k_rivals(const double* __restrict__ st, int stride, int iv, int ih, int ib, int E, int M, double radius,
                                                double reach2, double min_speed, const int32_t* __restrict__ mem,
                                                const int32_t* __restrict__ rng, double* __restrict__ obs, double* __restrict__ pace,
                                                int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (e >= E) return;                                               // (the whole wave: nothing below synchronises workgroups)
    int begin = 0, end = E;
    if (rng) { begin = rng[2 * e]; end = rng[2 * e + 1]; }
    const double* se = st + (size_t)e * stride;
    const double xi = se[0], yi = se[1];
    const double inf = __builtin_huge_val();

    // this lane's member of the first stride: its distance is formed once
    double d0 = inf; int j0 = F1P_RIV_NONE; bool c0 = false;
    if (begin + lane < end) {
        const int j = mem ? mem[begin + lane] : begin + lane;
        const double dx = st[(size_t)j * stride] - xi, dy = st[(size_t)j * stride + 1] - yi;
        const double d2 = dx * dx + dy * dy;
        c0 = (j != e) & !(d2 > reach2);                               // a NaN d2 is a candidate
        d0 = d2; j0 = j;
    }
    const bool more = end - begin > 64;                               // (wave-uniform)
    double pd = 0.0; int pj = -1;                                     // the last slot taken
    int myj = -1;                                                     // lane m: slot m's vehicle
    for (int m = 0; m < M; ++m) {
        double bd = inf; int bj = F1P_RIV_NONE;
        if (c0 && (m == 0 || argmin_better(pd, pj, d0, j0))) { bd = d0; bj = j0; }
        if (more) {
            for (int k = begin + 64 + lane; k < end; k += 64) {
                const int j = mem ? mem[k] : k;
                const double dx = st[(size_t)j * stride] - xi, dy = st[(size_t)j * stride + 1] - yi;
                const double d2 = dx * dx + dy * dy;
                const bool cand = (j != e) & !(d2 > reach2) & (m == 0 || argmin_better(pd, pj, d2, j));
                if (cand && argmin_better(d2, j, bd, bj)) { bd = d2; bj = j; }
            }
        }
        wave_argmin_2step(bd, bj);                                    // (every lane of the wave is here: the loop above has reconverged)
        if (bj == F1P_RIV_NONE) break;                                // no candidate left (a real one, even at d2 = +inf, carries a smaller index)
        if (lane == m) myj = bj;
        pd = bd; pj = bj;
    }

    if (lane < M) {
        const size_t o = (size_t)e * M + lane;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = -1.0;     // the empty slot
        if (myj >= 0) {
            const double* s = st + (size_t)myj * stride;
            double h = s[ih];
            if (ib >= 0) h = h + s[ib];
            double sn, cs;
            sincos(h, &sn, &cs);                                      // full range: a heading is unbounded here
            const double v = s[iv];
            r0 = s[0]; r1 = s[1]; r2 = v * cs; r3 = v * sn; r4 = radius;
        }
        double* q = obs + o * 5;
        q[0] = r0; q[1] = r1; q[2] = r2; q[3] = r3; q[4] = r4;
        if (idx) idx[o] = myj;
    }
    if (pace && lane == 0) {
        double a = fabs(se[iv]);
        if (!(a >= min_speed)) a = (a != a) ? a : min_speed;          // np.maximum(|v|, min_speed): a NaN speed stays NaN
        pace[e] = 1.0 / a;
    }
}

int launch_rivals(f1p_ctx* ctx, const double* d_states, int layout, int E, int M, double radius, double reach2, double min_speed,
                  const int32_t* d_mem, const int32_t* d_rng, double* d_obs, double* d_pace, int32_t* d_idx) {
    if (E <= 0) return F1P_OK;
    // (stride, speed column, heading column, column added to the heading or -1) of the three layouts
    const int stride = layout == F1P_RIVALS_ST7 ? 7 : 4;
    const int iv = layout == F1P_RIVALS_XYVYAW ? 2 : 3;
    const int ih = layout == F1P_RIVALS_XYVYAW ? 3 : layout == F1P_RIVALS_POSE ? 2 : 4;
    const int ib = layout == F1P_RIVALS_ST7 ? 6 : -1;
    hipLaunchKernelGGL(k_rivals, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, stride, iv, ih, ib, E, M, radius, reach2, min_speed, d_mem,
                       d_rng, d_obs, d_pace, d_idx);
    return check_hip(ctx, hipGetLastError(), "k_rivals launch");
}

}  // namespace f1p
