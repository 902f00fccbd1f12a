// tracker_device.h -- device helpers of the waypoint trackers, shared by the single-raceline kernels (k_controllers.hip) and their
// track-set twins (k_tracks.hip): the front-axle errors of Stanley / LQR and the LQR's Riccati iteration, moved here unchanged from
// k_controllers.hip (whose ISA is the same as before the move), the reference extraction of the kinematic MPC, and the per-ego
// track look-up of the track-set kernels (k_tracks.hip and the lattice planner's track plans).
#pragma once
#include "f1p_internal.h"

namespace f1p {

struct FrontErr { double theta_e, ef; int idx; };

// front-axle point -> nearest raceline segment -> cross-track and heading error (stanley.py:57-88 == lqr.py:60-103)
__device__ __forceinline__ FrontErr front_axle_errors(double x, double y, double theta, double wheelbase,
                                                      const double* __restrict__ wx, const double* __restrict__ wy,
                                                      const double* __restrict__ wpsi, const double* __restrict__ wbox, int n) {
    // executed by ONE wave: all 64 lanes call it with the same arguments and get the same result
    const double fx = x + wheelbase * cos(theta);            // stanley.py:66
    const double fy = y + wheelbase * sin(theta);            // :67
    double bd; int bi;
    nearest_scan_boxed(fx, fy, wx, wy, wbox, n, threadIdx.x & 63, 64, bd, bi);   // :69
    wave_argmin(bd, bi);
    const SegProj s = seg_project(fx, fy, wx[bi], wy[bi], wx[bi + 1], wy[bi + 1]);
    const double vx = fx - s.qx, vy = fy - s.qy;             // :70
    FrontErr r;
    r.ef = dot2(vx, vy, cos(theta - F1P_PI / 2.0), sin(theta - F1P_PI / 2.0));   // :73-75 (np.dot)
    double te = wpsi[bi] - theta;                            // :79-80 pi_2_pi: a single wrap
    if (te > F1P_PI) te = te - 2.0 * F1P_PI;
    else if (te < -F1P_PI) te = te + 2.0 * F1P_PI;
    r.theta_e = te;
    r.idx = bi;
    return r;
}

// row-major 4x4 product
__device__ __forceinline__ void mat4_mul(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            c[4 * i + j] = s;
        }
}

// solve_lqr (utils/utils.py:167-205) for one input: pinv of the 1x1 matrix R + B^T P B is a reciprocal
__device__ void solve_lqr4(const double* A, const double* B, const double* q, double R, double tolerance, int max_iter, double* K) {
    double AT[16], P[16], Pn[16], T1[16], T2[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { AT[4 * i + j] = A[4 * j + i]; P[4 * i + j] = (i == j) ? q[i] : 0.0; }   // P = Q  :190
    int it = 0;
    double diff = __builtin_huge_val();
    while (it < max_iter && diff > tolerance) {                // :194
        ++it;
        mat4_mul(AT, P, T1);                                   // A^T P
        mat4_mul(T1, A, T2);                                   // A^T P A
        double atpb[4], pb[4], btp[4], btpa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double s = 0.0, s2 = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { s += T1[4 * i + k] * B[k]; s2 += P[4 * i + k] * B[k]; }
            atpb[i] = s; pb[i] = s2;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += B[k] * P[4 * k + j];
            btp[j] = s;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += btp[k] * A[4 * k + j];
            btpa[j] = s;
        }
        double btpb = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) btpb += btp[k] * B[k];   /* (B^T P) B, the order numpy evaluates BT @ P @ B */
        const double den = R + btpb;
        const double inv = den != 0.0 ? 1.0 / den : 0.0;
        double mx = -__builtin_huge_val();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Pn[4 * i + j] = T2[4 * i + j] - atpb[i] * inv * btpa[j] + ((i == j) ? q[i] : 0.0);   // :196-197
                const double d = Pn[4 * i + j] - P[4 * i + j];
                if (d > mx) mx = d;
            }
        diff = fabs(mx);                                       // :200 np.abs(np.max(P_next - P))
#pragma unroll
        for (int i = 0; i < 16; ++i) P[i] = Pn[i];
    }
    double btp[4], pb[4], btpa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { s += B[k] * P[4 * k + j]; s2 += P[4 * j + k] * B[k]; }
        btp[j] = s; pb[j] = s2;
    }
    double btpb = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) btpb += btp[k] * B[k];   /* (B^T P) B, the order numpy evaluates BT @ P @ B */
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s += btp[k] * A[4 * k + j];
        btpa[j] = s;
    }
    const double den = btpb + R;
    const double inv = den != 0.0 ? 1.0 / den : 0.0;           // :203
#pragma unroll
    for (int j = 0; j < 4; ++j) K[j] = inv * btpa[j];
}

struct LqrParams { double wheelbase, ts, q[4], r, eps; int max_iter; };

// calc_ref_trajectory_kinematic :189-205 for ego e of a workgroup whose threads take the steps j = threadIdx.x, + blockDim.x, ... of the
// horizon: ind = the nearest segment (:180); (wx, wy, wv, wpsi, n) = the course the ego follows; ref [E][4][T+1].  The statements of
// k_kmpc_ref's epilogue (k_kmpc.hip), which keeps its own inline copy: called from there, this function gives the same results but an
// ISA with one integer add's operands swapped, and that kernel's ISA stays as it was.
__device__ __forceinline__ void kmpc_ref_rows(double v, double yaw, int ind, int e, int T, double dt, double dl, const double* wx,
                                              const double* wy, const double* wv, const double* wpsi,
                                              int n, int yaw_fixup, double* ref) {
    const double travel = fabs(v) * dt;   // :189
    const double dind = travel / dl;      // :190
    for (int j = threadIdx.x; j <= T; j += blockDim.x) {
        double cum = 0.0;                 // np.cumsum(np.repeat(dind, TK)): sequential adds  :191-193
        for (int q = 0; q < j; ++q) cum += dind;
        int il = ind + (int)cum;
        if (il >= n) il -= n;             // :194 single wrap
        if (il < 0 || il >= n) il = il < 0 ? 0 : n - 1;   // the reference would raise IndexError; clamp instead
        double cyw = wpsi[il];            // in-place fix-up of :198-203 applied to the gathered view
        if (yaw_fixup) {                  // (0: the caller folds its array itself, persistently, like the reference)
            if (cyw - yaw > 4.5) cyw = fabs(cyw - (2 * F1P_PI));
            if (cyw - yaw < -4.5) cyw = fabs(cyw + (2 * F1P_PI));
        }
        double* r = ref + (size_t)e * 4 * (T + 1);
        r[0 * (T + 1) + j] = wx[il];
        r[1 * (T + 1) + j] = wy[il];
        r[2 * (T + 1) + j] = wv[il];
        r[3 * (T + 1) + j] = cyw;
    }
}

// one track of the set, as the single-raceline kernels see the context's raceline
struct TrackView {
    const double *x, *y, *v, *psi, *kappa, *box;
    int n, off;
};

// the track of ego e (every lane of the calling wave passes the same e): false for an id outside [0, K)
__device__ __forceinline__ bool track_of(const TrackSetDev& ts, const int32_t* __restrict__ track_id, int e, TrackView& tv) {
    const int k = __builtin_amdgcn_readfirstlane(track_id[e]);
    if (k < 0 || k >= ts.K) return false;                   // wave-uniform
    const int4 t = ts.tab[k];
    const int off = __builtin_amdgcn_readfirstlane(t.x), n = __builtin_amdgcn_readfirstlane(t.y), bo = __builtin_amdgcn_readfirstlane(t.z);
    tv.x = ts.x + off; tv.y = ts.y + off; tv.v = ts.v + off;
    tv.psi = ts.psi ? ts.psi + off : nullptr;
    tv.kappa = ts.kappa ? ts.kappa + off : nullptr;
    tv.box = ts.box + 4 * (size_t)bo;
    tv.n = n; tv.off = off;
    return true;
}

}  // namespace f1p
