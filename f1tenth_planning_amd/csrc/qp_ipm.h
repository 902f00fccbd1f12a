// qp_ipm.h -- the batched fp64 interior-point QP solver of k_kmpc_qp and k_stmpc_qp.
//
// One ego's  min 1/2 u'Hu + g'u  s.t.  G u <= h  over n inputs, solved by a group of G lanes with a primal-dual interior-point method
// (Mehrotra predictor-corrector).  Lane l owns inputs P l .. P l + P - 1 (their rows of H and of the Newton matrix) and R inequality
// rows; a row with valid[r] == false is absent.  Stop: |r_d| <= tol (1 + |g|), |r_p| <= tol (1 + |h|) and s'lambda <= tol (max-norms),
// or max_iter (status 2: last iterate).  With Refine an ego that meets the rule takes ONE more step before it stops (not counted in
// it_done, not subject to max_iter): at a degenerate row slack and multiplier both go like the square root of the gap, so the rule
// alone leaves u up to ~sqrt(tol / curvature) from the optimum; the step is kept only if the iterate still meets the rule with a
// smaller gap, else the iterate that met it is returned.  An ego whose Newton matrix stops being numerically positive definite before that (lambda / s
// ~ 1e16 on its active rows) stops there, status 0 when its residuals are below tol and s'lambda <= tol (1 + |objective|), else 2.
//
// The model supplies G through three hooks, called by every lane of the workgroup:
//   gmul(vec, x[P], out[R])   this lane's rows of G x, with x published in vec[]
//   gtmul(w[R], o[P])         this lane's entries of G' w; publishes through LDS, so it holds barriers of its own
//   newton_rows(D[R])         this lane's rows of M = H + G' diag(D) G into QpIpmLds::M, lower triangle only
// Matrices live in LDS (row i written by its owner, the pivot column read as broadcasts); group reductions are xor butterflies of width
// G.  Every ego runs until the last ego of its workgroup stops, but an ego that has stopped takes no further steps, so its result does
// not depend on its neighbours.
#pragma once
#include "f1p_internal.h"

namespace f1p {

template <int G>
__device__ __forceinline__ double gsum(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, G);
    return v;
}
template <int G>
__device__ __forceinline__ double gmax(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {                    // NaN-propagating: a broken-down ego never looks converged
        const double o = __shfl_xor(v, m, G);
        v = (o > v || o != o) ? o : v;
    }
    return v;
}
template <int G>
__device__ __forceinline__ double gmin(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = fmin(v, __shfl_xor(v, m, G));
    return v;
}

// max |x_p| folded from the p = 0 term: fmax drops a NaN, and which NaNs reach gmax decides convergence
template <int P>
__device__ __forceinline__ double lane_absmax(const double (&x)[P]) {
    double a = fabs(x[0]);
#pragma unroll
    for (int p = 1; p < P; ++p) a = fmax(a, fabs(x[p]));
    return a;
}

// one ego's LDS: H and the Newton matrix / its Cholesky factor (n x n, row-major), U (published iterates) and Y (solve) (n each)
struct QpIpmLds {
    const double* H;
    double *M, *U, *Y;
};

// in: g[P] (this lane's entries), h[R], valid[R], m_rows (the number of valid rows of the ego), done (the ego takes no step), st;
// out: u[P], lam[R], st (0 / 2 unless it came in non-zero), it_done; U holds u on return
template <int G, int P, int R, bool Refine = false, class GMul, class GtMul, class NewtonRows>
__device__ __forceinline__ void qp_ipm(const QpIpmLds& L, int n, int lane, const double (&g)[P], const double (&h)[R], const bool (&valid)[R],
                                       double m_rows, int max_iter, double tol, bool done, int& st, int& it_done, double (&u)[P],
                                       double (&lam)[R], GMul&& gmul, GtMul&& gtmul, NewtonRows&& newton_rows) {
    const bool in_n = lane < n / P;
    double s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { s[r] = valid[r] ? fmax(h[r], 1.0) : 1.0; lam[r] = valid[r] ? 1.0 : 0.0; }
    double hmax = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) hmax = fmax(hmax, valid[r] ? fabs(h[r]) : 0.0);
    const double gn = 1.0 + gmax<G>(in_n ? lane_absmax(g) : 0.0), hn = 1.0 + gmax<G>(hmax);
#pragma unroll
    for (int p = 0; p < P; ++p) u[p] = 0.0;
    it_done = 0;
    bool conv = false;                                   // Refine: the rule is met, the refinement step is under way
    double u_c[P], s_c[R], lam_c[R], gap_c = 0.0;        // ... and the iterate that met it

    // publish x in vec[] (barriers on both sides)
    auto publish = [&](double* vec, const double (&x)[P]) {
        __syncthreads();
        if (in_n) {
#pragma unroll
            for (int p = 0; p < P; ++p) vec[P * lane + p] = x[p];
        }
        __syncthreads();
    };

    for (int it = 0;; ++it) {
        // residuals
        publish(L.U, u);
        double Gu[R], rp[R];
        gmul(L.U, u, Gu);
        double rpmax = 0.0, gap = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            rp[r] = valid[r] ? Gu[r] + s[r] - h[r] : 0.0;
            rpmax = fmax(rpmax, fabs(rp[r]));
            gap += valid[r] ? s[r] * lam[r] : 0.0;
        }
        double Hu[P] = {}, gl[P], rd[P];
        if (in_n)
            for (int c = 0; c < n; ++c) {
#pragma unroll
                for (int p = 0; p < P; ++p) Hu[p] += L.H[(P * lane + p) * n + c] * L.U[c];
            }
        gtmul(lam, gl);
#pragma unroll
        for (int p = 0; p < P; ++p) rd[p] = in_n ? Hu[p] + g[p] + gl[p] : 0.0;
        const double rdn = gmax<G>(lane_absmax(rd)) / gn, rpn = gmax<G>(rpmax) / hn;
        gap = gsum<G>(gap);
        double fl = u[0] * (0.5 * Hu[0] + g[0]);
#pragma unroll
        for (int p = 1; p < P; ++p) fl += u[p] * (0.5 * Hu[p] + g[p]);
        const double f = gsum<G>(in_n ? fl : 0.0);
        // converged: residuals and the gap s'lambda below tol.  The gap relative to the objective is the fallback for an ego whose
        // Newton matrix can no longer be factored (lambda / s ~ 1e16 on its active rows) before the absolute gap is reached.
        const bool res_ok = rdn <= tol && rpn <= tol;
        const bool gap_rel_ok = res_ok && gap <= tol * (1.0 + fabs(f));
        if (!done) {
            if (Refine && conv) {                        // after the refinement step: keep it, or go back
                if (!(res_ok && gap <= gap_c)) {
#pragma unroll
                    for (int p = 0; p < P; ++p) u[p] = u_c[p];
#pragma unroll
                    for (int r = 0; r < R; ++r) { s[r] = s_c[r]; lam[r] = lam_c[r]; }
                }
                done = true;
            } else if (res_ok && gap <= tol) {
                st = 0; it_done = it;
                if (Refine) {
                    conv = true; gap_c = gap;
#pragma unroll
                    for (int p = 0; p < P; ++p) u_c[p] = u[p];
#pragma unroll
                    for (int r = 0; r < R; ++r) { s_c[r] = s[r]; lam_c[r] = lam[r]; }
                } else {
                    done = true;
                }
            } else if (it >= max_iter) { done = true; st = 2; it_done = it; }
        }
        if (!__syncthreads_or(!done)) break;

        // Newton matrix M = H + G' diag(lambda / s) G
        double D[R];
#pragma unroll
        for (int r = 0; r < R; ++r) D[r] = valid[r] ? lam[r] / s[r] : 0.0;
        newton_rows(D);
        // Cholesky, in place: lower triangle of M = L.  Each lane scales its rows' pivot-column entries before the barrier, then
        // updates its rows in ascending order.
        bool broke = false;
        for (int k = 0; k < n; ++k) {
            __syncthreads();
            const double mk = L.M[k * n + k];
            broke |= !(mk > 0.0 && mk < INFINITY);
            const double dk = sqrt(mk);
            double l[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int ip = P * lane + p;
                l[p] = 0.0;
                if (in_n && ip > k) { l[p] = L.M[ip * n + k] / dk; L.M[ip * n + k] = l[p]; }
            }
            __syncthreads();
            if (k / P == lane) L.M[k * n + k] = dk;
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int ip = P * lane + p;
                if (in_n && ip > k) for (int c = k + 1; c <= ip; ++c) L.M[ip * n + c] -= l[p] * L.M[c * n + k];
            }
        }
        __syncthreads();
        if (broke && !done) {                            // (broke is uniform over the group)
            done = true;
            if (!conv) { st = gap_rel_ok ? 0 : 2; it_done = it; }                      // (conv: no refinement step; the iterate stands)
        }

        // one Newton solve for the complementarity right-hand side rc
        auto newton = [&](const double (&rc)[R], double (&du)[P], double (&ds)[R], double (&dl)[R]) {
            double w[R], b[P];
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = valid[r] ? (lam[r] * rp[r] - rc[r]) / s[r] : 0.0;
            gtmul(w, b);
#pragma unroll
            for (int p = 0; p < P; ++p) b[p] = -rd[p] - b[p];
            for (int k = 0; k < n; ++k) {                // L y = b
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (P * lane + p == k) { b[p] = b[p] / L.M[k * n + k]; L.Y[k] = b[p]; }
                __syncthreads();
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (in_n && P * lane + p > k) b[p] -= L.M[(P * lane + p) * n + k] * L.Y[k];
            }
            for (int k = n - 1; k >= 0; --k) {           // L' x = y
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (P * lane + p == k) { b[p] = b[p] / L.M[k * n + k]; L.Y[k] = b[p]; }
                __syncthreads();
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (P * lane + p < k) b[p] -= L.M[k * n + P * lane + p] * L.Y[k];
            }
#pragma unroll
            for (int p = 0; p < P; ++p) du[p] = in_n ? b[p] : 0.0;
            double Gd[R];
            publish(L.U, du);
            gmul(L.U, du, Gd);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ds[r] = valid[r] ? -rp[r] - Gd[r] : 0.0;
                dl[r] = valid[r] ? (-rc[r] - lam[r] * ds[r]) / s[r] : 0.0;
            }
        };
        auto step_max = [&](const double (&ds)[R], const double (&dl)[R]) -> double {
            double a = 1.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (valid[r] && ds[r] < 0.0) a = fmin(a, -s[r] / ds[r]);
                if (valid[r] && dl[r] < 0.0) a = fmin(a, -lam[r] / dl[r]);
            }
            return gmin<G>(a);
        };
        const double mu = gap / m_rows;
        double rc[R], du[P], ds[R], dl[R];
#pragma unroll
        for (int r = 0; r < R; ++r) rc[r] = valid[r] ? s[r] * lam[r] : 0.0;
        newton(rc, du, ds, dl);                          // predictor (affine scaling)
        double a = step_max(ds, dl), gap_aff = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) gap_aff += valid[r] ? (s[r] + a * ds[r]) * (lam[r] + a * dl[r]) : 0.0;
        gap_aff = gsum<G>(gap_aff);
        const double ratio = gap_aff / gap, sigma = ratio * ratio * ratio;
#pragma unroll
        for (int r = 0; r < R; ++r) rc[r] = valid[r] ? s[r] * lam[r] + ds[r] * dl[r] - sigma * mu : 0.0;
        newton(rc, du, ds, dl);                          // corrector
        a = fmin(1.0, 0.99 * step_max(ds, dl));
        if (!done) {
#pragma unroll
            for (int p = 0; p < P; ++p) u[p] += a * du[p];
#pragma unroll
            for (int r = 0; r < R; ++r) if (valid[r]) { s[r] += a * ds[r]; lam[r] += a * dl[r]; }
        }
    }
    publish(L.U, u);
}

// dynamic LDS above sharedMemPerBlock: opt the kernel in, up to the CU's LDS; F1P_EINVAL with `too_long` beyond that
inline int qp_lds_opt_in(f1p_ctx* ctx, const void* kern, size_t lds, const char* too_long) {
    if (lds <= (size_t)ctx->prop.sharedMemPerBlock) return F1P_OK;
    if (lds > (size_t)ctx->prop.maxSharedMemoryPerMultiProcessor) return set_error(ctx, F1P_EINVAL, too_long);
    F1P_HIP(ctx, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return F1P_OK;
}

}  // namespace f1p
