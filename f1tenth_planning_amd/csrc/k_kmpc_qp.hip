// k_kmpc_qp.hip -- the reference's linearised kinematic MPC QP (control/kinematic_mpc/kinematic_mpc.py:245-508), solved per ego in fp64.
//
// Per ego, in one launch:
//   1. linearisation point (:452-475): (v_t, phi_t), t < T, of predict_motion_kinematic(x0, oa_prev, od_prev) -- the previous solution,
//      NOT shifted -- through kmpc_step<false>, the step of k_kmpc_predict; get_kinematic_model_matrix(v_t, phi_t, 0) (:245-278)
//   2. condensing: x = S u + s (s: the free response of the linear model, S: one column per input), so the objective of :324-331 becomes
//      1/2 u'Hu + g'u + c over u = vec(uk) = (a_0, d_0, a_1, d_1, ...), n = 2T
//   3. the interior point of qp_ipm.h (with its refinement step) on  G u <= h  with the bounds of :379-389:
//        a upper / lower, delta upper / lower (unit rows), rate upper / lower (first differences of delta),
//        v_1..T upper / lower (DTK x prefix sums of a; v_0 is x0's speed: feasible iff MIN_SPEED <= v0 <= MAX_SPEED)
//      G is never formed: G'DG in the Newton matrix is O(n^2) from suffix sums.
//
// Mapping: a group of G lanes per ego (G = 64: one ego per wave, T <= 32; G = 16: four egos per wave, T <= 8).  Lane i owns input u_i,
// row i of H and of the Newton matrix, and the four inequality rows next to it:
//   i = 2t   (a_t):     a_t upper, a_t lower, v_{t+1} upper, v_{t+1} lower
//   i = 2t+1 (delta_t): delta_t upper, delta_t lower, rate_t upper, rate_t lower (none for t = T-1)
// An ego's result does not depend on its neighbours (tests/test_gpu_kmpc_qp.py: batch invariance).
//
// AV (f1p_kmpc_qp_avoid_*): moving-disc avoidance.  One slack eps is input number 2T (n + 1 lanes per ego: G = 32, two egos
// per wave, while 2T + 1 <= 32, else G = 64; T <= 31), cost rho eps^2 + lin eps, row -eps <= 0.  Per step t = 1..T the two live discs with
// the least clearance at the linearisation path's point pbar_t give half-planes  -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - (r + margin);
// step t's first row is the fifth row of lane 2(t-1) (a_{t-1}), its second that of lane 2(t-1)+1 (delta_{t-1}), the eps lane's fifth row
// is -eps <= 0.  The rows' u-coefficients are dense: kept in LDS (A, one row per lane, odd stride) before S becomes the Newton matrix.
// The disc load, the choice of the two discs, the half-plane and its `planes` record are qp_avoid.h's, shared with k_stmpc_qp.hip.
//
// WALL (f1p_kmpc_qp_walls_*): the AV variant whose two rows per step are the two nearest of {the two nearest live discs, the
// wall to the left of pbar_t, the wall to its right} on the active occupancy bitmap.  The two lanes of a step march one side each (lane
// 2(t-1) left, lane 2(t-1)+1 right: n_samples independent bit tests, qp_walls.h), swap their first hits, and each takes its own of the four
// candidates; from the half-plane on everything is the AV variant's.  M = 0 (no discs) is allowed here.
#include "qp_walls.h"

namespace f1p {

namespace {

// One ego's LDS, carved from b in doubles: the kernel's pointers (P = double*), or with P = int from 0 the members' offsets, `end` the
// size.  extra: the QP's inputs beyond u (nq = n + extra; AV: the slack).
template <class P>
struct QpLdsT {
    P S{}, M{}, H{}, U{}, W{}, Y{}, SUF{}, x0{}, ref{}, fr{}, vb{}, pb{}, cp{}, sp{}, pa{}, pd{}, end{};
    __host__ __device__ constexpr QpLdsT(P b, int T, int extra = 0) {
        const int n = 2 * T, Tp = T + 1, nq = n + extra;
        S = b; M = b; b += 4 * Tp * n;             // S until H and g are formed, then the Newton matrix (nq * nq <= 4 (T+1) n)
        H = b; b += nq * nq;
        U = b; b += nq; W = b; b += nq; Y = b; b += nq;
        SUF = b; b += T;
        x0 = b; b += 4;
        ref = b; b += 4 * Tp;
        fr = b; b += 4 * Tp;
        vb = b; b += T; pb = b; b += T; cp = b; b += T; sp = b; b += T; pa = b; b += T; pd = b; b += T;
        end = b;
    }
};
// the avoidance variant's: nq = n + 1 inputs, and behind the common members the avoidance rows A [n][nq] (odd stride: a lane per row reads
// conflict-free), their published w / D WA [nq], pbar_1..T (x, y, yaw), the discs [16][5]
template <class P>
struct QpLdsAvT : QpLdsT<P> {
    P A{}, WA{}, px{}, py{}, pw{}, ob{};
    __host__ __device__ constexpr QpLdsAvT(P b, int T) : QpLdsT<P>(b, T, 1) {
        const int n = 2 * T, nq = n + 1;
        b = this->end;
        A = b; b += n * nq;
        WA = b; b += nq;
        px = b; b += T; py = b; b += T; pw = b; b += T;
        ob = b; b += 5 * F1P_KMPC_MAX_OBS;
        this->end = b;
    }
};
template <bool AV> using QpLds = std::conditional_t<AV, QpLdsAvT<double*>, QpLdsT<double*>>;
// doubles of LDS per ego
__host__ __device__ constexpr int qp_lds_doubles(int T, bool av) { return av ? QpLdsAvT<int>(0, T).end : QpLdsT<int>(0, T).end; }

}  // namespace

// AvArgs: none (the plain QP), one QpAvoidArgs (AV; f1p_internal.h), or a QpAvoidArgs and a QpWallArgs (WALL)
template <int G, class... AvArgs>
__global__ __launch_bounds__(64) void k_kmpc_qp(const double* __restrict__ x0g, const double* __restrict__ refg,
                                                const double* pa_g, const double* pd_g, int pstride, int E, f1p_kmpc_cfg cfg,
                                                int max_iter, double tol, double* __restrict__ steer, double* __restrict__ speed,
                                                int32_t* __restrict__ status, double* __restrict__ u_out, double* __restrict__ xk_out,
                                                double* __restrict__ obj_out, double* __restrict__ duals, int32_t* __restrict__ iters_out,
                                                double* warm_out, AvArgs... av_args) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr bool AV = sizeof...(AvArgs) >= 1;
    constexpr bool WALL = sizeof...(AvArgs) == 2;
    [[maybe_unused]] const QpAvoidArgs av = qp_avoid_args(av_args...);
    constexpr int EPW = 64 / G;
    constexpr int R = AV ? 5 : 4;                  // inequality rows per lane
    const int T = cfg.horizon, n = 2 * T, Tp = T + 1;
    const int nq = AV ? n + 1 : n;                 // the QP's inputs: u, and eps with AV
    const int grp = threadIdx.x / G, i = threadIdx.x % G;
    const int e = blockIdx.x * EPW + grp;
    const bool ego = e < E;
    QpLds<AV> L(reinterpret_cast<double*>(lds_raw) + (size_t)grp * qp_lds_doubles(T, AV), T);
    const int tau = i >> 1, j = i & 1;
    const bool in_n = i < n;
    const double DTK = cfg.dt;
    const double NaN = __builtin_nan("");

    // ---- inputs -> LDS; finiteness ----------------------------------------------------------------------------------------------------
    bool bad = false;
    if (ego) {
        for (int k = i; k < 4; k += G) { const double v = x0g[(size_t)e * 4 + k]; L.x0[k] = v; bad |= !isfinite(v); }
        for (int k = i; k < 4 * Tp; k += G) { const double v = refg[(size_t)e * 4 * Tp + k]; L.ref[k] = v; bad |= !isfinite(v); }
        for (int k = i; k < T; k += G) {
            const double a = pa_g ? pa_g[((size_t)e * T + k) * pstride] : 0.0;
            const double d = pd_g ? pd_g[((size_t)e * T + k) * pstride] : 0.0;
            L.pa[k] = a; L.pd[k] = d; bad |= !(isfinite(a) && isfinite(d));
        }
        if constexpr (AV) bad |= qp_avoid_load<G>(av, e, i, L.ob);
    }
    bad = gmax<G>(bad ? 1.0 : 0.0) > 0.0;
    __syncthreads();
    const double v0 = ego ? L.x0[2] : 0.0;
    int st = !ego ? 0 : bad ? 3 : (v0 >= cfg.min_speed && v0 <= cfg.max_speed) ? 0 : 1;    // status 1: the t = 0 speed bound cannot hold
    bool done = !ego || st != 0;

    // ---- 1. linearisation point and the free response of the linear model ---------------------------------------------------------------
    if (i == 0 && !done) {
        KmpcStep s;
        s.x = L.x0[0]; s.y = L.x0[1]; s.v = L.x0[2]; s.yaw = L.x0[3];
        double fx = s.x, fy = s.y, fv = s.v, fw = s.yaw;
        L.fr[0] = fx; L.fr[Tp] = fy; L.fr[2 * Tp] = fv; L.fr[3 * Tp] = fw;
        for (int t = 0; t < T; ++t) {
            const double vb = s.v, pb = s.yaw;          // path_predict[2, t], path_predict[3, t]
            double sn, cs;
            sincos(pb, &sn, &cs);
            L.vb[t] = vb; L.pb[t] = pb; L.cp[t] = cs; L.sp[t] = sn;
            // A x + C with delta_bar = 0: A[3, 2] = 0, C[3] = 0 (:262-276)
            const double nx = fx + DTK * cs * fv + (-DTK * vb * sn) * fw + DTK * vb * sn * pb;
            const double ny = fy + DTK * sn * fv + (DTK * vb * cs) * fw + (-DTK * vb * cs * pb);
            fx = nx; fy = ny;
            L.fr[t + 1] = fx; L.fr[Tp + t + 1] = fy; L.fr[2 * Tp + t + 1] = fv; L.fr[3 * Tp + t + 1] = fw;
            kmpc_step<false>(s, L.pa[t], L.pd[t], cfg);
            if constexpr (AV) { L.px[t] = s.x; L.py[t] = s.y; L.pw[t] = s.yaw; }      // pbar_{t+1}
        }
    }
    __syncthreads();

    // ---- 2. condensing: column i of S, then row i of H and g_i ---------------------------------------------------------------------------
    if (in_n && !done) {
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
        for (int t = 0; t < Tp; ++t) {
            if (t == tau + 1) {                          // B_tau e_j: B[2, 0] = DTK, B[3, 1] = DTK v / WB (cos(0)^2 = 1)
                if (j == 0) d2 = DTK; else d3 = DTK * L.vb[tau] / cfg.wheelbase;
            } else if (t > tau + 1) {                    // A_{t-1} d
                const int q = t - 1;
                const double n0 = d0 + DTK * L.cp[q] * d2 + (-DTK * L.vb[q] * L.sp[q]) * d3;
                const double n1 = d1 + DTK * L.sp[q] * d2 + (DTK * L.vb[q] * L.cp[q]) * d3;
                d0 = n0; d1 = n1;
            }
            L.S[(4 * t + 0) * n + i] = d0; L.S[(4 * t + 1) * n + i] = d1; L.S[(4 * t + 2) * n + i] = d2; L.S[(4 * t + 3) * n + i] = d3;
        }
    }
    __syncthreads();
    double g = 0.0;
    if (in_n && !done) {
        for (int t = 1; t < Tp; ++t) {
            const double* w = t == T ? cfg.qf : cfg.q;
#pragma unroll
            for (int k = 0; k < 4; ++k) g += 2.0 * w[k] * L.S[(4 * t + k) * n + i] * (L.fr[k * Tp + t] - L.ref[k * Tp + t]);
        }
        for (int c = 0; c < n; ++c) {
            double h = 0.0;
            for (int t = 1; t < Tp; ++t) {
                const double* w = t == T ? cfg.qf : cfg.q;
#pragma unroll
                for (int k = 0; k < 4; ++k) h += 2.0 * w[k] * L.S[(4 * t + k) * n + i] * L.S[(4 * t + k) * n + c];
            }
            if (c == i) h += 2.0 * (cfg.r[j] + ((tau > 0) + (tau < T - 1)) * cfg.rd[j]);
            if (c == i - 2 || c == i + 2) h -= 2.0 * cfg.rd[j];
            L.H[i * nq + c] = h;
        }
        if constexpr (AV) L.H[i * nq + n] = 0.0;
    }
    // AV: this lane's half-plane (step tau + 1, the j-th nearest live disc), its row of A, and the eps lane's row of H
    [[maybe_unused]] QpPlane pl;
    if constexpr (WALL) {
        // this lane's side of step tau + 1 (j = 0: left, j = 1: right) marched from pbar, the first hits swapped between the step's two
        // lanes, then the j-th of the four candidates.  (The swap is outside the branch: lanes 2 tau and 2 tau + 1 are in or out of it together.)
        const QpWallArgs wl = qp_wall_args(av_args...);
        const bool act = in_n && !done;
        const int t = tau + 1;
        double px = 0.0, py = 0.0, llx = 0.0, lly = 0.0;                  // pbar and the LEFT direction (the right one is its negative)
        int ks = 0;
        if (act) {
            double sn, cs;
            px = L.px[tau]; py = L.py[tau];
            sincos(L.pw[tau], &sn, &cs);
            llx = -sn; lly = cs;
            ks = j == 0 ? qp_wall_march(wl, px, py, llx, lly) : qp_wall_march(wl, px, py, -llx, -lly);
        }
        const int ko = __shfl_xor(ks, 1);
        if (act) {
            const double tt = (double)t * DTK;
            const QpNearest nr = qp_avoid_nearest(L.ob, av.M, px, py, tt);
            const QpCand d0 = qp_disc_cand(L.ob, nr.m0, px, py, tt), d1 = qp_disc_cand(L.ob, nr.m1, px, py, tt);
            const QpWallCand wL = qp_wall_cand(wl, px, py, llx, lly, j == 0 ? ks : ko, F1P_QP_WALL_SLOT_L);
            const QpWallCand wR = qp_wall_cand(wl, px, py, -llx, -lly, j == 0 ? ko : ks, F1P_QP_WALL_SLOT_R);
            const int pick = qp_select4(d0, d1, wL, wR, j);
            if (pick == 0 || pick == 1) pl = qp_avoid_plane(L.ob, pick == 0 ? nr.m0 : nr.m1, px, py, L.pw[tau], tt, L.fr[t], L.fr[Tp + t], av.margin);
            else if (pick == 2) pl = qp_wall_plane(wL, llx, lly, L.fr[t], L.fr[Tp + t], wl.margin);
            else if (pick == 3) pl = qp_wall_plane(wR, -llx, -lly, L.fr[t], L.fr[Tp + t], wl.margin);
            for (int c = 0; c < n; ++c)
                L.A[i * nq + c] = pl.slot >= 0 ? -(pl.nx * L.S[(4 * t + 0) * n + c] + pl.ny * L.S[(4 * t + 1) * n + c]) : 0.0;
        }
    } else if constexpr (AV) {
        if (in_n && !done) {
            const int t = tau + 1;
            const double tt = (double)t * DTK, px = L.px[tau], py = L.py[tau];
            const QpNearest nr = qp_avoid_nearest(L.ob, av.M, px, py, tt);
            const int ms = j == 0 ? nr.m0 : nr.m1;
            if (ms >= 0) pl = qp_avoid_plane(L.ob, ms, px, py, L.pw[tau], tt, L.fr[t], L.fr[Tp + t], av.margin);
            for (int c = 0; c < n; ++c)
                L.A[i * nq + c] = pl.slot >= 0 ? -(pl.nx * L.S[(4 * t + 0) * n + c] + pl.ny * L.S[(4 * t + 1) * n + c]) : 0.0;
        }
    }
    if constexpr (AV) {
        if (i == n && !done) {
            for (int c = 0; c < n; ++c) L.H[n * nq + c] = 0.0;
            L.H[n * nq + n] = 2.0 * av.rho;
            g = av.lin;
        }
    }

    // ---- 3. interior point (qp_ipm.h) ----------------------------------------------------------------------------------------------------
    const double MD = cfg.max_dsteer * DTK;
    double h[R];
    bool valid[R];
    if (j == 0) { h[0] = cfg.max_accel; h[1] = cfg.max_accel; h[2] = cfg.max_speed - v0; h[3] = v0 - cfg.min_speed; }
    else        { h[0] = cfg.max_steer; h[1] = cfg.max_steer; h[2] = MD; h[3] = MD; }
#pragma unroll
    for (int r = 0; r < 4; ++r) valid[r] = in_n && (j == 0 || r < 2 || tau < T - 1);
    double m_rows = 8.0 * T - 2.0;
    if constexpr (AV) {
        h[4] = in_n ? pl.h : 0.0;
        valid[4] = in_n ? pl.slot >= 0 : i == n;
        m_rows += 1.0 + gsum<G>(in_n && pl.slot >= 0 ? 1.0 : 0.0);
    }

    // G x for this lane's rows (x published in vec[])
    auto gmul = [&](const double* vec, const double (&x)[1], double (&out)[R]) {
        const double xi = x[0];
        if (!in_n) {
            out[0] = out[1] = out[2] = out[3] = 0.0;
        } else if (j == 0) {
            double pre = 0.0;
            for (int q = 0; q <= tau; ++q) pre += vec[2 * q];
            out[0] = xi; out[1] = -xi; out[2] = DTK * pre; out[3] = -(DTK * pre);
        } else {
            const double r = tau < T - 1 ? vec[i + 2] - xi : 0.0;
            out[0] = xi; out[1] = -xi; out[2] = r; out[3] = -r;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = valid[r] ? out[r] : 0.0;
        if constexpr (AV) {                                  // A_i . u - eps; the eps lane: -eps  (A_i is zero from column 2 (tau + 1))
            double o = 0.0;
            if (valid[4]) {
                if (in_n) for (int c = 0; c < 2 * tau + 2; ++c) o += L.A[i * nq + c] * vec[c];
                o -= vec[n];
            }
            out[4] = o;
        }
    };
    // (G' w)_i: the rows' w_2 - w_3 published in W[]
    auto gtmul = [&](const double (&w)[R], double (&o)[1]) {
        double w2 = valid[2] ? w[2] - w[3] : 0.0;
        __syncthreads();
        if (in_n) L.W[i] = w2;
        if constexpr (AV) { if (i < nq) L.WA[i] = valid[4] ? w[4] : 0.0; }
        __syncthreads();
        o[0] = (valid[0] ? w[0] : 0.0) - (valid[1] ? w[1] : 0.0);
        if (!in_n) {
            o[0] = 0.0;
        } else if (j == 0) {
            double suf = 0.0;
            for (int q = T - 1; q >= tau; --q) suf += L.W[2 * q];
            o[0] += DTK * suf;
        } else {
            o[0] += -w2 + (tau > 0 ? L.W[i - 2] : 0.0);
        }
        if constexpr (AV) {                                  // column i of A over the rows of steps > tau; the eps lane: minus every row's w
            if (in_n) {
                double a = 0.0;
                for (int r = 2 * tau; r < n; ++r) a += L.A[r * nq + i] * L.WA[r];
                o[0] += a;
            } else if (i == n) {
                double a = 0.0;
                for (int r = 0; r < nq; ++r) a += L.WA[r];
                o[0] = -a;
            }
        }
    };
    // row i of M = H + G' diag(D) G, lower triangle: a diagonal, the rate rows' tridiagonal (delta), DTK^2 x suffix sums of the
    // v rows' D over max(tau, c / 2) (a)
    // AV: + sum_r D_r A_r A_r' on the u block, -sum_r D_r A_r in the eps row, 2 rho + sum_r D_r + D_eps on its diagonal
    auto newton_rows = [&](const double (&D)[R]) {
        __syncthreads();
        if (in_n) L.W[i] = D[2] + D[3];
        if constexpr (AV) { if (i < nq) L.WA[i] = D[4]; }
        __syncthreads();
        if (j == 0 && in_n) {
            double suf = 0.0;
            for (int q = T - 1; q >= tau; --q) suf += L.W[2 * q];
            L.SUF[tau] = suf;
        }
        __syncthreads();
        if (in_n) {
            for (int c = 0; c <= i; ++c) {
                double m = L.H[i * nq + c];
                if (j == 0 && (c & 1) == 0) m += DTK * DTK * L.SUF[max(tau, c >> 1)];
                if (c == i) m += D[0] + D[1] + (j == 1 ? L.W[i] + (tau > 0 ? L.W[i - 2] : 0.0) : 0.0);
                if (j == 1 && c == i - 2) m -= L.W[i - 2];
                if constexpr (AV) {
                    double a = 0.0;
                    for (int r = 2 * tau; r < n; ++r) a += L.WA[r] * L.A[r * nq + i] * L.A[r * nq + c];
                    m += a;
                }
                L.M[i * nq + c] = m;
            }
        }
        if constexpr (AV) {
            if (i == n) {
                double sd = 0.0;
                for (int r = 0; r < nq; ++r) sd += L.WA[r];
                for (int c = 0; c < n; ++c) {
                    double a = 0.0;
                    for (int r = c & ~1; r < n; ++r) a += L.WA[r] * L.A[r * nq + c];
                    L.M[n * nq + c] = -a;
                }
                L.M[n * nq + n] = 2.0 * av.rho + sd;
            }
        }
    };

    const double gv[1] = {g};
    double u[1], lam[R];
    int it_done;
    qp_ipm<G, 1, R, true>(QpIpmLds{L.H, L.M, L.U, L.Y}, nq, i, gv, h, valid, m_rows, max_iter, tol, done, st, it_done, u, lam, gmul, gtmul,
                    newton_rows);

    // ---- outputs --------------------------------------------------------------------------------------------------------------------
    if (!ego) return;
    const bool ok = st == 0 || st == 2;
    if (in_n) {
        if (u_out) u_out[(size_t)e * n + i] = ok ? u[0] : NaN;
        if (warm_out) warm_out[(size_t)e * n + i] = ok ? u[0] : 0.0;     // a failed solve leaves the reference's oa / od = None: zeros next call
        if (duals) {
            double* du_ = duals + (size_t)e * (8 * T - 2);
            const int R4 = 4 * T, R6 = 6 * T - 2;
            if (j == 0) {
                du_[tau] = ok ? lam[0] : NaN; du_[T + tau] = ok ? lam[1] : NaN;
                du_[R6 + tau] = ok ? lam[2] : NaN; du_[R6 + T + tau] = ok ? lam[3] : NaN;
            } else {
                du_[2 * T + tau] = ok ? lam[0] : NaN; du_[3 * T + tau] = ok ? lam[1] : NaN;
                if (tau < T - 1) { du_[R4 + tau] = ok ? lam[2] : NaN; du_[R4 + T - 1 + tau] = ok ? lam[3] : NaN; }
            }
        }
        if constexpr (AV) {
            if (av.planes) qp_avoid_write_plane(av.planes + ((size_t)e * n + i) * 4, pl, ok);
            if (av.duals) av.duals[(size_t)e * nq + i] = ok ? lam[4] : NaN;
        }
    }
    if constexpr (AV) {
        if (i == n) {
            if (av.duals) av.duals[(size_t)e * nq + n] = ok ? lam[4] : NaN;
            if (av.eps) av.eps[e] = ok ? u[0] : NaN;
        }
    }
    if (i == 0) {
        if (status) status[e] = st;
        if (iters_out) iters_out[e] = ok ? it_done : 0;
        steer[e] = ok ? L.U[1] : NaN;                                   // :503
        speed[e] = ok ? v0 + L.U[0] * DTK : NaN;                        // :505
        if (xk_out || obj_out) {
            // x_{t+1} = A_t x_t + B_t u_t + C_t and the objective cvxpy reports (:324-331), the constant t = 0 term included
            double x = L.x0[0], y = L.x0[1], v = L.x0[2], w = L.x0[3], f = 0.0;
            double* xo = xk_out ? xk_out + (size_t)e * 4 * Tp : nullptr;
            for (int t = 0; t < Tp; ++t) {
                if (xo) { xo[t] = ok ? x : NaN; xo[Tp + t] = ok ? y : NaN; xo[2 * Tp + t] = ok ? v : NaN; xo[3 * Tp + t] = ok ? w : NaN; }
                const double* q = t == T ? cfg.qf : cfg.q;
                const double ex = x - L.ref[t], ey = y - L.ref[Tp + t], ev = v - L.ref[2 * Tp + t], ew = w - L.ref[3 * Tp + t];
                f += q[0] * ex * ex + q[1] * ey * ey + q[2] * ev * ev + q[3] * ew * ew;
                if (t == T) break;
                const double a = L.U[2 * t], d = L.U[2 * t + 1];
                f += cfg.r[0] * a * a + cfg.r[1] * d * d;
                if (t < T - 1) {
                    const double da = L.U[2 * t + 2] - a, dd = L.U[2 * t + 3] - d;
                    f += cfg.rd[0] * da * da + cfg.rd[1] * dd * dd;
                }
                const double vb = L.vb[t], pb = L.pb[t], cs = L.cp[t], sn = L.sp[t];
                const double nx = x + DTK * cs * v + (-DTK * vb * sn) * w + DTK * vb * sn * pb;
                const double ny = y + DTK * sn * v + (DTK * vb * cs) * w + (-DTK * vb * cs * pb);
                const double nv = v + DTK * a;
                const double nw = w + (DTK * vb / cfg.wheelbase) * d;
                x = nx; y = ny; v = nv; w = nw;
            }
            if constexpr (AV) f += av.rho * L.U[n] * L.U[n] + av.lin * L.U[n];
            if (obj_out) obj_out[e] = ok ? f : NaN;
        }
    }
}

#ifndef F1P_KMPC_QP_PACK_T8
#define F1P_KMPC_QP_PACK_T8 4         // egos per wave at T <= 8 (1 or 4)
#endif

static int kmpc_qp_pack(const f1p_ctx* ctx, int T) {
    if (T > 8) return 1;
    return ctx->kmpc_qp_pack > 0 ? ctx->kmpc_qp_pack : F1P_KMPC_QP_PACK_T8;
}

// egos per wave: the plain QP four or one (kmpc_qp_pack); the avoidance variant, 2T + 1 lanes per ego, two while they fit 32 lanes
// (T <= 15), else one; the wall variant as the avoidance variant
int launch_kmpc_qp(f1p_ctx* ctx, int E, const f1p_kmpc_cfg* cfg, int max_iter, double tol, const QpIo& io, const QpAvoidArgs* avoid,
                   const QpWallArgs* walls) {
    if (E <= 0) return F1P_OK;
    const int T = cfg->horizon;
    if (avoid && (T > 31 || avoid->M < 0 || avoid->M > F1P_KMPC_MAX_OBS || (avoid->M > 0 && !avoid->obs)))
        return set_error(ctx, F1P_EINVAL, "kmpc qp avoid: bad horizon / obstacles");
    if (walls && (!avoid || !walls->g.bits || walls->g.w < 1 || walls->g.h < 1 || walls->n_samples < 1 || walls->n_samples > F1P_KMPC_QP_WALL_MAX_SAMPLES))
        return set_error(ctx, F1P_EINVAL, "kmpc qp walls: bad grid / n_samples");
    const int epw = avoid ? (2 * T + 1 <= 32 ? 2 : 1) : (kmpc_qp_pack(ctx, T) == 4 ? 4 : 1);
    const size_t lds = sizeof(double) * (size_t)qp_lds_doubles(T, avoid != nullptr) * epw;
    const auto launch = [&](auto kern, const char* what, auto... av) {
        const int rc = qp_lds_opt_in(ctx, reinterpret_cast<const void*>(kern), lds, "kmpc qp: horizon too long for the CU's LDS");
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)((E + epw - 1) / epw)), dim3(64), lds, ctx->stream, io.x0, io.ref, io.pa, io.pd, io.pstride, E,
                           *cfg, max_iter, tol, io.steer, io.speed, io.status, io.u, io.x, io.obj, io.duals, io.iters, io.warm_out, av...);
        return check_hip(ctx, hipGetLastError(), what);
    };
    if (walls) return epw == 2 ? launch(&k_kmpc_qp<32, QpAvoidArgs, QpWallArgs>, "k_kmpc_qp_walls launch", *avoid, *walls)
                               : launch(&k_kmpc_qp<64, QpAvoidArgs, QpWallArgs>, "k_kmpc_qp_walls launch", *avoid, *walls);
    if (avoid) return epw == 2 ? launch(&k_kmpc_qp<32, QpAvoidArgs>, "k_kmpc_qp_avoid launch", *avoid)
                               : launch(&k_kmpc_qp<64, QpAvoidArgs>, "k_kmpc_qp_avoid launch", *avoid);
    return epw == 4 ? launch(&k_kmpc_qp<16>, "k_kmpc_qp launch") : launch(&k_kmpc_qp<64>, "k_kmpc_qp launch");
}

}  // namespace f1p
