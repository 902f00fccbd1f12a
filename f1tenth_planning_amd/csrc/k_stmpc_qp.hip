// k_stmpc_qp.hip -- the reference's linearised dynamic single-track MPC QP (control/dynamic_mpc/dynamic_mpc.py:428-535, :575-710,
// :995-1117), solved per ego in fp64.
//
// Per ego, in one launch:
//   1. linearisation point (linear_mpc_control :995-1040): (delta, v, yaw, yawrate, beta)_t, t < T, of predict_motion(x0, oa, od_v)
//      (:279-300) -- the previous solution, NOT shifted -- through dyn_step<false>, the step of k_stmpc_predict (update_state :317-404,
//      its input and output clamps included); get_dynamic_model_matrix(delta_t, v_t, yaw_t, yawrate_t, beta_t, oa[t]) (:428-535): the
//      dense Jacobian (the previous ACCELERATION enters it through the load-transfer terms).  Non-finite model data (a predicted speed
//      clamped to 0 divides by v) is status 3.
//   2. condensing, without S: x = S u + s (s: the free response of the linear model).  Lane tau holds the two 7-vectors d x_t / d u_tau
//      in registers and steps them forward with A_t; each step writes its slab (7 x n) to LDS and every lane adds its two rows of
//      H = 2 sum_t S_t' Q_t S_t (Qf at T) and of g.  The objective of :616-622 becomes 1/2 u'Hu + g'u + c over
//      u = vec(u) = (steer_v_0, accel_0, steer_v_1, accel_1, ...), n = 2T.
//   3. the interior point of qp_ipm.h on  G u <= h  with the rows of :683-706.  A's rows 2 and 3
//      are unit rows (B[2, 0] = B[3, 1] = DT, C[2] = C[3] = 0), so delta_t = delta0 + DT sum_{k<t} u0_k and v_t = v0 + DT sum_{k<t} u1_k
//      exactly, and every row is a unit row, a first difference of u0 or a DT-scaled prefix sum:
//        steer_v_t upper / lower, accel_t upper / lower (unit rows), delta_{t+1} upper / lower (prefix sums of u0),
//        v_{t+1} upper / lower (prefix sums of u1), rate_t upper / lower (u0_{t+1} - u0_t, :685: no DT factor)
//      (the t = 0 rows are constants: feasible iff |delta0| <= MAX_STEER and MIN_SPEED <= v0 <= MAX_SPEED, then u = 0 is feasible).
//      Newton matrix H + G' diag(lambda / s) G: the u0 block gets a diagonal, a tridiagonal (rate rows) and
//      DT^2 (suffix sum over max(s, s')) (delta rows); the u1 block a diagonal and the same suffix-sum term (v rows); no u0-u1 term.
//      G is never formed.
//
// Mapping: one wave per ego; lane tau owns time step tau -- both inputs (rows 2 tau, 2 tau + 1 of H and of the Newton matrix) and the
// ten inequality rows of step tau -- so T <= 64 on one wave; the LDS of H and the Newton matrix (2 n^2 doubles) bounds T at
// F1P_STMPC_QP_MAX_T.  An ego's arithmetic depends on nothing outside its own workgroup: results are batch invariant.
//
// AV (f1p_stmpc_qp_avoid_*): moving-disc avoidance.  The QP has nq = 2T + 2 inputs: lane T owns the slack eps (input 2T, cost
// rho eps^2 + lin eps, row -eps <= 0; solved for as eps / sig, sig = 1 / sqrt(2 rho)) and a padding input 2T + 1 (H = 1, g = 0, no row: it stays 0) that keeps nq a multiple of the two
// inputs a lane owns.  Lane t - 1 owns the two avoidance rows of step t (rows 10 and 11 of its twelve): the two live discs with the least
// clearance at the linearisation path's point pbar_t give  -n.(S_xy(t) u) - eps <= n.(s_xy(t) - c) - (r + margin).  Their u-coefficients
// are taken from step t's slab as it passes through LDS and kept packed: the rows of step t are zero from column 2t on, so row 2(t-1) + j
// holds 2t doubles at A[2 t (t-1) + 2 t j], 2T(T+1) in all.  The disc load, the choice of the two discs, the half-plane and its `planes`
// record are qp_avoid.h's, shared with k_kmpc_qp.hip.
//
// WALL (f1p_stmpc_qp_walls_*): the AV variant whose two rows per step are the two nearest of {the two nearest live discs, the
// wall to the left of pbar_t, the wall to its right} on the active occupancy bitmap, left and right of the direction of travel
// psibar_t + betabar_t (L.pw).  Lane t - 1 marches both sides of step t itself (qp_walls.h) and takes the first and the second of the four
// candidates; lanes >= T march nothing.  From the half-plane on everything is the AV variant's.  M = 0 (no discs) is allowed here.
#include "qp_walls.h"

namespace f1p {

namespace {

// Jacobian entries per step (get_dynamic_model_matrix :428-535); the unit diagonal of rows 0-4, A[4, 5] = B[2, 0] = B[3, 1] = DT are implicit
enum { J03, J04, J06, J13, J14, J16, J52, J53, J55, J56, J62, J63, J65, J66, JB51, JB61, JC0, JC1, JC5, JC6, NJ };

// One ego's LDS, carved from b in doubles: the kernel's pointers (P = double*), or with P = int from 0 the members' offsets, `end` the
// size.  extra: the QP's inputs beyond u (nq = n + extra; AV: the slack and its padding).
template <class P>
struct StQpLdsT {
    P H{}, M{}, x0{}, ref{}, fr{}, J{}, SL{}, U{}, W{}, Y{}, Wd{}, Wv{}, Wr{}, Sd{}, Sv{}, pa{}, pd{}, pv{}, end{};
    __host__ __device__ constexpr StQpLdsT(P b, int T, int extra = 0) {
        const int n = 2 * T, Tp = T + 1, nq = n + extra;
        H = b; b += nq * nq;
        M = b; b += nq * nq;
        x0 = b; b += 8;
        ref = b; b += 7 * Tp;
        fr = b; b += 7 * Tp;
        J = b; b += NJ * T;                 // J[k * T + t]
        SL = b; b += 7 * n;                 // the slab of step t: SL[k * n + i] = d x_t[k] / d u_i
        U = b; b += nq; W = b; b += nq; Y = b; b += nq;
        Wd = b; b += T; Wv = b; b += T; Wr = b; b += T; Sd = b; b += T; Sv = b; b += T;
        pa = b; b += T; pd = b; b += T; pv = b; b += T;
        end = b;
    }
};
// the avoidance variant's: nq = n + 2 inputs, and behind the common members the packed rows A, their published w / D WA [n + 1], pbar_1..T
// (x, y, yaw + beta), the discs [16][5]
template <class P>
struct StQpLdsAvT : StQpLdsT<P> {
    P A{}, WA{}, px{}, py{}, pw{}, ob{};
    __host__ __device__ constexpr StQpLdsAvT(P b, int T) : StQpLdsT<P>(b, T, 2) {
        const int n = 2 * T, Tp = T + 1;
        b = this->end;
        A = b; b += n * Tp;                 // rows 2 q, 2 q + 1 (step q + 1): 2 (q + 1) doubles each from A[2 q (q + 1)]
        WA = b; b += n + 1;
        px = b; b += T; py = b; b += T; pw = b; b += T;
        ob = b; b += 5 * F1P_KMPC_MAX_OBS;
        this->end = b;
    }
};
template <bool AV> using StQpLds = std::conditional_t<AV, StQpLdsAvT<double*>, StQpLdsT<double*>>;
// doubles of LDS per ego
__host__ __device__ constexpr int stqp_lds_doubles(int T, bool av) { return av ? StQpLdsAvT<int>(0, T).end : StQpLdsT<int>(0, T).end; }
// the default horizon must run; F1P_STMPC_QP_AVOID_MAX_T is the longest horizon whose layout one workgroup may claim (160 KiB) with
// room left for the 1 KiB the plain kernel's cap leaves too
static_assert(8 * stqp_lds_doubles(F1P_STMPC_QP_AVOID_MAX_T, true) <= 160 * 1024 - 1024, "F1P_STMPC_QP_AVOID_MAX_T does not fit the CU's LDS");
static_assert(8 * stqp_lds_doubles(F1P_STMPC_QP_AVOID_MAX_T + 1, true) > 160 * 1024 - 1024, "F1P_STMPC_QP_AVOID_MAX_T is not the cap");

// y = A_t x (the structure of :478-511)
__device__ __forceinline__ void amul(const double* J, int T, int t, double DT, const double x[7], double y[7]) {
    const double* j = J + t;
    y[0] = x[0] + j[J03 * T] * x[3] + j[J04 * T] * x[4] + j[J06 * T] * x[6];
    y[1] = x[1] + j[J13 * T] * x[3] + j[J14 * T] * x[4] + j[J16 * T] * x[6];
    y[2] = x[2];
    y[3] = x[3];
    y[4] = x[4] + DT * x[5];
    y[5] = j[J52 * T] * x[2] + j[J53 * T] * x[3] + j[J55 * T] * x[5] + j[J56 * T] * x[6];
    y[6] = j[J62 * T] * x[2] + j[J63 * T] * x[3] + j[J65 * T] * x[5] + j[J66 * T] * x[6];
}

}  // namespace

// AvArgs: none (the plain QP), one QpAvoidArgs (AV; f1p_internal.h), or a QpAvoidArgs and a QpWallArgs (WALL)
template <class... AvArgs>
__global__ __launch_bounds__(64) void k_stmpc_qp(const double* __restrict__ x0g, const double* __restrict__ refg, const double* pa_g,
                                                 const double* pd_g, int pstride, int E, f1p_stmpc_cfg cfg, int max_iter, double tol,
                                                 double* __restrict__ steer, double* __restrict__ speed, int32_t* __restrict__ status,
                                                 double* __restrict__ u_out, double* __restrict__ x_out, double* __restrict__ obj_out,
                                                 double* __restrict__ duals, int32_t* __restrict__ iters_out, double* warm_out,
                                                 AvArgs... av_args) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr bool AV = sizeof...(AvArgs) >= 1;
    constexpr bool WALL = sizeof...(AvArgs) == 2;
    [[maybe_unused]] const QpAvoidArgs av = qp_avoid_args(av_args...);
    constexpr int R = AV ? 12 : 10;                      // inequality rows per lane
    // AV: the solver's slack is e' = eps / sig, sig = 1 / sqrt(2 rho): its curvature is 1 like the inputs' (2 rho = 2e4 beside weights of
    // 0.01 leaves the dual residual a floor at the stopping rule's 1e-10).  The rows, hence the multipliers, are the unscaled problem's.
    [[maybe_unused]] const double sig = AV ? 1.0 / sqrt(2.0 * av.rho) : 1.0;
    const int T = cfg.horizon, n = 2 * T, Tp = T + 1;
    const int nq = AV ? n + 2 : n;                       // the QP's inputs: u, and (eps, padding) with AV
    const int tau = threadIdx.x, i0 = 2 * tau, i1 = 2 * tau + 1;
    const int e = blockIdx.x;
    if (e >= E) return;                                  // (one ego per workgroup: uniform)
    StQpLds<AV> L(reinterpret_cast<double*>(lds_raw), T);
    const bool in_n = tau < T;
    const double DT = cfg.dt;
    const double NaN = __builtin_nan("");

    // ---- inputs -> LDS; finiteness ----------------------------------------------------------------------------------------------------
    bool bad = false;
    for (int k = tau; k < 7; k += 64) { const double v = x0g[(size_t)e * 7 + k]; L.x0[k] = v; bad |= !isfinite(v); }
    for (int k = tau; k < 7 * Tp; k += 64) { const double v = refg[(size_t)e * 7 * Tp + k]; L.ref[k] = v; bad |= !isfinite(v); }
    for (int k = tau; k < T; k += 64) {
        const double a = pa_g ? pa_g[((size_t)e * T + k) * pstride] : 0.0;
        const double d = pd_g ? pd_g[((size_t)e * T + k) * pstride] : 0.0;
        L.pa[k] = a; L.pd[k] = d; bad |= !(isfinite(a) && isfinite(d));
    }
    if constexpr (AV) bad |= qp_avoid_load<64>(av, e, tau, L.ob);
    bad = gmax<64>(bad ? 1.0 : 0.0) > 0.0;
    __syncthreads();
    const double d0 = L.x0[2], v0 = L.x0[3];
    int st = bad ? 3 : (fabs(d0) <= cfg.max_steer && v0 >= cfg.min_speed && v0 <= cfg.max_speed) ? 0 : 1;   // 1: a t = 0 row cannot hold
    bool done = st != 0;

    // ---- 1. linearisation point (predict_motion :279-300), Jacobians, free response -----------------------------------------------------
    const DynConst kc = dyn_const(cfg);
    if (tau == 0 && !done) {
        DynState s;
        s.x = L.x0[0]; s.y = L.x0[1]; s.delta = L.x0[2]; s.v = L.x0[3]; s.yaw = L.x0[4]; s.yr = L.x0[5]; s.beta = L.x0[6];
        for (int t = 0; t < T; ++t) {                    // path_predict[2..6, t] -> pd / pv and J scratch (rows JC*, overwritten below)
            L.J[JC0 * T + t] = s.delta; L.J[JC1 * T + t] = s.v; L.J[JC5 * T + t] = s.yaw; L.J[JC6 * T + t] = s.yr; L.pv[t] = s.beta;
            dyn_step<false>(s, L.pa[t], L.pd[t], cfg, kc);
            if constexpr (AV) { L.px[t] = s.x; L.py[t] = s.y; L.pw[t] = s.yaw + s.beta; }      // pbar_{t+1} and its direction of travel
        }
    }
    __syncthreads();
    bool nf = false;
    double j[NJ];
    if (in_n && !done) {                                 // get_dynamic_model_matrix(delta, v, yaw, yawrate, beta, oa[t]) :428-535
        const double delta = L.J[JC0 * T + tau], v = L.J[JC1 * T + tau], yaw = L.J[JC5 * T + tau], yr = L.J[JC6 * T + tau];
        const double beta = L.pv[tau], a = L.pa[tau];
        const double Tl = kc.gl_r - (a * kc.h);          // :451-464
        const double V = kc.gl_f + (a * kc.h);
        const double A1 = kc.K * kc.F * Tl;
        const double A2 = kc.K * (kc.R * V - kc.F * Tl);
        const double A3 = kc.K * (kc.lf2cf * Tl + kc.lr2cr * V);
        const double A4 = kc.M * Tl;
        const double A5 = kc.N * V + kc.M * Tl;
        const double A6 = kc.N * V * kc.l_r - kc.M * Tl * kc.l_f;
        const double B1 = (-kc.h * kc.F * kc.K) * delta + (kc.h * kc.K * (kc.F + kc.R)) * beta -
                          (kc.h * kc.K * (kc.lr2cr - kc.lf2cf)) * (yr / v);                              // :466-470
        const double B2 = (-kc.h * kc.M) * (delta / v) - kc.h * (kc.N - kc.M) * (beta / v) +
                          kc.h * (kc.l_f * kc.M + kc.l_r * kc.N) * (yr / (v * v));                       // :471-475
        double sn, cs;
        sincos(yaw + beta, &sn, &cs);
        j[J55] = -DT * (A3 / v) + 1;                     // :486-487
        j[J66] = -DT * A5 + 1;
        j[J03] = DT * cs;                                // :489-496
        j[J04] = -DT * v * sn;
        j[J06] = -DT * v * sn;
        j[J13] = DT * sn;
        j[J14] = DT * v * cs;
        j[J16] = DT * v * cs;
        j[J52] = DT * A1;                                // :500-503
        j[J53] = DT * A3 * (yr / (v * v));
        j[J56] = DT * A2;
        j[J62] = DT * (A4 / v);                          // :504-511
        j[J63] = DT * (-A4 * beta * v + A5 * beta * v - A6 * 2 * yr) / (v * v * v);
        j[J65] = DT * ((A6 / (v * v)) - 1);
        j[JB51] = DT * B1;                               // :518-519
        j[JB61] = DT * B2;
        j[JC0] = DT * (v * sn * yaw + v * sn * beta);    // :522-533
        j[JC1] = DT * (-v * cs * yaw - v * cs * beta);
        j[JC5] = DT * (-A3 * (yr / v) - B1 * a);
        j[JC6] = DT * (((A4 * delta * v - A5 * beta * v + A6 * 2 * yr) / (v * v)) - B2 * a);
    }
    __syncthreads();                                     // every lane has read its scratch before the rows are written
    if (in_n && !done) {
#pragma unroll
        for (int k = 0; k < NJ; ++k) { L.J[k * T + tau] = j[k]; nf |= !isfinite(j[k]); }
    }
    __syncthreads();
    if (tau == 0 && !done) {                             // free response: fr_{t+1} = A_t fr_t + C_t
        double x[7], y[7];
        for (int k = 0; k < 7; ++k) { x[k] = L.x0[k]; L.fr[k * Tp] = x[k]; }
        for (int t = 0; t < T; ++t) {
            amul(L.J, T, t, DT, x, y);
            y[0] += L.J[JC0 * T + t]; y[1] += L.J[JC1 * T + t]; y[5] += L.J[JC5 * T + t]; y[6] += L.J[JC6 * T + t];
            for (int k = 0; k < 7; ++k) { x[k] = y[k]; L.fr[k * Tp + t + 1] = x[k]; nf |= !isfinite(x[k]); }
        }
    }
    nf = gmax<64>(nf ? 1.0 : 0.0) > 0.0;
    if (!done && nf) { st = 3; done = true; }            // non-finite model data (a predicted speed of 0)
    __syncthreads();

    // AV: this lane's two half-planes (step tau + 1: the nearest and the second nearest live disc)
    [[maybe_unused]] QpPlane pl[2];
    [[maybe_unused]] const int a_off = 2 * tau * (tau + 1), a_len = 2 * (tau + 1);     // this lane's packed rows: A[a_off + j a_len + c]
    if constexpr (WALL) {
        // both sides of step tau + 1 marched from pbar along +-l, l = (-sin w, cos w), w the direction of travel; then the first and the
        // second of the four candidates.  The two marches are independent: their word loads may be in flight together.
        if (in_n && !done) {
            const QpWallArgs wl = qp_wall_args(av_args...);
            const int t = tau + 1;
            const double tt = (double)t * DT, px = L.px[tau], py = L.py[tau];
            double sn, cs;
            sincos(L.pw[tau], &sn, &cs);
            const double llx = -sn, lly = cs;                             // the LEFT direction (the right one is its negative)
            const int kl = qp_wall_march(wl, px, py, llx, lly), kr = qp_wall_march(wl, px, py, -llx, -lly);
            const QpNearest nr = qp_avoid_nearest(L.ob, av.M, px, py, tt);
            const QpCand d0 = qp_disc_cand(L.ob, nr.m0, px, py, tt), d1 = qp_disc_cand(L.ob, nr.m1, px, py, tt);
            const QpWallCand wL = qp_wall_cand(wl, px, py, llx, lly, kl, F1P_QP_WALL_SLOT_L);
            const QpWallCand wR = qp_wall_cand(wl, px, py, -llx, -lly, kr, F1P_QP_WALL_SLOT_R);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int pick = qp_select4(d0, d1, wL, wR, jj);
                if (pick == 0 || pick == 1) pl[jj] = qp_avoid_plane(L.ob, pick == 0 ? nr.m0 : nr.m1, px, py, L.pw[tau], tt, L.fr[t], L.fr[Tp + t], av.margin);
                else if (pick == 2) pl[jj] = qp_wall_plane(wL, llx, lly, L.fr[t], L.fr[Tp + t], wl.margin);
                else if (pick == 3) pl[jj] = qp_wall_plane(wR, -llx, -lly, L.fr[t], L.fr[Tp + t], wl.margin);
            }
        }
    } else if constexpr (AV) {
        if (in_n && !done) {
            const int t = tau + 1;
            const double tt = (double)t * DT, px = L.px[tau], py = L.py[tau];
            const QpNearest nr = qp_avoid_nearest(L.ob, av.M, px, py, tt);
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int ms = jj == 0 ? nr.m0 : nr.m1;
                if (ms >= 0) pl[jj] = qp_avoid_plane(L.ob, ms, px, py, L.pw[tau], tt, L.fr[t], L.fr[Tp + t], av.margin);
            }
        }
    }

    // ---- 2. condensing: H and g, one slab per step -----------------------------------------------------------------------------------
    double g0 = 0.0, g1 = 0.0;
    if (!done) {
        if (in_n) for (int c = 0; c < nq; ++c) { L.H[i0 * nq + c] = 0.0; L.H[i1 * nq + c] = 0.0; }
        if constexpr (AV) {
            if (tau == T) {                              // eps and the padding input
                for (int c = 0; c < nq; ++c) { L.H[i0 * nq + c] = 0.0; L.H[i1 * nq + c] = 0.0; }
                L.H[i0 * nq + i0] = 1.0; L.H[i1 * nq + i1] = 1.0;         // 2 rho sig^2
                g0 = av.lin * sig;
            }
        }
        double dv[7] = {0, 0, 0, 0, 0, 0, 0}, ev[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int t = 1; t < Tp; ++t) {
            if (in_n) {
                if (t == tau + 1) {                      // B_tau e_j
                    dv[2] = DT;
                    ev[3] = DT; ev[5] = L.J[JB51 * T + tau]; ev[6] = L.J[JB61 * T + tau];
                } else if (t > tau + 1) {                // A_{t-1} d
                    double y[7];
                    amul(L.J, T, t - 1, DT, dv, y);
                    for (int k = 0; k < 7; ++k) dv[k] = y[k];
                    amul(L.J, T, t - 1, DT, ev, y);
                    for (int k = 0; k < 7; ++k) ev[k] = y[k];
                }
                for (int k = 0; k < 7; ++k) { L.SL[k * n + i0] = dv[k]; L.SL[k * n + i1] = ev[k]; }
            }
            const double* w = t == T ? cfg.qf : cfg.q;
            __syncthreads();
            if (in_n && t > tau) {
                for (int k = 0; k < 7; ++k) {
                    const double r = L.fr[k * Tp + t] - L.ref[k * Tp + t];
                    g0 += 2.0 * w[k] * dv[k] * r;
                    g1 += 2.0 * w[k] * ev[k] * r;
                }
                for (int c = 0; c < 2 * t; ++c) {        // columns of steps < t (the others are zero at t)
                    double h0 = 0.0, h1 = 0.0;
                    for (int k = 0; k < 7; ++k) {
                        const double s = 2.0 * w[k] * L.SL[k * n + c];
                        h0 += s * dv[k];
                        h1 += s * ev[k];
                    }
                    L.H[i0 * nq + c] += h0;
                    L.H[i1 * nq + c] += h1;
                }
                if constexpr (AV) {
                    if (t == tau + 1) {                  // this lane's rows, from the slab of its step (c < 2 t = a_len)
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj)
                            for (int c = 0; c < a_len; ++c)
                                L.A[a_off + jj * a_len + c] = pl[jj].slot >= 0 ? -(pl[jj].nx * L.SL[c] + pl[jj].ny * L.SL[n + c]) : 0.0;
                    }
                }
            }
            __syncthreads();
        }
        if (in_n) {                                      // R and Rd (:616, :622)
            const int nb = (tau > 0) + (tau < T - 1);
            L.H[i0 * nq + i0] += 2.0 * (cfg.r[0] + nb * cfg.rd[0]);
            L.H[i1 * nq + i1] += 2.0 * (cfg.r[1] + nb * cfg.rd[1]);
            if (tau > 0) { L.H[i0 * nq + i0 - 2] -= 2.0 * cfg.rd[0]; L.H[i1 * nq + i1 - 2] -= 2.0 * cfg.rd[1]; }
            if (tau < T - 1) { L.H[i0 * nq + i0 + 2] -= 2.0 * cfg.rd[0]; L.H[i1 * nq + i1 + 2] -= 2.0 * cfg.rd[1]; }
        }
    }
    __syncthreads();

    // ---- 3. interior point (qp_ipm.h) ----------------------------------------------------------------------------------------------------
    const double MSV = cfg.max_steer_v;
    double h[R];
    bool valid[R];
    h[0] = MSV; h[1] = MSV; h[2] = cfg.max_accel; h[3] = cfg.max_accel;
    h[4] = cfg.max_steer - d0; h[5] = cfg.max_steer + d0; h[6] = cfg.max_speed - v0; h[7] = v0 - cfg.min_speed; h[8] = MSV; h[9] = MSV;
#pragma unroll
    for (int r = 0; r < 10; ++r) valid[r] = in_n && (r < 8 || tau < T - 1);
    double m_rows = 10.0 * T - 2.0;
    if constexpr (AV) {                                  // rows 10, 11: the half-planes; lane T: -eps <= 0
        h[10] = pl[0].h; h[11] = pl[1].h;
        valid[10] = in_n ? pl[0].slot >= 0 : tau == T;
        valid[11] = in_n && pl[1].slot >= 0;
        m_rows += 1.0 + gsum<64>((double)((in_n && pl[0].slot >= 0) + (in_n && pl[1].slot >= 0)));
    }

    // G x for this lane's rows (x published in vec[])
    auto gmul = [&](const double* vec, const double (&x)[2], double (&out)[R]) {
        double p0 = 0.0, p1 = 0.0;
        if (in_n) for (int q = 0; q <= tau; ++q) { p0 += vec[2 * q]; p1 += vec[2 * q + 1]; }
        const double r = in_n && tau < T - 1 ? vec[i0 + 2] - x[0] : 0.0;
        out[0] = x[0]; out[1] = -x[0]; out[2] = x[1]; out[3] = -x[1];
        out[4] = DT * p0; out[5] = -(DT * p0); out[6] = DT * p1; out[7] = -(DT * p1); out[8] = r; out[9] = -r;
#pragma unroll
        for (int k = 0; k < 10; ++k) out[k] = valid[k] ? out[k] : 0.0;
        if constexpr (AV) {                              // A_r . u - eps; lane T: -eps
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                double o = 0.0;
                if (valid[10 + jj]) {
                    if (in_n) for (int c = 0; c < a_len; ++c) o += L.A[a_off + jj * a_len + c] * vec[c];
                    o -= sig * vec[n];
                }
                out[10 + jj] = o;
            }
        }
    };
    // AV: (sum_r w_r A_r) at columns i0 and i1 over the rows of steps > tau, w published in WA[]
    [[maybe_unused]] auto a_cols = [&](double& o0, double& o1) {
        o0 = o1 = 0.0;
        if constexpr (AV) {
            for (int q = tau; q < T; ++q) {
                const int len = 2 * (q + 1);
                const double* a = L.A + 2 * q * (q + 1);
                const double w0 = L.WA[2 * q], w1 = L.WA[2 * q + 1];
                o0 += w0 * a[i0] + w1 * a[len + i0];
                o1 += w0 * a[i1] + w1 * a[len + i1];
            }
        }
    };
    // (G' w) at u0_tau, u1_tau: the rows' differences published in Wd[], Wv[], Wr[]
    auto gtmul = [&](const double (&w)[R], double (&o)[2]) {
        const double wd = valid[4] ? w[4] - w[5] : 0.0, wv = valid[6] ? w[6] - w[7] : 0.0, wr = valid[8] ? w[8] - w[9] : 0.0;
        __syncthreads();
        if (in_n) { L.Wd[tau] = wd; L.Wv[tau] = wv; L.Wr[tau] = wr; }
        if constexpr (AV) {
            if (in_n) { L.WA[i0] = valid[10] ? w[10] : 0.0; L.WA[i1] = valid[11] ? w[11] : 0.0; }
            else if (tau == T) L.WA[n] = w[10];
        }
        __syncthreads();
        o[0] = o[1] = 0.0;
        if (in_n) {
            double sd = 0.0, sv = 0.0;
            for (int q = T - 1; q >= tau; --q) { sd += L.Wd[q]; sv += L.Wv[q]; }
            o[0] = (valid[0] ? w[0] - w[1] : 0.0) + DT * sd - wr + (tau > 0 ? L.Wr[tau - 1] : 0.0);
            o[1] = (valid[2] ? w[2] - w[3] : 0.0) + DT * sv;
        }
        if constexpr (AV) {
            if (in_n) {
                double a0, a1;
                a_cols(a0, a1);
                o[0] += a0; o[1] += a1;
            } else if (tau == T) {                       // eps: minus every row's w
                double a = 0.0;
                for (int r = 0; r <= n; ++r) a += L.WA[r];
                o[0] = -(sig * a);
            }
        }
    };
    // rows i0 and i1 of M = H + G' diag(D) G, lower triangle
    // AV: + sum_r D_r A_r A_r' on the u block; the scaled slack's row: -sig sum_r D_r A_r (each lane its own two columns),
    // 1 + sig^2 (sum_r D_r + D_eps) on the diagonal; the padding input's row: its unit diagonal
    auto newton_rows = [&](const double (&D)[R]) {
        __syncthreads();
        if (in_n) { L.Wd[tau] = D[4] + D[5]; L.Wv[tau] = D[6] + D[7]; L.Wr[tau] = D[8] + D[9]; }
        if constexpr (AV) {
            if (in_n) { L.WA[i0] = D[10]; L.WA[i1] = D[11]; }
            else if (tau == T) L.WA[n] = D[10];
        }
        __syncthreads();
        if (in_n) {
            double sd = 0.0, sv = 0.0;
            for (int q = T - 1; q >= tau; --q) { sd += L.Wd[q]; sv += L.Wv[q]; }
            L.Sd[tau] = sd; L.Sv[tau] = sv;
        }
        __syncthreads();
        if (in_n) {
            const double wr = L.Wr[tau], wrm = tau > 0 ? L.Wr[tau - 1] : 0.0;
            for (int c = 0; c <= i1; ++c) {
                const int q = c >> 1, m_ = max(tau, q);
                double m0 = L.H[i0 * nq + c], m1 = L.H[i1 * nq + c];
                if ((c & 1) == 0) m0 += DT * DT * L.Sd[m_];
                else m1 += DT * DT * L.Sv[m_];
                if (c == i0) m0 += D[0] + D[1] + wr + wrm;
                if (c == i0 - 2) m0 -= wrm;
                if (c == i1) m1 += D[2] + D[3];
                if constexpr (AV) {
                    for (int q = tau; q < T; ++q) {
                        const int len = 2 * (q + 1);
                        const double* a = L.A + 2 * q * (q + 1);
                        const double w0 = L.WA[2 * q] * a[c], w1 = L.WA[2 * q + 1] * a[len + c];
                        m0 += w0 * a[i0] + w1 * a[len + i0];
                        m1 += w0 * a[i1] + w1 * a[len + i1];
                    }
                }
                if (c <= i0) L.M[i0 * nq + c] = m0;
                L.M[i1 * nq + c] = m1;
            }
        }
        if constexpr (AV) {
            if (in_n) {
                double a0, a1;
                a_cols(a0, a1);
                L.M[n * nq + i0] = -(sig * a0); L.M[n * nq + i1] = -(sig * a1);
            } else if (tau == T) {
                double sd = 0.0;
                for (int r = 0; r <= n; ++r) sd += L.WA[r];
                L.M[n * nq + n] = 1.0 + sig * sig * sd;
                for (int c = 0; c <= n; ++c) L.M[(n + 1) * nq + c] = 0.0;
                L.M[(n + 1) * nq + n + 1] = 1.0;
            }
        }
    };

    const double gv[2] = {g0, g1};
    double u[2], lam[R];
    int it_done;
    qp_ipm<64, 2, R>(QpIpmLds{L.H, L.M, L.U, L.Y}, nq, tau, gv, h, valid, m_rows, max_iter, tol, done, st, it_done, u, lam, gmul,
                     gtmul, newton_rows);

    // ---- outputs --------------------------------------------------------------------------------------------------------------------
    const bool ok = st == 0 || st == 2;
    if (in_n) {
        if (u_out) { u_out[(size_t)e * n + i0] = ok ? u[0] : NaN; u_out[(size_t)e * n + i1] = ok ? u[1] : NaN; }
        // the reference's (self.oa, self.odelta_v) = (u[1, :], u[0, :]) (:1089-1103); a failed solve leaves None: zeros next call
        if (warm_out) { warm_out[(size_t)e * n + i0] = ok ? u[1] : 0.0; warm_out[(size_t)e * n + i1] = ok ? u[0] : 0.0; }
        if (duals) {
            // rate upper, rate lower (T-1 each), delta_1..T upper, lower, v_1..T upper, lower, steer_v upper, lower, accel upper, lower (T each)
            double* du_ = duals + (size_t)e * (10 * T - 2);
            const int R2 = 2 * T - 2;
            if (tau < T - 1) { du_[tau] = ok ? lam[8] : NaN; du_[T - 1 + tau] = ok ? lam[9] : NaN; }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int blk = r < 4 ? 4 + r : r - 4;   // rows 4..7 (delta, v) come before rows 0..3 (the boxes)
                du_[R2 + blk * T + tau] = ok ? lam[r] : NaN;
            }
        }
        if constexpr (AV) {
            if (av.planes) {
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) qp_avoid_write_plane(av.planes + ((size_t)e * n + i0 + jj) * 4, pl[jj], ok);
            }
            if (av.duals) { av.duals[(size_t)e * (n + 1) + i0] = ok ? lam[10] : NaN; av.duals[(size_t)e * (n + 1) + i1] = ok ? lam[11] : NaN; }
        }
    }
    if constexpr (AV) {
        if (tau == T) {
            if (av.duals) av.duals[(size_t)e * (n + 1) + n] = ok ? lam[10] : NaN;
            if (av.eps) av.eps[e] = ok ? sig * u[0] : NaN;
        }
    }
    if (tau == 0) {
        if (status) status[e] = st;
        if (iters_out) iters_out[e] = ok ? it_done : 0;
        steer[e] = ok ? d0 + L.U[0] * DT : NaN;                          // :1112-1114
        speed[e] = ok ? v0 + L.U[1] * DT : NaN;                          // :1116-1117
        if (x_out || obj_out) {
            // x_{t+1} = A_t x_t + B_t u_t + C_t and the objective cvxpy reports (:616-622), the constant t = 0 term included
            double x[7], y[7], f = 0.0;
            for (int k = 0; k < 7; ++k) x[k] = L.x0[k];
            double* xo = x_out ? x_out + (size_t)e * 7 * Tp : nullptr;
            for (int t = 0; t < Tp; ++t) {
                const double* q = t == T ? cfg.qf : cfg.q;
                for (int k = 0; k < 7; ++k) {
                    if (xo) xo[k * Tp + t] = ok ? x[k] : NaN;
                    const double ek = x[k] - L.ref[k * Tp + t];
                    f += q[k] * ek * ek;
                }
                if (t == T) break;
                const double a0 = L.U[2 * t], a1 = L.U[2 * t + 1];
                f += cfg.r[0] * a0 * a0 + cfg.r[1] * a1 * a1;
                if (t < T - 1) {
                    const double da0 = L.U[2 * t + 2] - a0, da1 = L.U[2 * t + 3] - a1;
                    f += cfg.rd[0] * da0 * da0 + cfg.rd[1] * da1 * da1;
                }
                amul(L.J, T, t, DT, x, y);
                y[0] += L.J[JC0 * T + t]; y[1] += L.J[JC1 * T + t];
                y[2] += DT * a0; y[3] += DT * a1;
                y[5] += L.J[JB51 * T + t] * a1 + L.J[JC5 * T + t];
                y[6] += L.J[JB61 * T + t] * a1 + L.J[JC6 * T + t];
                for (int k = 0; k < 7; ++k) x[k] = y[k];
            }
            if constexpr (AV) { const double eps = sig * L.U[n]; f += av.rho * eps * eps + av.lin * eps; }
            if (obj_out) obj_out[e] = ok ? f : NaN;
        }
    }
}

// gather an ego subset's warm start [idx[k]][t][2] (W steps per ego) into [k][t][2] (Tb steps), zeros where use[k] == 0
__global__ __launch_bounds__(256) void k_stmpc_qp_warm_in(const double* __restrict__ warm, const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ use, int nb, int Tb, int W, double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb * Tb * 2) return;
    const int k = j / (Tb * 2), r = j % (Tb * 2);
    out[j] = use[k] ? warm[(size_t)idx[k] * W * 2 + r] : 0.0;
}

// scatter [k][t][2] (Tb steps) back to [idx[k]][t][2] (W steps per ego)
__global__ __launch_bounds__(256) void k_stmpc_qp_warm_out(const double* __restrict__ in, const int32_t* __restrict__ idx, int nb, int Tb,
                                                           int W, double* __restrict__ warm) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb * Tb * 2) return;
    const int k = j / (Tb * 2), r = j % (Tb * 2);
    warm[(size_t)idx[k] * W * 2 + r] = in[j];
}

// rows x, y, v, yaw of a 7-row reference [k][7][Tp] (k_stmpc_ref) -> [k][4][Tp], the kinematic branch's (:236-276)
__global__ __launch_bounds__(256) void k_stmpc_qp_kref(const double* __restrict__ ref7, int nb, int Tp, double* __restrict__ ref4) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb * 4 * Tp) return;
    const int k = j / (4 * Tp), r = (j / Tp) % 4, t = j % Tp;
    const int row = r < 2 ? r : r + 1;
    ref4[j] = ref7[((size_t)k * 7 + row) * Tp + t];
}

// gather an ego subset's discs [idx[k]][M][5] into [k][M][5]
__global__ __launch_bounds__(256) void k_stmpc_qp_obs_in(const double* __restrict__ obs, const int32_t* __restrict__ idx, int nb, int M5,
                                                         double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb * M5) return;
    const int k = j / M5, r = j % M5;
    out[j] = obs[(size_t)idx[k] * M5 + r];
}

size_t stmpc_qp_avoid_lds_bytes(int T) { return sizeof(double) * (size_t)stqp_lds_doubles(T, true); }

// one wave per ego; in the avoidance variant lane T takes the slack; the wall variant as the avoidance variant
int launch_stmpc_qp(f1p_ctx* ctx, int E, const f1p_stmpc_cfg* cfg, int max_iter, double tol, const QpIo& io, const QpAvoidArgs* avoid,
                    const QpWallArgs* walls) {
    if (E <= 0) return F1P_OK;
    const int T = cfg->horizon;
    if (avoid && (T > F1P_STMPC_QP_AVOID_MAX_T || avoid->M < 0 || avoid->M > F1P_KMPC_MAX_OBS || (avoid->M > 0 && !avoid->obs)))
        return set_error(ctx, F1P_EINVAL, "stmpc qp avoid: bad horizon / obstacles");
    if (walls && (!avoid || !walls->g.bits || walls->g.w < 1 || walls->g.h < 1 || walls->n_samples < 1 || walls->n_samples > F1P_KMPC_QP_WALL_MAX_SAMPLES))
        return set_error(ctx, F1P_EINVAL, "stmpc qp walls: bad grid / n_samples");
    const size_t lds = sizeof(double) * (size_t)stqp_lds_doubles(T, avoid != nullptr);
    const auto launch = [&](auto kern, const char* too_long, const char* what, auto... av) {
        const int rc = qp_lds_opt_in(ctx, reinterpret_cast<const void*>(kern), lds, too_long);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)E), dim3(64), lds, ctx->stream, io.x0, io.ref, io.pa, io.pd, io.pstride, E, *cfg, max_iter, tol,
                           io.steer, io.speed, io.status, io.u, io.x, io.obj, io.duals, io.iters, io.warm_out, av...);
        return check_hip(ctx, hipGetLastError(), what);
    };
    if (walls)
        return launch(&k_stmpc_qp<QpAvoidArgs, QpWallArgs>, "stmpc qp walls: horizon too long for the CU's LDS", "k_stmpc_qp_walls launch", *avoid, *walls);
    if (avoid) return launch(&k_stmpc_qp<QpAvoidArgs>, "stmpc qp avoid: horizon too long for the CU's LDS", "k_stmpc_qp_avoid launch", *avoid);
    return launch(&k_stmpc_qp<>, "stmpc qp: horizon too long for the CU's LDS", "k_stmpc_qp launch");
}

int launch_stmpc_qp_obs_in(f1p_ctx* ctx, const double* d_obs, const int32_t* d_idx, int nb, int M, double* d_out) {
    if (nb <= 0 || M <= 0) return F1P_OK;
    const int n = nb * M * 5;
    hipLaunchKernelGGL(k_stmpc_qp_obs_in, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_obs, d_idx, nb, M * 5, d_out);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_qp_obs_in launch");
}

int launch_stmpc_qp_warm_in(f1p_ctx* ctx, const double* d_warm, const int32_t* d_idx, const int32_t* d_use, int nb, int Tb, int W, double* d_out) {
    if (nb <= 0) return F1P_OK;
    const int n = nb * Tb * 2;
    hipLaunchKernelGGL(k_stmpc_qp_warm_in, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_warm, d_idx, d_use, nb, Tb, W, d_out);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_qp_warm_in launch");
}

int launch_stmpc_qp_warm_out(f1p_ctx* ctx, const double* d_in, const int32_t* d_idx, int nb, int Tb, int W, double* d_warm) {
    if (nb <= 0) return F1P_OK;
    const int n = nb * Tb * 2;
    hipLaunchKernelGGL(k_stmpc_qp_warm_out, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_in, d_idx, nb, Tb, W, d_warm);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_qp_warm_out launch");
}

int launch_stmpc_qp_kref(f1p_ctx* ctx, const double* d_ref7, int nb, int T, double* d_ref4) {
    if (nb <= 0) return F1P_OK;
    const int n = nb * 4 * (T + 1);
    hipLaunchKernelGGL(k_stmpc_qp_kref, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_ref7, nb, T + 1, d_ref4);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_qp_kref launch");
}

}  // namespace f1p
