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
#include "qp_ipm.h"

namespace f1p {

namespace {

// Jacobian entries per step (get_dynamic_model_matrix :428-535); the unit diagonal of rows 0-4, A[4, 5] = B[2, 0] = B[3, 1] = DT are implicit
enum { J03, J04, J06, J13, J14, J16, J52, J53, J55, J56, J62, J63, J65, J66, JB51, JB61, JC0, JC1, JC5, JC6, NJ };

// doubles of LDS per ego
__host__ __device__ inline int stqp_lds_doubles(int T) {
    const int n = 2 * T, Tp = T + 1;
    return 2 * n * n + 8 + 14 * Tp + NJ * T + 7 * n + 3 * n + 8 * T;
}

struct StQpLds {
    double *H, *M, *x0, *ref, *fr, *J, *SL, *U, *W, *Y, *Wd, *Wv, *Wr, *Sd, *Sv, *pa, *pd, *pv;
    __device__ StQpLds(double* b, int T) {
        const int n = 2 * T, Tp = T + 1;
        H = b; b += n * n;
        M = b; b += n * n;
        x0 = b; b += 8;
        ref = b; b += 7 * Tp;
        fr = b; b += 7 * Tp;
        J = b; b += NJ * T;                 // J[k * T + t]
        SL = b; b += 7 * n;                 // the slab of step t: SL[k * n + i] = d x_t[k] / d u_i
        U = b; b += n; W = b; b += n; Y = b; b += n;
        Wd = b; b += T; Wv = b; b += T; Wr = b; b += T; Sd = b; b += T; Sv = b; b += T;
        pa = b; b += T; pd = b; b += T; pv = b; b += T;
    }
};

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

__global__ __launch_bounds__(64) void k_stmpc_qp(const double* __restrict__ x0g, const double* __restrict__ refg, const double* pa_g,
                                                 const double* pd_g, int pstride, int E, f1p_stmpc_cfg cfg, int max_iter, double tol,
                                                 double* __restrict__ steer, double* __restrict__ speed, int32_t* __restrict__ status,
                                                 double* __restrict__ u_out, double* __restrict__ x_out, double* __restrict__ obj_out,
                                                 double* __restrict__ duals, int32_t* __restrict__ iters_out, double* warm_out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int T = cfg.horizon, n = 2 * T, Tp = T + 1;
    const int tau = threadIdx.x, i0 = 2 * tau, i1 = 2 * tau + 1;
    const int e = blockIdx.x;
    if (e >= E) return;                                  // (one ego per workgroup: uniform)
    StQpLds L(reinterpret_cast<double*>(lds_raw), T);
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

    // ---- 2. condensing: H and g, one slab per step -----------------------------------------------------------------------------------
    double g0 = 0.0, g1 = 0.0;
    if (!done) {
        if (in_n) for (int c = 0; c < n; ++c) { L.H[i0 * n + c] = 0.0; L.H[i1 * n + c] = 0.0; }
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
                    L.H[i0 * n + c] += h0;
                    L.H[i1 * n + c] += h1;
                }
            }
            __syncthreads();
        }
        if (in_n) {                                      // R and Rd (:616, :622)
            const int nb = (tau > 0) + (tau < T - 1);
            L.H[i0 * n + i0] += 2.0 * (cfg.r[0] + nb * cfg.rd[0]);
            L.H[i1 * n + i1] += 2.0 * (cfg.r[1] + nb * cfg.rd[1]);
            if (tau > 0) { L.H[i0 * n + i0 - 2] -= 2.0 * cfg.rd[0]; L.H[i1 * n + i1 - 2] -= 2.0 * cfg.rd[1]; }
            if (tau < T - 1) { L.H[i0 * n + i0 + 2] -= 2.0 * cfg.rd[0]; L.H[i1 * n + i1 + 2] -= 2.0 * cfg.rd[1]; }
        }
    }
    __syncthreads();

    // ---- 3. interior point (qp_ipm.h) ----------------------------------------------------------------------------------------------------
    const double MSV = cfg.max_steer_v;
    double h[10];
    bool valid[10];
    h[0] = MSV; h[1] = MSV; h[2] = cfg.max_accel; h[3] = cfg.max_accel;
    h[4] = cfg.max_steer - d0; h[5] = cfg.max_steer + d0; h[6] = cfg.max_speed - v0; h[7] = v0 - cfg.min_speed; h[8] = MSV; h[9] = MSV;
#pragma unroll
    for (int r = 0; r < 10; ++r) valid[r] = in_n && (r < 8 || tau < T - 1);

    // G x for this lane's rows (x published in vec[])
    auto gmul = [&](const double* vec, const double (&x)[2], double (&out)[10]) {
        double p0 = 0.0, p1 = 0.0;
        if (in_n) for (int q = 0; q <= tau; ++q) { p0 += vec[2 * q]; p1 += vec[2 * q + 1]; }
        const double r = in_n && tau < T - 1 ? vec[i0 + 2] - x[0] : 0.0;
        out[0] = x[0]; out[1] = -x[0]; out[2] = x[1]; out[3] = -x[1];
        out[4] = DT * p0; out[5] = -(DT * p0); out[6] = DT * p1; out[7] = -(DT * p1); out[8] = r; out[9] = -r;
#pragma unroll
        for (int k = 0; k < 10; ++k) out[k] = valid[k] ? out[k] : 0.0;
    };
    // (G' w) at u0_tau, u1_tau: the rows' differences published in Wd[], Wv[], Wr[]
    auto gtmul = [&](const double (&w)[10], double (&o)[2]) {
        const double wd = valid[4] ? w[4] - w[5] : 0.0, wv = valid[6] ? w[6] - w[7] : 0.0, wr = valid[8] ? w[8] - w[9] : 0.0;
        __syncthreads();
        if (in_n) { L.Wd[tau] = wd; L.Wv[tau] = wv; L.Wr[tau] = wr; }
        __syncthreads();
        o[0] = o[1] = 0.0;
        if (in_n) {
            double sd = 0.0, sv = 0.0;
            for (int q = T - 1; q >= tau; --q) { sd += L.Wd[q]; sv += L.Wv[q]; }
            o[0] = (valid[0] ? w[0] - w[1] : 0.0) + DT * sd - wr + (tau > 0 ? L.Wr[tau - 1] : 0.0);
            o[1] = (valid[2] ? w[2] - w[3] : 0.0) + DT * sv;
        }
    };
    // rows i0 and i1 of M = H + G' diag(D) G, lower triangle
    auto newton_rows = [&](const double (&D)[10]) {
        __syncthreads();
        if (in_n) { L.Wd[tau] = D[4] + D[5]; L.Wv[tau] = D[6] + D[7]; L.Wr[tau] = D[8] + D[9]; }
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
                double m0 = L.H[i0 * n + c], m1 = L.H[i1 * n + c];
                if ((c & 1) == 0) m0 += DT * DT * L.Sd[m_];
                else m1 += DT * DT * L.Sv[m_];
                if (c == i0) m0 += D[0] + D[1] + wr + wrm;
                if (c == i0 - 2) m0 -= wrm;
                if (c == i1) m1 += D[2] + D[3];
                if (c <= i0) L.M[i0 * n + c] = m0;
                L.M[i1 * n + c] = m1;
            }
        }
    };

    const double gv[2] = {g0, g1};
    double u[2], lam[10];
    int it_done;
    qp_ipm<64, 2, 10>(QpIpmLds{L.H, L.M, L.U, L.Y}, n, tau, gv, h, valid, 10.0 * T - 2.0, max_iter, tol, done, st, it_done, u, lam, gmul,
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

size_t stmpc_qp_lds_bytes(int T) { return sizeof(double) * (size_t)stqp_lds_doubles(T); }

int launch_stmpc_qp(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_pa, const double* d_pd, int pstride, int E,
                    const f1p_stmpc_cfg* cfg, int max_iter, double tol, double* d_steer, double* d_speed, int32_t* d_status, double* d_u,
                    double* d_x, double* d_obj, double* d_duals, int32_t* d_iters, double* d_warm_out) {
    if (E <= 0) return F1P_OK;
    const size_t lds = stmpc_qp_lds_bytes(cfg->horizon);
    const int rc = qp_lds_opt_in(ctx, reinterpret_cast<const void*>(&k_stmpc_qp), lds, "stmpc qp: horizon too long for the CU's LDS");
    if (rc) return rc;
    hipLaunchKernelGGL(k_stmpc_qp, dim3((unsigned)E), dim3(64), lds, ctx->stream, d_x0, d_ref, d_pa, d_pd, pstride, E, *cfg, max_iter, tol,
                       d_steer, d_speed, d_status, d_u, d_x, d_obj, d_duals, d_iters, d_warm_out);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_qp launch");
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
