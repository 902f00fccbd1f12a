// k_stmpc.hip -- dynamic single-track model as a second rollout model for shooting MPC.
//
// Replaces update_state / predict_motion / calc_ref_trajectory of control/dynamic_mpc/dynamic_mpc.py (:195-233, :280-404),
// its objective (:616-622), bounds (:685-706) applied as a projection of each sampled control sequence, and the output
// map (:1112-1117).  Same mapping as K4 (k_kmpc.hip): one 256-thread workgroup per ego, one thread per rollout, f32
// controls [ego][t][steering speed | accel][rollout] streamed from HBM, the 7-row reference in LDS, fp64 arithmetic.
// f1p_stmpc_plan_* runs the same kernel templates with the controls GENERATED in registers (the *_gen kernels).
#include "f1p_internal.h"
#include "shoot_gen.h"
#include "shoot_col.h"

namespace f1p {

__device__ __forceinline__ double clampd2(double v, double lo, double hi) { return v > hi ? hi : (v < lo ? lo : v); }

// predict_motion :280-300, one thread per ego
__global__ __launch_bounds__(256) void k_stmpc_predict(const double* __restrict__ x0, const double* __restrict__ oa,
                                                       const double* __restrict__ od, int E, f1p_stmpc_cfg cfg,
                                                       double* __restrict__ path) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int T = cfg.horizon;
    const DynConst k = dyn_const(cfg);
    DynState s;
    s.x = x0[7 * e]; s.y = x0[7 * e + 1]; s.delta = x0[7 * e + 2]; s.v = x0[7 * e + 3]; s.yaw = x0[7 * e + 4];
    s.yr = x0[7 * e + 5]; s.beta = x0[7 * e + 6];
    double* p = path + (size_t)e * 7 * (T + 1);
    for (int t = 0; t <= T; ++t) {
        if (t > 0) dyn_step<false>(s, oa[(size_t)e * T + t - 1], od[(size_t)e * T + t - 1], cfg, k);
        p[t] = s.x; p[(T + 1) + t] = s.y; p[2 * (T + 1) + t] = s.delta; p[3 * (T + 1) + t] = s.v; p[4 * (T + 1) + t] = s.yaw;
        p[5 * (T + 1) + t] = s.yr; p[6 * (T + 1) + t] = s.beta;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Where a rollout's controls come from (the seam of k_kmpc.hip's SrcStream / SrcGen, for the dynamic model's channels):
//   streamed : the f32 buffer [t][steering speed | accel][rollout] of one ego in HBM (f1p_stmpc_shoot_*);
//   generated: in registers from (seed, call, ego, rollout, t) around the ego's warm start (f1p_stmpc_plan_*; shoot_gen.h: channel 0 =
//              steering speed with sigma sig_dv, channel 1 = accel with sig_a).  The filter, the refinement, the all-fp64 fallback and
//              the winner's re-emission call the same pure function, so they all see the same controls and no controls buffer exists.
// The shooting kernels are templates over the source (below).
// StCtlGen is the generating kernels' parameter.  ids (nullable): the launch is a compacted list of a larger batch, ego e of the launch
// is ego ids[e] of that batch.  The generator's ego word is the ego's index in the caller's batch (+ ego_off: the batch is itself a
// shard of a larger one), its warm start the row of that index in `warm` (wstride floats per ego, [T][2] = (steering speed, accel)
// used; all zero = none): an ego's plan depends on that ego alone.  The decision kernel overwrites the row with the next warm start.
// ---------------------------------------------------------------------------------------------------------------------------------
// the generated source of the fp64 paths, read the way the shooting kernels read a step: its steering speed, then its accel.  dv(t, r)
// makes the step's one Philox call and keeps the accel; a() hands it out and must follow dv() of the same step.
struct StGenSrc {
    SrcGenT<true> g;
    mutable float a_;
    __device__ __forceinline__ float dv(int t, int r) const { float v; g.get(t, r, v, a_); return v; }
    __device__ __forceinline__ float a() const { return a_; }
};
struct StCtlGen {
    uint32_t k0, k1, call, ego_off;
    float sig_dv, sig_a;
    float* warm;
    const int32_t* ids;
    int wstride;
    __device__ __forceinline__ int row(int e) const { return ids ? ids[e] : e; }
    __device__ __forceinline__ float* warm_row(int e) const { return warm + (size_t)row(e) * wstride; }
    __device__ __forceinline__ SrcGenT<true> src(int e, const float* w) const {
        SrcGenT<true> s;
        s.k0 = k0; s.k1 = k1; s.call = call; s.ego = (uint32_t)row(e) + ego_off; s.sig_a = sig_dv; s.sig_d = sig_a;   // (SrcGenT calls its channels 0 / 1 "a" / "d")
        s.warm = w;
        return s;
    }
};

// ===================================================================================================================
// Round 3: f32 filter + fp64 decision for the dynamic single-track shooting (the pattern of k_kmpc_shoot_mixed / the lattice
// filter; VERDICT r2 "next" #8).  Outputs are bit-identical to k_stmpc_shoot.
//   pass A (f32, every rollout): the step of dyn_step in ego-relative coordinates (x - x0, y - y0, yaw - yaw0: the map-frame
//     magnitudes would cost the cost terms their digits), hardware sin / cos of the relative heading + slip angle rotated by the start
//     heading, tan(delta) by its odd polynomial (|delta| <= 0.45) or sin / cos, the five divisions by v as ONE v_rcp_f32.
//   TRUST: the yaw-rate equation is yr' = ... - A3 yr / v, integrated by explicit Euler with dt A3 / v ~ 2.8 / v for the reference's
//     vehicle: below v ~ 1.5 m/s the REFERENCE'S OWN integration is unstable (|1 - dt A3 / v| > 1) and beta / yr grow chaotically --
//     in fp64 as in f32, but differently, so an f32 cost of such a rollout says nothing about its fp64 cost (and beta enters x, y
//     through cos / sin, so those costs are moderate, not huge: they can be near the minimum).  A rollout is trusted only while
//     v >= v_trust at every step, v_trust = 1.05 dt max(A3, 2 A5) / 1.8 from the configuration (both modes contractive with margin);
//     everything else -- and every non-finite f32 cost -- is refined.
//   near-minimum set: trusted rollouts within the margin of the trusted f32 minimum + all untrusted ones; more than 64 (or none
//     trusted) -> the ego falls back to the all-fp64 loop.
//   pass B (fp64): the listed rollouts by stmpc_rollouts' own arithmetic (k_stmpc_refine_tp: one wave each, lanes over the time steps),
//     np.argmin's rule over THOSE costs (k_stmpc_decide).
//   NaN controls: the fp64 bounds (clampd2) keep a NaN, the rollout's fp64 cost is NaN and np.argmin's rule makes the first such rollout the
//     winner -- while v_med3_f32 with a NaN operand returns the smaller of the other two, so the f32 rollout would carry on with -max and a
//     finite cost.  RULE: a rollout with a NaN among its raw controls is UNTRUSTED (listed, fp64 decides).  Streamed controls: each
//     step's two raw controls go through one unordered compare (v_cmp_u_f32 dv_raw, a_raw: true iff either is a NaN; exact, +-inf is not
//     flagged) that ANDs into `trusted` beside the speed test -- scalar registers, no VGPR.  Generated controls are fma(sigma z, warm[t]) with sigma validated finite by
//     the entry points: a NaN needs a non-finite warm-start entry (inf x 0 in rollout 1 included), and only f1p_stmpc_warm_set can put one
//     there (the emission writes clamped controls).  It scans what it uploads, and while the flag stands stmpc_shoot_any runs the generated
//     plan through the all-fp64 kernel: no device code for it.  The f32 arithmetic of a finite rollout is what it was.
// Exactness: the fp64 minimiser r* has cost64(r*) <= cost64(r32), so if trusted cost32(r*) <= cost32(r32) + 2 err <= min32 + margin
// (margin >= 2 err, measured by tools/stmpc_filter_error.py and sized 40x above it); untrusted r* is listed by construction.
// ===================================================================================================================
#ifndef F1P_ST_MARGIN_REL
#define F1P_ST_MARGIN_REL 2.0e-5f     // per time step of the horizon, relative to the minimum (measured error <= 3e-7 T, tools/stmpc_filter_error.py)
#endif
#ifndef F1P_ST_MARGIN_ABS
#define F1P_ST_MARGIN_ABS 2.0e-2f
#endif
#define F1P_ST_MAX_REFINE 64
#ifndef F1P_ST_FILTER_NR
#define F1P_ST_FILTER_NR 1             // rollouts per thread of k_stmpc_filter side by side (2: 154 VGPRs -> 3 waves per SIMD, or spills at 128: 58.8 us against 55)
#endif
struct DynF32 {
    // dt A_i(a) = ap[i] + aq[i] a (i = 1..6 -> index 0..5): the six coefficients of update_state are affine in the acceleration
    float ap[6], aq[6], dt, dt_inv_wb, c0, s0;
    float max_steer, max_steer_v, max_accel, max_speed, min_speed, v_trust;
    float q[7], qf[7], r[2], rd[2];
};

// a wave-uniform f32 in a VGPR: VALU instructions with an SGPR operand issue in 4.3 cycles instead of 2.5 (profiles/r03_valu_issue_cycles.txt)
__device__ __forceinline__ float in_vgpr(float x) { float r; asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x)); return r; }

// f32 cost of one rollout in ego-relative coordinates; trusted = the speed stayed in the stable range of the reference's integrator.
// sref8: [T+1][8] floats (x - x0, y - y0, delta, v, yaw - yaw0, yr, beta, -) so one step's reference is two ds_read_b128.
// NR rollouts of one thread side by side (r, r + stride, ...).  At 4 waves per SIMD one chain per wave leaves a third of the issue slots
// empty (55 us against 36 us of instructions), but two chains need 154 VGPRs with the configuration held in registers: measured 58.8 us
// (3 waves per SIMD, or spills under a 128-register cap); with the configuration left in SGPRs two chains fit in 90 VGPRs but measure
// 0.105 ms per plan against 0.101 for one chain (and 0.090 with the configuration in VGPRs): NR = 1 is what runs.
// QM: bit j set = row j of the state carries weight in q or qf (compile-time: the reference's own weights leave delta, yr and beta
// unweighted, three of the seven terms of every step)
// one step of the f32 filter for rollout slot i, as text: the stage cost of the OLD state, then the step (dynamic_mpc.py:317-404; B_i = dt A_i,
// the angle in revolutions for the hardware sin / cos).  Expects dv, a (this step's controls after the bounds :701-706; the rate limit :685
// is applied here), t, r0 / r1 (the step's reference row), k and the state arrays.  A macro so that the streamed and the generating rollouts
// share it while the streamed function's tokens stay exactly what they were.
#define F1P_ST_F32_STEP(i) \
            if (t > 0) dv = __builtin_amdgcn_fmed3f(dv, pdv[i] - k.max_steer_v, pdv[i] + k.max_steer_v); \
            { \
                const float sv_[7] = {x[i], y[i], delta[i], v[i], yaw[i], yr[i], beta[i]}, rf_[7] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z}; \
                float qs = 0.f; \
_Pragma("unroll") \
                for (int j = 0; j < 7; ++j) if (QM & (1 << j)) { const float er = sv_[j] - rf_[j]; qs += k.q[j] * er * er; } \
                cost[i] += qs; \
            } \
            cost[i] += k.r[0] * dv * dv + k.r[1] * a * a; \
            if (t > 0) { const float d0 = dv - pdv[i], d1 = a - pa[i]; cost[i] += k.rd[0] * d0 * d0 + k.rd[1] * d1 * d1; } \
            trusted[i] &= v[i] >= k.v_trust; \
            const float B1 = k.ap[0] + k.aq[0] * a, B2 = k.ap[1] + k.aq[1] * a, B3 = k.ap[2] + k.aq[2] * a; \
            const float B4 = k.ap[3] + k.aq[3] * a, B5 = k.ap[4] + k.aq[4] * a, B6 = k.ap[5] + k.aq[5] * a; \
            const float ang = (yaw[i] + beta[i]) * 0.15915494309189535f; \
            const float sn_r = __builtin_amdgcn_sinf(ang), cs_r = __builtin_amdgcn_cosf(ang); \
            const float cs = k.c0 * cs_r - k.s0 * sn_r, sn = k.s0 * cs_r + k.c0 * sn_r; \
            float tn; \
            if (POLY) { \
                const float d2 = delta[i] * delta[i]; \
                tn = delta[i] * (1.0f + d2 * (0.33333333f + d2 * (0.13333333f + d2 * (0.053968254f + d2 * (0.021869489f + d2 * 0.0088632355f))))); \
            } else { \
                const float dr = delta[i] * 0.15915494309189535f; \
                tn = __builtin_amdgcn_sinf(dr) * __builtin_amdgcn_rcpf(__builtin_amdgcn_cosf(dr)); \
            } \
            const float iv = __builtin_amdgcn_rcpf(v[i]); \
            const float vdt = v[i] * k.dt; \
            const float x_new = x[i] + vdt * cs, y_new = y[i] + vdt * sn; \
            const float delta_new = __builtin_amdgcn_fmed3f(delta[i] + dv * k.dt, -k.max_steer, k.max_steer); \
            const float v_new = __builtin_amdgcn_fmed3f(v[i] + a * k.dt, k.min_speed, k.max_speed); \
            const float yaw_new = yaw[i] + (v[i] * k.dt_inv_wb) * tn; \
            const float yri = yr[i] * iv; \
            const float yr_new = yr[i] + (B1 * delta[i] + B2 * beta[i] - B3 * yri); \
            const float beta_new = (beta[i] - yr[i] * k.dt) + (B4 * delta[i] - B5 * beta[i] + B6 * yri) * iv; \
            x[i] = x_new; y[i] = y_new; delta[i] = delta_new; v[i] = v_new; yaw[i] = yaw_new; yr[i] = yr_new; beta[i] = beta_new; \
            pdv[i] = dv; pa[i] = a;

template <bool POLY, int NR, int QM>
__device__ __forceinline__ void stmpc_rollout_f32(const float* __restrict__ ce, const float* sref8, const DynF32& k, int T, int R, const int (&rr)[NR],
                                                  float delta0, float v0, float yr0, float beta0, float (&cost_out)[NR], bool (&trusted)[NR]) {
#pragma clang fp contract(fast)
    float x[NR], y[NR], delta[NR], v[NR], yaw[NR], yr[NR], beta[NR], cost[NR], pdv[NR], pa[NR], n_dv[NR], n_a[NR];
    const float* cp[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        x[i] = 0.f; y[i] = 0.f; delta[i] = delta0; v[i] = v0; yaw[i] = 0.f; yr[i] = yr0; beta[i] = beta0; cost[i] = 0.f; pdv[i] = 0.f; pa[i] = 0.f;
        trusted[i] = true;
        cp[i] = ce + rr[i];                                                // [t][2][R]: two loads per step, fetched one step ahead
        n_dv[i] = cp[i][0]; n_a[i] = cp[i][R];
    }
    const float4* sr = reinterpret_cast<const float4*>(sref8);
    for (int t = 0; t < T; ++t) {
        const float4 r0 = sr[2 * t], r1 = sr[2 * t + 1];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            float dv = __builtin_amdgcn_fmed3f(n_dv[i], -k.max_steer_v, k.max_steer_v);
            const float a = __builtin_amdgcn_fmed3f(n_a[i], -k.max_accel, k.max_accel);
            trusted[i] &= !__builtin_isunordered(n_dv[i], n_a[i]);      // NaN controls (the filter's header): ONE compare takes both raw channels, its result in scalar registers
            cp[i] += 2 * (size_t)R;
            if (t + 1 < T) { n_dv[i] = cp[i][0]; n_a[i] = cp[i][R]; }   // (two steps ahead measured slower: 0.094 against 0.089 ms per plan)
            F1P_ST_F32_STEP(i)
        }
    }
    const float4 r0 = sr[2 * T], r1 = sr[2 * T + 1];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const float sv_[7] = {x[i], y[i], delta[i], v[i], yaw[i], yr[i], beta[i]}, rf_[7] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z};
        float qs = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) if (QM & (1 << j)) { const float er = sv_[j] - rf_[j]; qs += k.qf[j] * er * er; }
        cost_out[i] = cost[i] + qs;
    }
}

// the same rollout with its controls GENERATED: one Philox4x32-10 call per pair of steps (SrcGenT::get2), nothing fetched but the step's
// warm-start row (LDS, wave-uniform address).  An overload on the source type; R is unused.  After every step the step's n_sub tested
// points -- formed from the f32 states, relative to the ego with the map's axes (unsure<false>) -- are tested as `test` says (shoot_col.h):
// ColTestNone: not at all, the plain filter; ColTestGrid: looked up in the clearance map (f1p_stmpc_set_collision, k_stmpc_filter_gen_col;
// the position bound: DESIGN.md 5i); ColTestObs: compared with every live slot of the ego's LDS table at the point's own time, and looked
// up as well while the occupancy test is on (f1p_stmpc_set_obstacles, k_stmpc_filter_gen_obs).
// unsure = a point is near an occupied cell, off the image, NaN or not clear of a disc: the rollout is not proved FREE.
template <bool POLY, int NR, int QM, typename Test>
__device__ __forceinline__ void stmpc_rollout_f32(const SrcGenT<true>& ce, const float* sref8, const DynF32& k, int T, int R, const int (&rr)[NR],
                                                  float delta0, float v0, float yr0, float beta0, float (&cost_out)[NR], bool (&trusted)[NR],
                                                  const Test& test, bool (&unsure)[NR]
#ifdef F1P_ST_DBG_POS    // variant build (tools/stmpc_pos_error.py): the f32 positions after every step, [t][x | y] planes of pos_stride floats
                                                  , float* pos_out, size_t pos_stride
#endif
                                                  ) {
#pragma clang fp contract(fast)
    (void)R;
    float x[NR], y[NR], delta[NR], v[NR], yaw[NR], yr[NR], beta[NR], cost[NR], pdv[NR], pa[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        x[i] = 0.f; y[i] = 0.f; delta[i] = delta0; v[i] = v0; yaw[i] = 0.f; yr[i] = yr0; beta[i] = beta0; cost[i] = 0.f; pdv[i] = 0.f; pa[i] = 0.f;
        trusted[i] = true; unsure[i] = false;
    }
    [[maybe_unused]] bool testing = true;                              // (the discs: every slot empty and no grid -> the plain filter, step by step)
    if constexpr (std::is_same_v<Test, ColTestObs>) testing = test.of.grid | (test.of.n_live > 0);
    const float4* sr = reinterpret_cast<const float4*>(sref8);
    for (int te = 0; te < T; te += 2) {
        float c_dv[NR][2], c_a[NR][2];
#pragma unroll
        for (int i = 0; i < NR; ++i) ce.get2(te, T, rr[i], c_dv[i][0], c_a[i][0], c_dv[i][1], c_a[i][1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = te + h;
            if (t < T) {
                const float4 r0 = sr[2 * t], r1 = sr[2 * t + 1];
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    float dv = __builtin_amdgcn_fmed3f(c_dv[i][h], -k.max_steer_v, k.max_steer_v);
                    const float a = __builtin_amdgcn_fmed3f(c_a[i][h], -k.max_accel, k.max_accel);
                    [[maybe_unused]] const float px = x[i], py = y[i];
                    F1P_ST_F32_STEP(i)
                    if constexpr (std::is_same_v<Test, ColTestGrid>) {          // j = 1 .. n_sub - 1, then p_{t+1} itself
                        const KmpcColF& cf = test.cf;
                        for (int j = 1; j < cf.n_sub; ++j) {
                            const float f = (float)j * cf.inv_nsub;
                            unsure[i] |= cf.template unsure<false>(px + (x[i] - px) * f, py + (y[i] - py) * f);
                        }
                        unsure[i] |= cf.template unsure<false>(x[i], y[i]);
                    }
                    if constexpr (std::is_same_v<Test, ColTestObs>) {           // j = 1 .. n_sub, every point at its own time
                        const KmpcColF& cf = test.cf;
                        const KmpcObsF& of = test.of;
                        if (testing) {
                            for (int j = 1; j <= cf.n_sub; ++j) {
                                const bool end = j == cf.n_sub;
                                const float f = end ? 1.0f : (float)j * cf.inv_nsub;
                                const float qx = end ? x[i] : px + (x[i] - px) * f, qy = end ? y[i] : py + (y[i] - py) * f;
                                if (of.grid) unsure[i] |= cf.template unsure<false>(qx, qy);
                                const float tau = ((float)t + f) * of.dt;
                                for (int m = 0; m < of.n_live; ++m) {
                                    const float* o = of.live + 5 * m;
                                    const float cx = o[0] + o[2] * tau, cy = o[1] + o[3] * tau;
                                    const float dx = qx - cx, dy = qy - cy, d2 = dx * dx + dy * dy;
                                    unsure[i] |= !(d2 > o[4]);
                                }
                            }
                        }
                    }
#ifdef F1P_ST_DBG_POS
                    if (pos_out) { pos_out[((size_t)t * 2 + 0) * pos_stride + rr[i]] = x[i]; pos_out[((size_t)t * 2 + 1) * pos_stride + rr[i]] = y[i]; }
#endif
                }
            }
        }
    }
    const float4 r0 = sr[2 * T], r1 = sr[2 * T + 1];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const float sv_[7] = {x[i], y[i], delta[i], v[i], yaw[i], yr[i], beta[i]}, rf_[7] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z};
        float qs = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) if (QM & (1 << j)) { const float er = sv_[j] - rf_[j]; qs += k.qf[j] * er * er; }
        cost_out[i] = cost[i] + qs;
    }
}

// ---- K-A: f32 filter, one workgroup per ego; no fp64 rollout code in this kernel (registers for 8 waves per SIMD) ----------------
// nlist[e] = listed rollouts (<= 64) or -1 (this ego is decided by the all-fp64 loop in k_stmpc_decide); the listed rollouts go to
// rl[e][slot] and, as (e * 64 + slot, r), onto the global queue that k_stmpc_refine packs into full waves across egos.
// (The kernels K-A, K-B, K-B' and K-C themselves follow below, as templates; their types and their notes stay here.)
struct StItem { int es, r; };

// ---- K-B', time-parallel: ONE WAVE per queued rollout, lanes over the time steps (horizon <= 63) ---------------------------------
// Of the 7 states only (yr, beta) are truly recurrent.  delta and v follow from the controls alone (clamped running sums), yaw from
// (v, delta), x / y from (v, yaw + beta), and the cost from all of them -- so everything expensive (tan(delta), the six A_i(a), the
// sincos of yaw + beta, the 7-term cost rows) is computed with lane = step, and what stays sequential are five short loops of additions,
// clamps and the three quotients by v, fed from LDS one step ahead:
//   1  dv_t (rate clamp), delta_t, v_t                      2  (lanes) A_i, tan delta_t, yaw increment, the yr / beta coefficients
//   3  yr_t, beta_t, yaw_t  (3 divisions + 12 operations per step: the recurrence proper)
//   4  (lanes) sincos(yaw_t + beta_t) -> x / y increments    5  x_t, y_t      6  (lanes) cost rows      7  the cost's running sum
// Every operation is the one dyn_step / stmpc_rollouts performs on the same operands, and every running sum is formed in their order,
// so the cost is bit-identical to stmpc_one_rollout's (tests/test_gpu_stmpc.py compares whole plans with k_stmpc_shoot).
struct StS1 { double u, a; };
struct StS3 { double P1, A2, A3, A4d, A5, A6, v, vv, w, pad; };
struct StO3 { double yr, beta, yaw, pad; };
struct StXY { double x, y; };
struct StC { double q, r, rd, pad; };
#define F1P_ST_TP_LDS_PER_WAVE (64 * (sizeof(StS1) + sizeof(StS3) + sizeof(StO3) + 2 * sizeof(StXY) + sizeof(StC)))

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): this wave's LDS traffic is done
    __builtin_amdgcn_wave_barrier();
}

// ---- the shooting kernels: templates over the control source and the optional occupancy test --------------------------------------
// Ctl, the kernels' control parameter, is StCtlStream or StCtlGen.  The bodies choose by `if constexpr (st_gen<Ctl>)`; the streamed branch
// spells the raw pointer and its index arithmetic out at the use site, which is what keeps the streamed kernels' instructions what they
// were (a wrapper object or an accessor function does not: tools/listing_diff.py is the check after every change here).
// Col..., nothing or one KmpcCol (StColRef in the two refinement kernels), is the occupancy test of f1p_stmpc_set_collision (DESIGN.md 5i;
// shoot_col.h has_col / col_of): the fp64 rollouts test each step as they take it, the filter looks its tested points up in the clearance
// map and lists FREE and UNSURE rollouts, the refinement marks a blocked item (cost +inf, listed index F1P_K4_NONE), the decision skips
// those.  Filter, refinement and decision with the test exist for generated controls only: f1p_stmpc_shoot_* run the plain-fp64 kernel
// while the test is on.  The instantiations are the ones named below the kernels -- nothing that is not launched.
// Col can also be StObs (StObsRef in the refinement), the moving discs of f1p_stmpc_set_obstacles with the grid or without:
// a KmpcCol too, so the same statements serve it; has_obs marks what the discs add, col_seg(col, t, dt, ...) picks the segment rule.
using StCtlStream = const float* __restrict__;
template <typename Ctl> constexpr bool st_gen = std::is_same_v<Ctl, StCtlGen>;
// ego e's source: as a value, and as the device functions take it
template <typename Ctl> using st_ego_t = std::conditional_t<st_gen<Ctl>, StGenSrc, const float*>;
template <typename Ctl> using st_src_t = std::conditional_t<st_gen<Ctl>, const StGenSrc&, const float* __restrict__>;
// the refinement kernels' form of the test: they also rewrite the listed index of a blocked item
struct StColRef : KmpcCol { int32_t* rl; };

// The moving discs of f1p_stmpc_set_obstacles: KmpcObs with what the dynamic model's kernels need beside it.  The drop rule of
// obs_compact takes its operands in fp64 from here (the filter kernel has the configuration in f32 only).  The ego's obstacle row is
// ids ? ids[e] : e -- the array is in the CALLER's ego order, a plan_batch branch is a compacted list.  The kernels that own an ego per workgroup
// (shoot, filter, decide) compact the live slots into LDS (st_obs_setup / st_obs_bind); the filter also copies its table to tab / ntab, where
// the refinement -- whose items come from many egos -- reads it with wave-uniform addresses.
// nan_all: the ego has a live slot (before the drop).  Against a live slot a tested point with a NaN coordinate is blocked wherever the slot
// is (!(NaN > r r)), and the dynamic model makes NaN positions out of finite states (yr / v and beta / v at v = 0), so a dropped slot must
// still block those: seg_t tests the point itself.  An infinite coordinate is free against every tame slot, dropped or not.
#define F1P_ST_OBS_LDS64 (sizeof(double) * 5 * F1P_KMPC_MAX_OBS + sizeof(int) * 4)                    // fp64 rows, the two counts
#define F1P_ST_OBS_LDS32 (8 + F1P_ST_OBS_LDS64 + sizeof(float) * 5 * F1P_KMPC_MAX_OBS)                 // (+ alignment) + the filter's f32 rows
struct StObs : KmpcObs {
    double dt, max_speed, min_speed, pos_err;
    const int32_t* ids;
    double* tab;                      // [E][F1P_KMPC_MAX_OBS][5]
    int32_t* ntab;                    // [E]: n_live | nan_all << 8
    int nan_all;
    __device__ __forceinline__ bool seg_t(int t, double dt_, double px, double py, double qx, double qy) const {
        bool hit = false;
        for (int j = 1; j <= n_sub; ++j) {
            const double f = (double)j / (double)n_sub;
            const bool end = j == n_sub;
            const double x = end ? qx : px + (qx - px) * f, y = end ? qy : py + (qy - py) * f;
            if (g.bits) hit |= occupied(x, y);
            hit |= disc(x, y, ((double)t + f) * dt_);
            hit |= (nan_all != 0) & !((x == x) & (y == y));
        }
        return hit;
    }
};
struct StObsRef : StObs { int32_t* rl; };
__device__ __forceinline__ bool col_seg(const StObs& c, int t, double dt, double px, double py, double qx, double qy) { return c.seg_t(t, dt, px, py, qx, qy); }
// the workgroup's first wave (all its lanes): ego e's live slots -> live64 (and live32), the counts -> n2[0] (kept), n2[1] (any live slot)
__device__ __forceinline__ void st_obs_setup(const StObs& ob, int e, double sx, double sy, double sv, double syaw, int T, double* live64, float* live32, int* n2) {
    const int row = ob.ids ? ob.ids[e] : e;
    const bool live = (int)threadIdx.x < ob.M && ob.obs[((size_t)row * ob.M + threadIdx.x) * 5 + 4] >= 0.0;
    const unsigned long long any = __ballot(live);
    if (threadIdx.x == 0) n2[1] = any != 0ull;
    obs_compact(ob, row, sx, sy, sv, syaw, T, ob.dt, ob.max_speed, ob.min_speed, false, 1.0, 0.0, live64, live32, n2, ob.pos_err);
}
// behind the barrier
__device__ __forceinline__ void st_obs_bind(StObs& ob, const double* live64, const int* n2) {
    ob.live = live64; ob.n_live = __builtin_amdgcn_readfirstlane(n2[0]); ob.nan_all = __builtin_amdgcn_readfirstlane(n2[1]);
}
// the refinement's: ego e's table as the filter left it
template <typename O> __device__ __forceinline__ O st_obs_of_ego(const O& ob, int e) {
    O o = ob;
    const int w = ob.ntab[e];
    o.live = ob.tab + (size_t)e * 5 * F1P_KMPC_MAX_OBS; o.n_live = w & 0xff; o.nan_all = w >> 8;
    return o;
}

#ifdef F1P_ST_PHASES
#define F1P_STPH() do { ph[nph++] = clock64(); } while (0)
#else
#define F1P_STPH() do {} while (0)
#endif

// all rollouts of this thread, first-minimum argmin (objective :616-622, bounds :685-706 as a projection)
template <bool FAST, typename Ctl, typename... Col>
__device__ __forceinline__ void stmpc_rollouts(st_src_t<Ctl> ce, const double* sref, const f1p_stmpc_cfg& cfg, const DynConst& k,
                                               const DynState& s0, int tid, double& bc, int& bi, const Col&... col) {
    const int T = cfg.horizon, R = cfg.n_rollouts;
    for (int r = tid; r < R; r += blockDim.x) {
        DynState s = s0;
        double cost = 0.0, pdv = 0.0, pa = 0.0;
        [[maybe_unused]] bool blocked = false;
        for (int t = 0; t < T; ++t) {
            float c;                                                  // (generated: dv() makes the step's one Philox call, a() hands out its accel)
            if constexpr (st_gen<Ctl>) c = ce.dv(t, r); else c = ce[((size_t)t * 2 + 0) * R + r];
            double dv = clampd2((double)c, -cfg.max_steer_v, cfg.max_steer_v);   // :701-703
            if constexpr (st_gen<Ctl>) c = ce.a(); else c = ce[((size_t)t * 2 + 1) * R + r];
            double a = clampd2((double)c, -cfg.max_accel, cfg.max_accel);        // :704-706
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);                         // :685
            const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + t]; q += cfg.q[j] * er * er; }   // :619
            cost += q;
            cost += cfg.r[0] * dv * dv + cfg.r[1] * a * a;                                                       // :616
            if (t > 0) { const double d0 = dv - pdv, d1 = a - pa; cost += cfg.rd[0] * d0 * d0 + cfg.rd[1] * d1 * d1; }   // :622
            [[maybe_unused]] const double px = s.x, py = s.y;
            dyn_step<FAST>(s, a, dv, cfg, k);
            if constexpr (has_col<Col...>) {
                if (col_seg(col_of(col...), t, cfg.dt, px, py, s.x, s.y)) { blocked = true; break; }   // the points of step t -> t + 1; a blocked rollout stops at its first occupied point
            }
            pdv = dv; pa = a;
        }
        if constexpr (has_col<Col...>) { if (blocked) continue; }     // takes no part in the argmin: (bc, bi) stays (+inf, F1P_K4_NONE) while nothing is free
        const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + T]; q += cfg.qf[j] * er * er; }
        cost += q;
        if (argmin_better(cost, r, bc, bi)) { bc = cost; bi = r; }
    }
}

// The winner's re-emission (every thread, bi known to all) stands in k_stmpc_shoot_t and in k_stmpc_decide_t, and so does the "every
// rollout blocked" epilogue: as shared device functions they change the kernels' register allocation (LABNOTES R10).  Streamed controls:
// thread 0 reads the winner's steps, and stops after step 0 when no best_seq is wanted.  Generated controls: the winner's T steps are
// regenerated with one thread per step into LDS (the kernels' reference rows are free by then), so that the one emitting thread neither
// runs T Philox calls in sequence nor waits for a warm-start load per step behind its own warm-start stores; the emission writes the next
// warm start -- the winner's APPLIED sequence shifted by one step, the last step repeated, rounded to f32 (the rule of kmpc_emit;
// dynamic_mpc.py:1052-1055 keeps self.oa / self.odelta_v the same way) -- into the row the generator reads: every read of it is behind
// the barrier, before the first write.  A blocked ego's row is zeroed: no warm start for its next plan.
template <typename Ctl, typename... Col>
__global__ __launch_bounds__(256) void k_stmpc_shoot_t(const double* __restrict__ x0, const double* __restrict__ ref,
                                                     Ctl ctl, int E, f1p_stmpc_cfg cfg, Col... col,
                                                     double* __restrict__ steer, double* __restrict__ speed,
                                                     int32_t* __restrict__ best_idx, double* __restrict__ best_cost,
                                                     double* __restrict__ best_seq) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double* sref = reinterpret_cast<double*>(lds_raw);   // [7][T+1]
    double* red_d = sref + 7 * (cfg.horizon + 1);
    int* red_i = reinterpret_cast<int*>(red_d + 4);
    const int e = blockIdx.x;
    if (e >= E) return;
    const int T = cfg.horizon, R = cfg.n_rollouts, tid = threadIdx.x;
    for (int q = tid; q < 7 * (T + 1); q += blockDim.x) sref[q] = ref[(size_t)e * 7 * (T + 1) + q];
    __syncthreads();
    const DynConst k = dyn_const(cfg);
    DynState s0;
    s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
    s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
    st_ego_t<Ctl> ce;
    if constexpr (st_gen<Ctl>) ce = StGenSrc{ctl.src(e, ctl.warm_row(e)), 0.0f}; else ce = ctl + (size_t)e * T * 2 * R;
    double bc = __builtin_huge_val(); int bi = 0x7fffffff;
    if constexpr (has_obs<Col...>) {                                  // the ego's live discs -> LDS behind the reduction's words
        double* olive = reinterpret_cast<double*>(red_i + 4);
        int* on2 = reinterpret_cast<int*>(olive + 5 * F1P_KMPC_MAX_OBS);
        if (tid < 64) st_obs_setup(col_of(col...), e, s0.x, s0.y, s0.v, s0.yaw, T, olive, nullptr, on2);
        __syncthreads();
        auto ob = col_of(col...);
        st_obs_bind(ob, olive, on2);
        if (fabs(cfg.max_steer) <= 1.0e4) stmpc_rollouts<true, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, ob);
        else stmpc_rollouts<false, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, ob);
    } else
    if (fabs(cfg.max_steer) <= 1.0e4) stmpc_rollouts<true, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, col...);     // workgroup-uniform
    else stmpc_rollouts<false, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, col...);
    block_argmin(bc, bi, red_d, red_i);
    if constexpr (has_col<Col...>) {
        if (bi == F1P_K4_NONE) {                                      // every rollout blocked (workgroup-uniform): the lattice's ALL_BLOCKED outputs
            for (int q = tid; q < 2 * T; q += blockDim.x) {
                if (best_seq) best_seq[(size_t)e * T * 2 + q] = 0.0;
                if constexpr (st_gen<Ctl>) ctl.warm_row(e)[q] = 0.0f;
            }
            if (tid == 0) {
                steer[e] = 0.0; speed[e] = 0.0; best_idx[e] = -1;
                if (best_cost) best_cost[e] = __builtin_huge_val();
            }
            return;
        }
    }
    [[maybe_unused]] float* emit_s = reinterpret_cast<float*>(lds_raw);
    if constexpr (st_gen<Ctl>) {
        for (int t_ = tid; t_ < T; t_ += blockDim.x) ce.g.get(t_, bi, emit_s[2 * t_], emit_s[2 * t_ + 1]);
        __syncthreads();
    }
    if (tid == 0) {
        double pdv = 0.0;
        for (int t = 0; t < T; ++t) {
            float c;
            if constexpr (st_gen<Ctl>) c = emit_s[2 * t]; else c = ce[((size_t)t * 2 + 0) * R + bi];
            double dv = clampd2((double)c, -cfg.max_steer_v, cfg.max_steer_v);
            if constexpr (st_gen<Ctl>) c = emit_s[2 * t + 1]; else c = ce[((size_t)t * 2 + 1) * R + bi];
            const double a = clampd2((double)c, -cfg.max_accel, cfg.max_accel);
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
            if (t == 0) {
                steer[e] = s0.delta + dv * cfg.dt;   // :1112
                speed[e] = s0.v + a * cfg.dt;        // :1117
            }
            if (best_seq) { best_seq[((size_t)e * T + t) * 2] = dv; best_seq[((size_t)e * T + t) * 2 + 1] = a; }
            else if constexpr (!st_gen<Ctl>) { if (t == 0) break; }
            if constexpr (st_gen<Ctl>) {
                float* wo_ = ctl.warm_row(e);
                if (t > 0) { wo_[2 * (t - 1)] = (float)dv; wo_[2 * (t - 1) + 1] = (float)a; }
                if (t == T - 1) { wo_[2 * t] = (float)dv; wo_[2 * t + 1] = (float)a; }
            }
            pdv = dv;
        }
        best_idx[e] = bi;
        if (best_cost) best_cost[e] = bc;
    }
}

// fp64 cost of ONE rollout: the body of stmpc_rollouts for a given r (same operations, same order)
template <bool FAST, typename Ctl, typename... Col>
__device__ __forceinline__ double stmpc_one_rollout(st_src_t<Ctl> ce, const double* sref, const f1p_stmpc_cfg& cfg, const DynConst& k,
                                                    const DynState& s0, int r, bool& blocked, const Col&... col) {
    const int T = cfg.horizon, R = cfg.n_rollouts;
    DynState s = s0;
    double cost = 0.0, pdv = 0.0, pa = 0.0;
    blocked = false;
    for (int t = 0; t < T; ++t) {
        float c;
        if constexpr (st_gen<Ctl>) c = ce.dv(t, r); else c = ce[((size_t)t * 2 + 0) * R + r];
        double dv = clampd2((double)c, -cfg.max_steer_v, cfg.max_steer_v);
        if constexpr (st_gen<Ctl>) c = ce.a(); else c = ce[((size_t)t * 2 + 1) * R + r];
        double a = clampd2((double)c, -cfg.max_accel, cfg.max_accel);
        if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
        const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + t]; q += cfg.q[j] * er * er; }
        cost += q;
        cost += cfg.r[0] * dv * dv + cfg.r[1] * a * a;
        if (t > 0) { const double d0 = dv - pdv, d1 = a - pa; cost += cfg.rd[0] * d0 * d0 + cfg.rd[1] * d1 * d1; }
        [[maybe_unused]] const double px = s.x, py = s.y;
        dyn_step<FAST>(s, a, dv, cfg, k);
        if constexpr (has_col<Col...>) {
            if (col_seg(col_of(col...), t, cfg.dt, px, py, s.x, s.y)) { blocked = true; return __builtin_huge_val(); }
        }
        pdv = dv; pa = a;
    }
    const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + T]; q += cfg.qf[j] * er * er; }
    cost += q;
    return cost;
}

template <int QM, typename Ctl, typename... Col>
__global__ __launch_bounds__(256) void k_stmpc_filter_t(const double* __restrict__ x0, const double* __restrict__ ref,
                                                      Ctl ctl, int E, int T, int R, double max_steer_d, DynF32 kf, Col... col,
                                                      unsigned int* __restrict__ qcount, StItem* __restrict__ items, int32_t* __restrict__ nlist,
                                                      int32_t* __restrict__ rl, float* __restrict__ dbg_cost32) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    float* sref32 = reinterpret_cast<float*>(lds_raw);               // [T+1][8] relative to the ego state
    float* c32 = sref32 + 8 * (T + 1);                                // [R] filter costs (-inf = untrusted)
    float* red_f = c32 + R;                                           // [4]
    int* list = reinterpret_cast<int*>(red_f + 4);                    // [F1P_ST_MAX_REFINE]
    int* cnt = list + F1P_ST_MAX_REFINE;                              // [2]: listed, queue base
    const int e = blockIdx.x;
    if (e >= E) return;
    const double sx = x0[7 * e], sy = x0[7 * e + 1], sdelta = x0[7 * e + 2], sv = x0[7 * e + 3], syaw = x0[7 * e + 4], syr = x0[7 * e + 5], sbeta = x0[7 * e + 6];
    constexpr bool COL = has_col<Col...>;
    constexpr bool OBS = has_obs<Col...>;                            // moving discs, with the grid (a bitmap) or without (null)
    [[maybe_unused]] double bxd = 0.0, byd = 0.0;
    if constexpr (COL) {
        // the ego's cell (fp64) anchors the filter's cell coordinates; an ego without one is decided in fp64.  Without a grid (the discs
        // alone: a null bitmap) there is no cell: the discs' FREE threshold carries the filter's position bound itself (obs_compact)
        const KmpcCol& c_ = col_of(col...);
        if (!OBS || c_.g.bits) { bxd = (sx - c_.g.ox) * c_.g.inv_res; byd = (sy - c_.g.oy) * c_.g.inv_res; }
    }
    const bool in_range = fabs(syaw) <= 1.0e4 && fabs(max_steer_d) <= 1.0e4 && fabs(sbeta) <= 100.0 && fabs(sdelta) <= 100.0 &&
                          (!COL || (fabs(bxd) < 1.0e6 && fabs(byd) < 1.0e6));   // workgroup-uniform
    if (!in_range) { if (tid == 0) nlist[e] = -1; return; }
    int bad_ref = 0;                                                 // a non-finite reference in an UNWEIGHTED row makes every fp64 cost NaN (0 * NaN): fp64 decides
    for (int q = tid; q < 7 * (T + 1); q += blockDim.x) {
        const double rv = ref[(size_t)e * 7 * (T + 1) + q];
        const int row = q / (T + 1), t = q - row * (T + 1);
        sref32[8 * t + row] = (float)(row == 0 ? rv - sx : (row == 1 ? rv - sy : (row == 4 ? rv - syaw : rv)));
        if (!((QM >> row) & 1) && !(fabs(rv) < __builtin_huge_val())) bad_ref = 1;
    }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    if constexpr (st_gen<Ctl>) {                                     // the ego's warm start: read T x R times, so from LDS, behind the other arrays
        float* ws_ = reinterpret_cast<float*>(cnt + 2); const float* wg_ = ctl.warm_row(e);
        for (int q = tid; q < 2 * T; q += blockDim.x) ws_[q] = wg_[q];
    }
    // the ego's live discs -> LDS behind the warm start: fp64 rows (for the refinement's table), the filter's f32 rows, the counts
    [[maybe_unused]] double* olive = nullptr;
    [[maybe_unused]] float* olive32 = nullptr;
    [[maybe_unused]] int* on2 = nullptr;
    if constexpr (OBS) {
        olive = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(reinterpret_cast<float*>(cnt + 2) + 2 * T) + 7) & ~(uintptr_t)7);
        on2 = reinterpret_cast<int*>(olive + 5 * F1P_KMPC_MAX_OBS);
        olive32 = reinterpret_cast<float*>(on2 + 4);
        if (tid < 64) st_obs_setup(col_of(col...), e, sx, sy, sv, syaw, T, olive, olive32, on2);
    }
    if (__syncthreads_or(bad_ref | ((QM != 0x7f && !(fabs(syr) < __builtin_huge_val())) ? 1 : 0))) { if (tid == 0) nlist[e] = -1; return; }
    std::conditional_t<st_gen<Ctl>, SrcGenT<true>, const float*> ce;
    if constexpr (st_gen<Ctl>) ce = ctl.src(e, reinterpret_cast<const float*>(cnt + 2)); else ce = ctl + (size_t)e * T * 2 * R;
    DynF32 kk;
#pragma unroll
    for (int j = 0; j < 6; ++j) { kk.ap[j] = in_vgpr(kf.ap[j]); kk.aq[j] = in_vgpr(kf.aq[j]); }
#pragma unroll
    for (int j = 0; j < 7; ++j) { kk.q[j] = in_vgpr(kf.q[j]); kk.qf[j] = kf.qf[j]; }
#pragma unroll
    for (int j = 0; j < 2; ++j) { kk.r[j] = in_vgpr(kf.r[j]); kk.rd[j] = in_vgpr(kf.rd[j]); }
    kk.dt = in_vgpr(kf.dt); kk.dt_inv_wb = in_vgpr(kf.dt_inv_wb);
    kk.max_steer = in_vgpr(kf.max_steer); kk.max_steer_v = in_vgpr(kf.max_steer_v); kk.max_accel = in_vgpr(kf.max_accel);
    kk.max_speed = in_vgpr(kf.max_speed); kk.min_speed = in_vgpr(kf.min_speed); kk.v_trust = in_vgpr(kf.v_trust);
    double s0d, c0d;
    sincos_core(syaw, &s0d, &c0d);
    kk.c0 = (float)c0d; kk.s0 = (float)s0d;
    // the filter's test of a step's points (shoot_col.h): none, the clearance look-ups, or the look-ups and the discs
    [[maybe_unused]] std::conditional_t<OBS, ColTestObs, std::conditional_t<COL, ColTestGrid, ColTestNone>> test;
    if constexpr (OBS) {
        const auto& o_ = col_of(col...);
        KmpcObsF& of = test.of;
        of.live = olive32; of.n_live = __builtin_amdgcn_readfirstlane(on2[0]); of.grid = o_.g.bits != nullptr; of.dt = kf.dt;
        // the refinement's copy of the table (it cannot compact per workgroup: its items come from many egos)
        if (tid < 5 * of.n_live) o_.tab[(size_t)e * 5 * F1P_KMPC_MAX_OBS + tid] = olive[tid];
        if (tid == 0) o_.ntab[e] = on2[0] | (on2[1] << 8);
    }
    if constexpr (COL) test.cf = col_filter(col_of(col...), bxd, byd, true, 1.0f, 0.0f);   // (the filter's positions are relative to the ego with the map's axes)
    // the odd polynomial of tan is good for |delta| <= 0.45: every later delta is clamped to max_steer, but step 0 evaluates tan(delta0)
    // UNCLAMPED (dyn_step does, like the reference) -- an out-of-range initial steering state takes the sin / cos path (workgroup-uniform)
    const bool poly = kf.max_steer <= 0.45f && fabs(sdelta) <= 0.45;
    float tmin = __builtin_huge_valf();
    constexpr int NR = F1P_ST_FILTER_NR;
    for (int rb = tid; rb < R; rb += NR * blockDim.x) {
        int rr[NR]; float c[NR]; bool trusted[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) rr[i] = rb + i * (int)blockDim.x < R ? rb + i * (int)blockDim.x : rb;   // past the end: a shadow of the first, not stored
        [[maybe_unused]] bool unsure[NR];                            // a tested point near an occupied cell, off the image or NaN: not FREE
        if constexpr (st_gen<Ctl>) {
#ifdef F1P_ST_DBG_POS    // variant build: dbg_cost32 is [1 + 2 T][E][R] -- the costs, then the f32 (x, y) after every step (tools/stmpc_pos_error.py)
#define F1P_ST_POS_ARGS , COL && !OBS && dbg_cost32 ? dbg_cost32 + ((size_t)E + e) * R : nullptr, (size_t)E * R
#else
#define F1P_ST_POS_ARGS
#endif
            if (poly) stmpc_rollout_f32<true, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted, test, unsure F1P_ST_POS_ARGS);
            else stmpc_rollout_f32<false, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted, test, unsure F1P_ST_POS_ARGS);
#undef F1P_ST_POS_ARGS
        } else {
            if (poly) stmpc_rollout_f32<true, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted);
            else stmpc_rollout_f32<false, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (i > 0 && rr[i] == rb) continue;
            float ci = c[i];
            if (!trusted[i] || !(ci == ci) || !(fabsf(ci) < 1e30f)) ci = -__builtin_huge_valf();      // untrusted / non-finite: fp64 decides
            else if constexpr (COL) { if (!unsure[i]) tmin = fminf(tmin, ci); }   // the threshold comes from the FREE rollouts; an UNSURE one keeps its cost and is listed at or below it
            else tmin = fminf(tmin, ci);
            c32[rr[i]] = ci;
            if (dbg_cost32) dbg_cost32[(size_t)e * R + rr[i]] = ci;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) tmin = fminf(tmin, __shfl_xor(tmin, m, 64));
    if (lane == 0) red_f[wave] = tmin;
    __syncthreads();
    tmin = red_f[0];
    for (int w = 1; w < nwaves; ++w) tmin = fminf(tmin, red_f[w]);
    // (no trusted rollout: tmin = +inf, thr = +inf and every rollout is listed -> fallback)
    const float thr = tmin + (fabsf(tmin) * fminf(F1P_ST_MARGIN_REL * (float)T, 0.5f) + F1P_ST_MARGIN_ABS);
    for (int r = tid; r < R; r += blockDim.x) {
        if (!(c32[r] > thr)) {
            const int pos = atomicAdd(cnt, 1);
            if (pos < F1P_ST_MAX_REFINE) list[pos] = r;
        }
    }
    __syncthreads();
    const int n = cnt[0];
    const bool fallback = n > F1P_ST_MAX_REFINE || n < 1 || !(tmin < __builtin_huge_valf());
    if (fallback) { if (tid == 0) nlist[e] = -1; return; }
    if (tid == 0) { cnt[1] = (int)atomicAdd(qcount, (unsigned int)n); nlist[e] = n; }
    __syncthreads();
    if (tid < n) {
        const int r = list[tid];
        rl[(size_t)e * F1P_ST_MAX_REFINE + tid] = r;
        StItem it; it.es = e * F1P_ST_MAX_REFINE + tid; it.r = r;
        items[(size_t)cnt[1] + tid] = it;
    }
}

// ---- K-B: fp64 costs of the queued rollouts, one lane each, packed across egos (stmpc_rollouts' own arithmetic) ----------------
// ~1 rollout per ego survives the filter, so this kernel is a few dozen waves running 40 sequential fp64 steps: 1.3 us per step (34 us
// for a single wave of 17 rollouts, 52 us at 1024 egos), latency of the dependent fp64 chain and not throughput.  This kernel now only
// serves horizons > 63; k_stmpc_refine_tp below is what runs.  Measured and NOT kept
// (profiles/r03_stmpc_filter.md): splitting the step's independent chains over four waves with an LDS exchange per step, staging the
// controls in LDS and batching the reference loads -- each left the time where it was.
template <typename Ctl, typename... Col>
__global__ __launch_bounds__(64) void k_stmpc_refine_t(const double* __restrict__ x0, const double* __restrict__ ref, Ctl ctl,
                                                     f1p_stmpc_cfg cfg, const unsigned int* __restrict__ qcount, const StItem* __restrict__ items,
                                                     Col... col, double* __restrict__ rc) {
    const unsigned int count = *qcount;
    const int T = cfg.horizon, R = cfg.n_rollouts;
    const DynConst k = dyn_const(cfg);
    for (unsigned int i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const StItem it = items[i];
        const int e = it.es / F1P_ST_MAX_REFINE;
        DynState s0;
        s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
        s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
        st_ego_t<Ctl> ce;
        if constexpr (st_gen<Ctl>) ce = StGenSrc{ctl.src(e, ctl.warm_row(e)), 0.0f}; else ce = ctl + (size_t)e * T * 2 * R;
        bool blocked;
        if constexpr (has_obs<Col...>) rc[it.es] = stmpc_one_rollout<true, Ctl>(ce, ref + (size_t)e * 7 * (T + 1), cfg, k, s0, it.r, blocked, st_obs_of_ego(col_of(col...), e));
        else
        rc[it.es] = stmpc_one_rollout<true, Ctl>(ce, ref + (size_t)e * 7 * (T + 1), cfg, k, s0, it.r, blocked, col...);
        if constexpr (has_col<Col...>) { if (blocked) col_of(col...).rl[it.es] = F1P_K4_NONE; }   // (its cost is +inf: the pair loses to every unblocked item)
    }
}

template <typename Ctl, typename... Col>
__global__ __launch_bounds__(256) void k_stmpc_refine_tp_t(const double* __restrict__ x0, const double* __restrict__ ref, Ctl ctl,
                                                        f1p_stmpc_cfg cfg, const unsigned int* __restrict__ qcount, const StItem* __restrict__ items,
                                                        Col... col, double* __restrict__ rc, float* __restrict__ dbg_ticks) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#ifdef F1P_ST_PHASES
    long long ph[12]; int nph = 0;
#endif
    unsigned char* wl = lds_raw + (size_t)wave * F1P_ST_TP_LDS_PER_WAVE;
    StS1* __restrict__ s1 = reinterpret_cast<StS1*>(wl);
    StS3* __restrict__ s3 = reinterpret_cast<StS3*>(wl + 64 * sizeof(StS1));
    StO3* __restrict__ o3 = reinterpret_cast<StO3*>(wl + 64 * (sizeof(StS1) + sizeof(StS3)));
    StXY* __restrict__ s6 = reinterpret_cast<StXY*>(wl + 64 * (sizeof(StS1) + sizeof(StS3) + sizeof(StO3)));
    StXY* __restrict__ o6 = reinterpret_cast<StXY*>(wl + 64 * (sizeof(StS1) + sizeof(StS3) + sizeof(StO3) + sizeof(StXY)));
    StC* __restrict__ cr = reinterpret_cast<StC*>(wl + 64 * (sizeof(StS1) + sizeof(StS3) + sizeof(StO3) + 2 * sizeof(StXY)));
    const unsigned int count = *qcount;
    const int T = cfg.horizon, R = cfg.n_rollouts;
    const DynConst k = dyn_const(cfg);
    const unsigned int nw = gridDim.x * (blockDim.x >> 6);
    for (unsigned int i = blockIdx.x * (blockDim.x >> 6) + wave; i < count; i += nw) {   // wave-uniform
        F1P_STPH();
        const StItem it = items[i];
        const int e = it.es / F1P_ST_MAX_REFINE;
        const int t = lane;
        const bool act = t < T, act1 = t <= T;
        st_ego_t<Ctl> cp;                                                 // [t][2][R], or regenerated: step t of rollout r is a pure function of (e, r, t)
        if constexpr (st_gen<Ctl>) cp = StGenSrc{ctl.src(e, ctl.warm_row(e)), 0.0f}; else cp = ctl + (size_t)e * T * 2 * R + it.r;
        const double* sref = ref + (size_t)e * 7 * (T + 1);
        float c_dv, c_a;
        if constexpr (st_gen<Ctl>) { c_dv = act ? cp.dv(t, it.r) : 0.0f; c_a = act ? cp.a() : 0.0f; }
        else { c_dv = act ? cp[(size_t)t * 2 * R] : 0.0f; c_a = act ? cp[(size_t)t * 2 * R + R] : 0.0f; }
        double rf[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) rf[j] = act1 ? sref[j * (T + 1) + t] : 0.0;
        DynState s0;
        s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
        s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
        // ---- 1. controls: the bounds in parallel, the rate clamp and the two clamped running sums in sequence ----------------------
        const double my_a = clampd2((double)c_a, -cfg.max_accel, cfg.max_accel);         // :704-706
        {
            StS1 w1; w1.u = clampd2((double)c_dv, -cfg.max_steer_v, cfg.max_steer_v); w1.a = my_a;   // :701-703
            s1[t] = w1;
        }
        wave_lds_sync();
        F1P_STPH();
        double my_dv = 0.0, my_delta = 0.0, my_v = 0.0;
        {
            double dlt = s0.delta, v = s0.v, pdv = 0.0;
#pragma unroll 4
            for (int q = 0; q < T; ++q) {
                const StS1 cur = s1[q];
                double dv = cur.u;
                if (q > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);   // :685
                if (lane == 0) { StO3 w; w.yr = dv; w.beta = dlt; w.yaw = v; w.pad = 0.0; o3[q] = w; }   // (o3 is free until phase 3: one LDS write instead of six selects)
                const double delta_new = dlt + dv * cfg.dt;               // :360
                const double v_new = v + cur.a * cfg.dt;                  // :361
                v = v_new > cfg.max_speed ? cfg.max_speed : (v_new < cfg.min_speed ? cfg.min_speed : v_new);               // :393-396
                dlt = delta_new >= cfg.max_steer ? cfg.max_steer : (delta_new <= -cfg.max_steer ? -cfg.max_steer : delta_new);   // :399-402
                pdv = dv;
            }
            if (lane == 0) { StO3 w; w.yr = 0.0; w.beta = dlt; w.yaw = v; w.pad = 0.0; o3[T] = w; }
        }
        wave_lds_sync();
        if (act1) { const StO3 w = o3[t]; my_dv = w.yr; my_delta = w.beta; my_v = w.yaw; }
        wave_lds_sync();
        F1P_STPH();
        // ---- 2. per step: coefficients of the (yr, beta) recurrence and the yaw increment ----------------------------------------
        if (act) {
            const double Tz = k.gl_r - (my_a * k.h);                      // :343
            const double Vz = k.gl_f + (my_a * k.h);                      // :344
            const double A1 = k.K * k.F * Tz;                             // :350-355
            const double A2 = k.K * (k.R * Vz - k.F * Tz);
            const double A3 = k.K * (k.lf2cf * Tz + k.lr2cr * Vz);
            const double A4 = k.M * Tz;
            const double A5 = k.N * Vz + k.M * Tz;
            const double A6 = k.N * Vz * k.l_r - k.M * Tz * k.l_f;
            double sd, cd;
            sincos_core(my_delta, &sd, &cd);
            const double tn = sd / cd;
            StS3 w3;
            w3.P1 = A1 * my_delta; w3.A2 = A2; w3.A3 = A3; w3.A4d = A4 * (my_delta / my_v); w3.A5 = A5; w3.A6 = A6;
            w3.v = my_v; w3.vv = my_v * my_v; w3.w = my_v / cfg.wheelbase * tn * cfg.dt; w3.pad = 0.0;
            s3[t] = w3;
        }
        wave_lds_sync();
        F1P_STPH();
        // ---- 3. the recurrence: yr, beta (and yaw's running sum beside them) ------------------------------------------------------
        {
            double yr = s0.yr, beta = s0.beta, yaw = s0.yaw;
#pragma unroll 4
            for (int q = 0; q < T; ++q) {
                const StS3 cur = s3[q];
                if (lane == 0) { StO3 w; w.yr = yr; w.beta = beta; w.yaw = yaw; w.pad = 0.0; o3[q] = w; }
                const double yr_new = yr + (cur.P1 + cur.A2 * beta - cur.A3 * (yr / cur.v)) * cfg.dt;                       // :367-371
                const double beta_new = beta + (cur.A4d - cur.A5 * (beta / cur.v) + cur.A6 * (yr / cur.vv) - yr) * cfg.dt;   // :372-381
                yaw = yaw + cur.w;                                                                                          // :362-365
                yr = yr_new; beta = beta_new;
            }
            if (lane == 0) { StO3 w; w.yr = yr; w.beta = beta; w.yaw = yaw; w.pad = 0.0; o3[T] = w; }
        }
        wave_lds_sync();
        F1P_STPH();
        double my_yr = 0.0, my_beta = 0.0, my_yaw = 0.0;
        if (act1) { const StO3 w = o3[t]; my_yr = w.yr; my_beta = w.beta; my_yaw = w.yaw; }
        // ---- 4. x / y increments --------------------------------------------------------------------------------------------------
        if (act) {
            double sn, cs;
            sincos_fast(my_yaw + my_beta, &sn, &cs);
            StXY w; w.x = my_v * cs * cfg.dt; w.y = my_v * sn * cfg.dt;   // :358-359
            s6[t] = w;
        }
        wave_lds_sync();
        F1P_STPH();
        // ---- 5. x, y ---------------------------------------------------------------------------------------------------------------
        {
            double x = s0.x, y = s0.y;
#pragma unroll 8
            for (int q = 0; q < T; ++q) {
                const StXY cur = s6[q];
                if (lane == 0) { StXY w; w.x = x; w.y = y; o6[q] = w; }
                x = x + cur.x; y = y + cur.y;
            }
            if (lane == 0) { StXY w; w.x = x; w.y = y; o6[T] = w; }
        }
        wave_lds_sync();
        F1P_STPH();
        // ---- 5b. lane t tests the points of step t -> t + 1 (x_t, y_t are stmpc_rollouts' own values); a ballot ORs the verdicts --------
        [[maybe_unused]] bool blocked = false;
        if constexpr (has_col<Col...>) {
            bool hit = false;
            if constexpr (has_obs<Col...>) {                              // ego e's table, at wave-uniform addresses; lane t has the step's own t
                if (act) { const StXY p = o6[t], q = o6[t + 1]; hit = col_seg(st_obs_of_ego(col_of(col...), e), t, cfg.dt, p.x, p.y, q.x, q.y); }
            } else
            if (act) { const StXY p = o6[t], q = o6[t + 1]; hit = col_of(col...).seg(p.x, p.y, q.x, q.y); }
            blocked = __ballot(hit) != 0ull;
        }
        // ---- 6. cost rows ----------------------------------------------------------------------------------------------------------
        {
            const double p_dv = shfl_d(my_dv, lane > 0 ? lane - 1 : 0), p_a = shfl_d(my_a, lane > 0 ? lane - 1 : 0);
            StC w; w.q = 0.0; w.r = 0.0; w.rd = 0.0; w.pad = 0.0;
            if (act1) {
                const StXY xy = o6[t];
                const double sv[7] = {xy.x, xy.y, my_delta, my_v, my_yaw, my_yr, my_beta};
                double q = 0.0;
                if (act) {
#pragma unroll
                    for (int j = 0; j < 7; ++j) { const double er = sv[j] - rf[j]; q += cfg.q[j] * er * er; }    // :619
                    w.r = cfg.r[0] * my_dv * my_dv + cfg.r[1] * my_a * my_a;                                     // :616
                    if (t > 0) { const double d0 = my_dv - p_dv, d1 = my_a - p_a; w.rd = cfg.rd[0] * d0 * d0 + cfg.rd[1] * d1 * d1; }   // :622
                } else {
#pragma unroll
                    for (int j = 0; j < 7; ++j) { const double er = sv[j] - rf[j]; q += cfg.qf[j] * er * er; }
                }
                w.q = q;
                cr[t] = w;
            }
        }
        wave_lds_sync();
        F1P_STPH();
        // ---- 7. the running sum, in stmpc_rollouts' order ---------------------------------------------------------------------------
        {
            double cost = 0.0;
#pragma unroll 8
            for (int q = 0; q < T; ++q) {
                const StC cur = cr[q];
                cost += cur.q;
                cost += cur.r;
                if (q > 0) cost += cur.rd;
            }
            cost += cr[T].q;                                              // the terminal row (Qf)
            if constexpr (has_col<Col...>) { if (lane == 0) { rc[it.es] = blocked ? __builtin_huge_val() : cost; if (blocked) col_of(col...).rl[it.es] = F1P_K4_NONE; } }
            else if (lane == 0) rc[it.es] = cost;
        }
        wave_lds_sync();
#ifdef F1P_ST_PHASES
        F1P_STPH();
        if (dbg_ticks && lane == 0 && i < 4096u) { for (int q = 0; q + 1 < nph; ++q) dbg_ticks[i * 16u + q] = (float)(ph[q + 1] - ph[q]); dbg_ticks[i * 16u + 15] = (float)nph; }
        nph = 0;
#endif
    }
}

// ---- K-C: np.argmin's rule over the refined costs (or the all-fp64 loop for the egos the filter gave up on), outputs -------------
template <typename Ctl, typename... Col>
__global__ __launch_bounds__(256) void k_stmpc_decide_t(const double* __restrict__ x0, const double* __restrict__ ref,
                                                      Ctl ctl, int E, f1p_stmpc_cfg cfg,
                                                      unsigned int* __restrict__ qcount, const int32_t* __restrict__ nlist, const int32_t* __restrict__ rl,
                                                      const double* __restrict__ rc, Col... col,
                                                      double* __restrict__ steer, double* __restrict__ speed,
                                                      int32_t* __restrict__ best_idx, double* __restrict__ best_cost,
                                                      double* __restrict__ best_seq, int32_t* __restrict__ dbg_nref) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int T = cfg.horizon, R = cfg.n_rollouts, tid = threadIdx.x;
    double* sref = reinterpret_cast<double*>(lds_raw);                // [7][T+1] (fallback only)
    double* red_d = sref + 7 * (T + 1);                               // [4]
    int* red_i = reinterpret_cast<int*>(red_d + 4);                   // [4]
    const int e = blockIdx.x;
    if (e >= E) return;
    if (e == 0 && tid == 0) *qcount = 0u;                             // re-arm the queue for the next plan (k_stmpc_refine has finished)
    int n = nlist[e];
    DynState s0;
    s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
    s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
    st_ego_t<Ctl> ce;
    if constexpr (st_gen<Ctl>) ce = StGenSrc{ctl.src(e, ctl.warm_row(e)), 0.0f}; else ce = ctl + (size_t)e * T * 2 * R;
    double bc = __builtin_huge_val(); int bi = 0x7fffffff;
    [[maybe_unused]] double* olive = nullptr;
    [[maybe_unused]] int* on2 = nullptr;
    if constexpr (has_obs<Col...>) {                                  // the ego's live discs -> LDS (the all-fp64 loop's), behind the reduction's words
        olive = reinterpret_cast<double*>(red_i + 4);
        on2 = reinterpret_cast<int*>(olive + 5 * F1P_KMPC_MAX_OBS);
        if (n < 0 && tid < 64) st_obs_setup(col_of(col...), e, s0.x, s0.y, s0.v, s0.yaw, T, olive, nullptr, on2);
    }
    if constexpr (has_col<Col...>) {
        if (n >= 0) {                                                 // a blocked item is (+inf, F1P_K4_NONE): it loses to every unblocked one
            if (tid < n) {
                bc = rc[(size_t)e * F1P_ST_MAX_REFINE + tid];
                bi = rl[(size_t)e * F1P_ST_MAX_REFINE + tid];
            }
            block_argmin(bc, bi, red_d, red_i);
            // every listed rollout blocked: the list holds the FREE minimum, which the position bound proves unblocked, so this is not expected --
            // the ego is decided by the all-fp64 loop rather than declared blocked on the filter's word (workgroup-uniform)
            if (bi == F1P_K4_NONE) {
                n = -1; bc = __builtin_huge_val(); __syncthreads();
                if constexpr (has_obs<Col...>) { if (tid < 64) st_obs_setup(col_of(col...), e, s0.x, s0.y, s0.v, s0.yaw, T, olive, nullptr, on2); }
            }
        }
    }
    if (n < 0) {                                                      // workgroup-uniform
        for (int q = tid; q < 7 * (T + 1); q += blockDim.x) sref[q] = ref[(size_t)e * 7 * (T + 1) + q];
        __syncthreads();
        const DynConst k = dyn_const(cfg);
        if constexpr (has_obs<Col...>) {                              // (the barrier above is behind st_obs_setup)
            auto ob = col_of(col...);
            st_obs_bind(ob, olive, on2);
            if (fabs(cfg.max_steer) <= 1.0e4) stmpc_rollouts<true, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, ob);
            else stmpc_rollouts<false, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, ob);
        } else
        if (fabs(cfg.max_steer) <= 1.0e4) stmpc_rollouts<true, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, col...);
        else stmpc_rollouts<false, Ctl>(ce, sref, cfg, k, s0, tid, bc, bi, col...);
        if constexpr (has_col<Col...>) block_argmin(bc, bi, red_d, red_i);
    } else if constexpr (!has_col<Col...>) {
        if (tid < n) {
            bc = rc[(size_t)e * F1P_ST_MAX_REFINE + tid];
            bi = rl[(size_t)e * F1P_ST_MAX_REFINE + tid];
        }
    }
    if constexpr (has_col<Col...>) {
        if (bi == F1P_K4_NONE) {                                      // every rollout blocked (workgroup-uniform): the lattice's ALL_BLOCKED outputs
            for (int q = tid; q < 2 * T; q += blockDim.x) {
                if (best_seq) best_seq[(size_t)e * T * 2 + q] = 0.0;
                if constexpr (st_gen<Ctl>) ctl.warm_row(e)[q] = 0.0f;
            }
            if (tid == 0) {
                steer[e] = 0.0; speed[e] = 0.0; best_idx[e] = -1;
                if (best_cost) best_cost[e] = __builtin_huge_val();
                if (dbg_nref) dbg_nref[e] = n;
            }
            return;
        }
    } else {
        block_argmin(bc, bi, red_d, red_i);
    }
    [[maybe_unused]] float* emit_s = reinterpret_cast<float*>(lds_raw);
    if constexpr (st_gen<Ctl>) {
        for (int t_ = tid; t_ < T; t_ += blockDim.x) ce.g.get(t_, bi, emit_s[2 * t_], emit_s[2 * t_ + 1]);
        __syncthreads();
    }
    if (tid == 0) {
        double pdv = 0.0;
        for (int t = 0; t < T; ++t) {
            float c;
            if constexpr (st_gen<Ctl>) c = emit_s[2 * t]; else c = ce[((size_t)t * 2 + 0) * R + bi];
            double dv = clampd2((double)c, -cfg.max_steer_v, cfg.max_steer_v);
            if constexpr (st_gen<Ctl>) c = emit_s[2 * t + 1]; else c = ce[((size_t)t * 2 + 1) * R + bi];
            const double a = clampd2((double)c, -cfg.max_accel, cfg.max_accel);
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
            if (t == 0) {
                steer[e] = s0.delta + dv * cfg.dt;   // :1112
                speed[e] = s0.v + a * cfg.dt;        // :1117
            }
            if (best_seq) { best_seq[((size_t)e * T + t) * 2] = dv; best_seq[((size_t)e * T + t) * 2 + 1] = a; }
            else if constexpr (!st_gen<Ctl>) { if (t == 0) break; }
            if constexpr (st_gen<Ctl>) {
                float* wo_ = ctl.warm_row(e);
                if (t > 0) { wo_[2 * (t - 1)] = (float)dv; wo_[2 * (t - 1) + 1] = (float)a; }
                if (t == T - 1) { wo_[2 * t] = (float)dv; wo_[2 * t + 1] = (float)a; }
            }
            pdv = dv;
        }
        best_idx[e] = bi;
        if (best_cost) best_cost[e] = bc;
        if (dbg_nref) dbg_nref[e] = n;
    }
}

// the kernels under the names their launches, the profiles and bench.py's labels know them by: streamed controls (f1p_stmpc_shoot_*),
// generated controls (_gen: f1p_stmpc_plan_*), and with the occupancy test (_col).  (The launches below go through the templates: one helper per
// schedule over the source and the test.)
[[maybe_unused]] static constexpr auto k_stmpc_shoot = k_stmpc_shoot_t<StCtlStream>;
[[maybe_unused]] static constexpr auto k_stmpc_shoot_gen = k_stmpc_shoot_t<StCtlGen>;
[[maybe_unused]] static constexpr auto k_stmpc_shoot_col = k_stmpc_shoot_t<StCtlStream, KmpcCol>;
[[maybe_unused]] static constexpr auto k_stmpc_shoot_gen_col = k_stmpc_shoot_t<StCtlGen, KmpcCol>;
template <int QM> [[maybe_unused]] static constexpr auto k_stmpc_filter = k_stmpc_filter_t<QM, StCtlStream>;
template <int QM> [[maybe_unused]] static constexpr auto k_stmpc_filter_gen = k_stmpc_filter_t<QM, StCtlGen>;
template <int QM> [[maybe_unused]] static constexpr auto k_stmpc_filter_gen_col = k_stmpc_filter_t<QM, StCtlGen, KmpcCol>;
[[maybe_unused]] static constexpr auto k_stmpc_refine = k_stmpc_refine_t<StCtlStream>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_gen = k_stmpc_refine_t<StCtlGen>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_gen_col = k_stmpc_refine_t<StCtlGen, StColRef>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_tp = k_stmpc_refine_tp_t<StCtlStream>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_tp_gen = k_stmpc_refine_tp_t<StCtlGen>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_tp_gen_col = k_stmpc_refine_tp_t<StCtlGen, StColRef>;
[[maybe_unused]] static constexpr auto k_stmpc_decide = k_stmpc_decide_t<StCtlStream>;
[[maybe_unused]] static constexpr auto k_stmpc_decide_gen = k_stmpc_decide_t<StCtlGen>;
[[maybe_unused]] static constexpr auto k_stmpc_decide_gen_col = k_stmpc_decide_t<StCtlGen, KmpcCol>;
// with the moving discs of f1p_stmpc_set_obstacles (_obs), alone or with the occupancy test (the bitmap of the KmpcCol part: null = no grid)
[[maybe_unused]] static constexpr auto k_stmpc_shoot_obs = k_stmpc_shoot_t<StCtlStream, StObs>;
[[maybe_unused]] static constexpr auto k_stmpc_shoot_gen_obs = k_stmpc_shoot_t<StCtlGen, StObs>;
template <int QM> [[maybe_unused]] static constexpr auto k_stmpc_filter_gen_obs = k_stmpc_filter_t<QM, StCtlGen, StObs>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_gen_obs = k_stmpc_refine_t<StCtlGen, StObsRef>;
[[maybe_unused]] static constexpr auto k_stmpc_refine_tp_gen_obs = k_stmpc_refine_tp_t<StCtlGen, StObsRef>;
[[maybe_unused]] static constexpr auto k_stmpc_decide_gen_obs = k_stmpc_decide_t<StCtlGen, StObs>;

// materialise the generator's controls as the [E][T][2][R] f32 buffer of the streamed entry points (tests: generated == streamed)
__global__ __launch_bounds__(256) void k_stmpc_gen_controls(float* __restrict__ controls, int E, int T, int R, StCtlGen ctl) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)E * T * R) return;
    const size_t et = i / R;
    const int r = (int)(i - et * R), e = (int)(et / T), t = (int)(et - (size_t)e * T);
    float dv, a;
    ctl.src(e, ctl.warm_row(e)).get(t, r, dv, a);
    controls[(et * 2 + 0) * R + r] = dv;
    controls[(et * 2 + 1) * R + r] = a;
}

// rows[k] (k < n) of the warm start <- 0: the egos that start over (no warm start yet, or the other branch's)
__global__ __launch_bounds__(256) void k_stmpc_warm_zero(float* __restrict__ warm, const int32_t* __restrict__ rows, int n, int wstride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * wstride) return;
    const size_t k = i / wstride;
    warm[(size_t)rows[k] * wstride + (i - k * wstride)] = 0.0f;
}


// calc_ref_trajectory :195-233; states [E][4] = (x, y, v, yaw); ref [E][7][T+1] rows x, y, 0, v, yaw, 0, 0
__global__ __launch_bounds__(256) void k_stmpc_ref(const double* __restrict__ states, int E, int T, double dt, double dl,
                                                   const double* __restrict__ wx, const double* __restrict__ wy,
                                                   const double* __restrict__ wv, const double* __restrict__ wpsi,
                                                  const double* __restrict__ wbox, int n,
                                                   double* __restrict__ ref) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int e = blockIdx.x;
    if (e >= E) return;
    const double px = states[4 * e], py = states[4 * e + 1], v = states[4 * e + 2], yaw = states[4 * e + 3];
    double bd; int ind;
    nearest_scan_boxed(px, py, wx, wy, wbox, n, threadIdx.x, blockDim.x, bd, ind);
    block_argmin(bd, ind, sd, si);
    const double dind = (fabs(v) * dt) / dl;
    double* r = ref + (size_t)e * 7 * (T + 1);
    for (int j = threadIdx.x; j <= T; j += blockDim.x) {
        double cum = 0.0;
        for (int q = 0; q < j; ++q) cum += dind;
        int il = ind + (int)cum;
        if (il >= n) il -= n;
        if (il < 0 || il >= n) il = il < 0 ? 0 : n - 1;
        double cyw = wpsi[il];
        if (cyw - yaw > 5) cyw = fabs(cyw - (2 * F1P_PI));      // :227
        if (cyw - yaw < -5) cyw = fabs(cyw + (2 * F1P_PI));     // :228
        r[0 * (T + 1) + j] = wx[il];
        r[1 * (T + 1) + j] = wy[il];
        r[2 * (T + 1) + j] = 0.0;
        r[3 * (T + 1) + j] = wv[il];
        r[4 * (T + 1) + j] = cyw;
        r[5 * (T + 1) + j] = 0.0;
        r[6 * (T + 1) + j] = 0.0;
    }
}

int launch_stmpc_predict(f1p_ctx* ctx, const double* d_x0, const double* d_oa, const double* d_od, int E, const f1p_stmpc_cfg* cfg, double* d_path) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_stmpc_predict, dim3((E + 255) / 256), dim3(256), 0, ctx->stream, d_x0, d_oa, d_od, E, *cfg, d_path);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_predict launch");
}

static DynF32 make_dyn_f32(const f1p_stmpc_cfg* cfg) {
    const double* p = cfg->params;
    const double mass = p[0], l_f = p[1], l_r = p[2], h_cog = p[3], c_f = p[4], c_r = p[5], iz = p[6], mu = p[7], g = 9.81;
    const double K = (mu * mass) / ((l_f + l_r) * iz), F = l_f * c_f, Rr = l_r * c_r, M = (mu * c_f) / (l_f + l_r), N = (mu * c_r) / (l_f + l_r);
    DynF32 k;
    const double dt = cfg->dt, glr = g * l_r, glf = g * l_f, h = h_cog;
    // A1 = K F T, A2 = K (R V - F T), A3 = K (lf^2 cf T + lr^2 cr V), A4 = M T, A5 = N V + M T, A6 = N V lr - M T lf;  T = glr - a h, V = glf + a h
    const double cT[6] = {K * F, -K * F, K * l_f * l_f * c_f, M, M, -M * l_f}, cV[6] = {0.0, K * Rr, K * l_r * l_r * c_r, 0.0, N, N * l_r};
    for (int i = 0; i < 6; ++i) { k.ap[i] = (float)(dt * (cT[i] * glr + cV[i] * glf)); k.aq[i] = (float)(dt * h * (cV[i] - cT[i])); }
    k.dt = (float)dt; k.dt_inv_wb = (float)(dt / cfg->wheelbase);
    k.c0 = 1.f; k.s0 = 0.f;
    k.max_steer = (float)cfg->max_steer; k.max_steer_v = (float)cfg->max_steer_v; k.max_accel = (float)cfg->max_accel;
    k.max_speed = (float)cfg->max_speed; k.min_speed = (float)cfg->min_speed;
    // trust speed: both Euler modes contractive with margin (|1 - dt A3 / v| and |1 - dt A5 / v| <= 0.9 ...) for |a| <= max_accel
    const double am = fabs(cfg->max_accel) * h_cog;
    const double A3max = K * (l_f * l_f * c_f * (g * l_r + am) + l_r * l_r * c_r * (g * l_f + am));
    const double A5max = N * (g * l_f + am) + M * (g * l_r + am);
    k.v_trust = (float)(1.05 * cfg->dt * fmax(A3max, 2.0 * A5max) / 1.8);
    for (int j = 0; j < 7; ++j) { k.q[j] = (float)cfg->q[j]; k.qf[j] = (float)cfg->qf[j]; }
    for (int j = 0; j < 2; ++j) { k.r[j] = (float)cfg->r[j]; k.rd[j] = (float)cfg->rd[j]; }
    return k;
}

// the mixed schedule's scratch for E egos: queue counter (256 B) | nlist [E] | rl [E][64] | items [E][64] | rc [E][64]; the queue counter is
// zeroed when the scratch is new or a plan failed between its kernels, and st_q_dirty stays set until the caller's last launch succeeded
// | the discs' tables otab [E][16][5] fp64 | their counts ontab [E] (the filter writes them for the refinement while obstacles are set)
struct StScratch { unsigned int* qcount; int32_t *nlist, *rl; StItem* items; double* rc; double* otab; int32_t* ontab; };
static int st_scratch(f1p_ctx* ctx, int E, StScratch& sc) {
    const size_t n_off = 256, rl_off = (n_off + 4 * (size_t)E + 255) & ~(size_t)255;
    const size_t it_off = (rl_off + 4 * (size_t)E * F1P_ST_MAX_REFINE + 255) & ~(size_t)255;
    const size_t rc_off = (it_off + sizeof(StItem) * (size_t)E * F1P_ST_MAX_REFINE + 255) & ~(size_t)255;
    const size_t ot_off = (rc_off + 8 * (size_t)E * F1P_ST_MAX_REFINE + 255) & ~(size_t)255;
    const size_t on_off = (ot_off + sizeof(double) * 5 * F1P_KMPC_MAX_OBS * (size_t)E + 255) & ~(size_t)255;
    const size_t need = on_off + 4 * (size_t)E;
    if (need > ctx->st_scratch_bytes) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_st_scratch) (void)hipFree(ctx->d_st_scratch);
        ctx->d_st_scratch = nullptr; ctx->st_scratch_bytes = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_st_scratch, need));
        ctx->st_scratch_bytes = need;
        ctx->st_q_dirty = true;
    }
    sc.qcount = reinterpret_cast<unsigned int*>(ctx->d_st_scratch);
    sc.nlist = reinterpret_cast<int32_t*>(ctx->d_st_scratch + n_off);
    sc.rl = reinterpret_cast<int32_t*>(ctx->d_st_scratch + rl_off);
    sc.items = reinterpret_cast<StItem*>(ctx->d_st_scratch + it_off);
    sc.rc = reinterpret_cast<double*>(ctx->d_st_scratch + rc_off);
    sc.otab = reinterpret_cast<double*>(ctx->d_st_scratch + ot_off);
    sc.ontab = reinterpret_cast<int32_t*>(ctx->d_st_scratch + on_off);
    if (ctx->st_q_dirty) F1P_HIP(ctx, hipMemsetAsync(sc.qcount, 0, 256, ctx->stream));
    ctx->st_q_dirty = true;
    return F1P_OK;
}

// Bound on the f32 filter's position error against the fp64 rollout over the horizon [m], for a TRUSTED rollout (only those can be FREE);
// DESIGN.md 5i derives the terms.  u = 2^-24.
static double st_pos_err_bound(const f1p_stmpc_cfg* cfg) {
    const double u = 5.9604644775390625e-8, T = cfg->horizon;
    const double vmax = fmax(fabs(cfg->max_speed), fabs(cfg->min_speed)), reach = vmax * T * cfg->dt;
    const double yr_max = vmax / cfg->wheelbase * tan(fmin(fabs(cfg->max_steer), 1.4));   // steady-state yaw rate at full lock
    const double yaw_max = yr_max * T * cfg->dt;                                           // the relative heading's range
    // heading = yaw + beta.  yaw: T accumulations, each rounding u (|yaw| + its increment), + the tan polynomial's 2.5e-7 relative on the
    // increments; (yr, beta): per-step roundings 8 u max(yr_max, 1) through a contraction of factor <= 0.9 (the trust speed) = x 10;
    // the hardware sin / cos: 1e-6 absolute
    const double dth = T * u * (yaw_max + 1.0) + 2.5e-7 * yaw_max + 80.0 * u * fmax(yr_max, 1.0) + 1.0e-6;
    // positions: the heading error at the reach; T accumulations of u |x|; the increments' 2 u + 1e-6; the speed's T u over the horizon;
    // the interpolation, the ego-cell offset and the cell conversion 4 u
    return reach * (dth + T * u + 2.0 * u + 1.0e-6 + T * u + 4.0 * u);
}
#define F1P_ST_POS_HEADROOM 5.0        // the filter gets the clearance map only while headroom x bound < one cell (DESIGN.md 5h's factor)

// the refinement kernels' form of the test, and the scratch the obstacle test keeps its tables in
static StColRef st_ref(const KmpcCol& c, int32_t* rl) { return StColRef{c, rl}; }
static StObsRef st_ref(const StObs& c, int32_t* rl) { return StObsRef{c, rl}; }
static void st_bind_scratch(KmpcCol&, const StScratch&) {}
static void st_bind_scratch(StObs& o, const StScratch& sc) { o.tab = sc.otab; o.ntab = sc.ontab; }
template <typename... Col> static const char* st_what(const char* plain, const char* col, const char* obs) {
    if constexpr (has_obs<Col...>) return obs; else if constexpr (sizeof...(Col) > 0) return col; else return plain;
}

// the mixed schedule, filter -> refinement -> decision, over the control source and the optional occupancy test
template <typename Ctl, typename... Col>
static int stmpc_mixed(f1p_ctx* ctx, const double* d_x0, const double* d_ref, Ctl ctl, int E, const f1p_stmpc_cfg* cfg, const DynF32& kf, size_t lds_a, size_t lds_c,
                       double* d_steer, double* d_speed, int32_t* d_best_idx, double* d_best_cost, double* d_best_seq, Col... col) {
    constexpr bool COL = sizeof...(Col) > 0;                         // (the error strings name the kernels as they always did)
    StScratch sc;
    if (const int rs = st_scratch(ctx, E, sc)) return rs;
    (st_bind_scratch(col, sc), ...);
    int qm = 0;                                                      // rows that carry weight in the stage or the terminal cost
    for (int j = 0; j < 7; ++j) if (cfg->q[j] != 0.0 || cfg->qf[j] != 0.0) qm |= 1 << j;
    // 0x1b: the reference's weights (x, y, v, yaw): the delta / yr / beta terms are not evaluated
    hipLaunchKernelGGL(qm == 0x1b ? (k_stmpc_filter_t<0x1b, Ctl, Col...>) : (k_stmpc_filter_t<0x7f, Ctl, Col...>), dim3(E), dim3(256), (lds_a + 15) & ~(size_t)15,
                       ctx->stream, d_x0, d_ref, ctl, E, cfg->horizon, cfg->n_rollouts, cfg->max_steer, kf, col..., sc.qcount, sc.items, sc.nlist, sc.rl, ctx->d_dbg_st_cost32);
    int rcode = check_hip(ctx, hipGetLastError(), st_what<Col...>("k_stmpc_filter launch", "k_stmpc_filter_gen_col launch", "k_stmpc_filter_gen_obs launch"));
    if (rcode != F1P_OK) return rcode;
    if (cfg->horizon <= 63 && 4 * F1P_ST_TP_LDS_PER_WAVE <= (size_t)ctx->prop.sharedMemPerBlock) {
        const int nb = E * F1P_ST_MAX_REFINE / 4 < 2 * ctx->prop.multiProcessorCount ? (E * F1P_ST_MAX_REFINE + 3) / 4 : 2 * ctx->prop.multiProcessorCount;
        hipLaunchKernelGGL((k_stmpc_refine_tp_t<Ctl, decltype(st_ref(col, sc.rl))...>), dim3(nb), dim3(256), 4 * F1P_ST_TP_LDS_PER_WAVE, ctx->stream, d_x0, d_ref, ctl,
                           *cfg, sc.qcount, sc.items, st_ref(col, sc.rl)..., sc.rc, COL ? (float*)nullptr : ctx->d_dbg_st_cost32);
    } else {
        hipLaunchKernelGGL((k_stmpc_refine_t<Ctl, decltype(st_ref(col, sc.rl))...>), dim3(E), dim3(64), 0, ctx->stream, d_x0, d_ref, ctl, *cfg, sc.qcount, sc.items,
                           st_ref(col, sc.rl)..., sc.rc);
    }
    rcode = check_hip(ctx, hipGetLastError(), st_what<Col...>("k_stmpc_refine launch", "k_stmpc_refine_gen_col launch", "k_stmpc_refine_gen_obs launch"));
    if (rcode != F1P_OK) return rcode;
    hipLaunchKernelGGL((k_stmpc_decide_t<Ctl, Col...>), dim3(E), dim3(256), (lds_c + 15) & ~(size_t)15, ctx->stream, d_x0, d_ref, ctl, E, *cfg, sc.qcount,
                       sc.nlist, sc.rl, sc.rc, col..., d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq, ctx->d_dbg_st_nref);
    rcode = check_hip(ctx, hipGetLastError(), st_what<Col...>("k_stmpc_decide launch", "k_stmpc_decide_gen_col launch", "k_stmpc_decide_gen_obs launch"));
    if (rcode == F1P_OK) ctx->st_q_dirty = false;
    return rcode;
}

// the schedule of f1p_stmpc_shoot_* (gen == nullptr: streamed d_controls) and of f1p_stmpc_plan_* (gen: generated controls, d_controls unused)
static int stmpc_shoot_any(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, const StCtlGen* gen, int E, const f1p_stmpc_cfg* cfg,
                           double* d_steer, double* d_speed, int32_t* d_best_idx, double* d_best_cost, double* d_best_seq) {
    if (E <= 0) return F1P_OK;
    const size_t T1 = (size_t)cfg->horizon + 1;
    const bool discs = ctx->stmpc_obs.cur != nullptr;                      // f1p_stmpc_set_obstacles (the caller checked E: stmpc_collision_check)
    const size_t lds = sizeof(double) * (7 * T1 + 4) + sizeof(int) * 4 + (discs ? F1P_ST_OBS_LDS64 : 0);   // the plain-fp64 kernel's, and the decision's
    // the plain-fp64 evaluation, over the control source and the optional occupancy test
    auto shoot = [&](const char* what, auto... col) {
        if (gen) hipLaunchKernelGGL((k_stmpc_shoot_t<StCtlGen, decltype(col)...>), dim3(E), dim3(256), (lds + 15) & ~(size_t)15, ctx->stream, d_x0, d_ref, *gen, E, *cfg, col...,
                                    d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
        else hipLaunchKernelGGL((k_stmpc_shoot_t<StCtlStream, decltype(col)...>), dim3(E), dim3(256), (lds + 15) & ~(size_t)15, ctx->stream, d_x0, d_ref, d_controls, E, *cfg, col...,
                                d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
        return check_hip(ctx, hipGetLastError(), what);
    };
    if (discs) {
        // the moving discs, with the occupancy test (a bitmap) or without (null).  Streamed controls: plain fp64 in every mode, as with the grid.
        // Generated controls in the mixed mode: filter -> refinement -> decision; with the grid under the occupancy test's own guard (the
        // position bound below one cell and a clearance map), without one no cell guard applies -- the discs' FREE threshold carries the bound.
        StObs ob;
        ob.g = ctx->stmpc_collision ? grid_dev(ctx) : GridDev{nullptr, 0, 0, 0, 0.0, 0.0, 0.0};
        ob.clear = nullptr; ob.n_sub = ctx->stmpc_col_nsub; ob.force64 = 1;
        ob.obs = ctx->stmpc_obs.cur; ob.M = ctx->stmpc_obs.M; ob.live = nullptr; ob.n_live = 0;
        ob.dt = cfg->dt; ob.max_speed = cfg->max_speed; ob.min_speed = cfg->min_speed; ob.pos_err = st_pos_err_bound(cfg);
        ob.ids = gen ? gen->ids : nullptr; ob.tab = nullptr; ob.ntab = nullptr; ob.nan_all = 0;
        if (lds > (size_t)ctx->prop.sharedMemPerBlock) return set_error(ctx, F1P_EINVAL, "stmpc: the horizon needs more LDS than a workgroup has");
        if (gen && ctx->stmpc_mixed && !ctx->stmpc_warm_nonfinite) {
            const DynF32 kf = make_dyn_f32(cfg);
            const size_t lds_a = sizeof(float) * (8 * T1 + (size_t)cfg->n_rollouts + 4) + sizeof(int) * (F1P_ST_MAX_REFINE + 2) + sizeof(float) * 2 * (size_t)cfg->horizon +
                                 F1P_ST_OBS_LDS32;
            if (lds_a <= (size_t)ctx->prop.sharedMemPerBlock && kf.v_trust == kf.v_trust && (size_t)E * F1P_ST_MAX_REFINE < ((size_t)1 << 31) &&
                (!ctx->stmpc_collision || (F1P_ST_POS_HEADROOM * st_pos_err_bound(cfg) * ctx->inv_res < 1.0 && ensure_clear_map(ctx, F1P_K4_CLEAR_CELLS) == F1P_OK))) {
                if (ctx->stmpc_collision) ob.clear = ctx->d_bits_clear;
                ob.force64 = 0;
                return stmpc_mixed(ctx, d_x0, d_ref, *gen, E, cfg, kf, lds_a, lds, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq, ob);
            }
        }
        return shoot("k_stmpc_shoot_obs launch", ob);
    }
    if (ctx->stmpc_collision) {
        // the occupancy test (the caller checked the grid: stmpc_collision_check).  Streamed controls: plain fp64 in every mode, so that
        // gen_controls + shoot == plan bit for bit.  Generated controls in the mixed mode: filter -> refinement -> decision with the test, as
        // long as the f32 position bound (with its headroom) stays below one cell and the clearance map can be built; otherwise plain fp64.
        KmpcCol col;
        col.g = grid_dev(ctx); col.clear = nullptr; col.n_sub = ctx->stmpc_col_nsub; col.force64 = 1;
        if (lds > (size_t)ctx->prop.sharedMemPerBlock) return set_error(ctx, F1P_EINVAL, "stmpc: the horizon needs more LDS than a workgroup has");
        if (gen && ctx->stmpc_mixed && !ctx->stmpc_warm_nonfinite) {
            const DynF32 kf = make_dyn_f32(cfg);
            const size_t lds_a = sizeof(float) * (8 * T1 + (size_t)cfg->n_rollouts + 4) + sizeof(int) * (F1P_ST_MAX_REFINE + 2) + sizeof(float) * 2 * (size_t)cfg->horizon;
            if (lds_a <= (size_t)ctx->prop.sharedMemPerBlock && kf.v_trust == kf.v_trust && (size_t)E * F1P_ST_MAX_REFINE < ((size_t)1 << 31) &&
                F1P_ST_POS_HEADROOM * st_pos_err_bound(cfg) * ctx->inv_res < 1.0 && ensure_clear_map(ctx, F1P_K4_CLEAR_CELLS) == F1P_OK) {
                col.clear = ctx->d_bits_clear; col.force64 = 0;
                return stmpc_mixed(ctx, d_x0, d_ref, *gen, E, cfg, kf, lds_a, lds, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq, col);
            }
        }
        return shoot("k_stmpc_shoot_col launch", col);
    }
    if (ctx->stmpc_mixed && !(gen && ctx->stmpc_warm_nonfinite)) {      // (NaN controls: a warm start set with a non-finite entry -> plain fp64)
        const DynF32 kf = make_dyn_f32(cfg);
        const size_t lds_a = sizeof(float) * (8 * T1 + (size_t)cfg->n_rollouts + 4) + sizeof(int) * (F1P_ST_MAX_REFINE + 2) +
                             (gen ? sizeof(float) * 2 * (size_t)cfg->horizon : 0);   // + the ego's warm start
        if (lds_a <= (size_t)ctx->prop.sharedMemPerBlock && lds <= (size_t)ctx->prop.sharedMemPerBlock && kf.v_trust == kf.v_trust &&
            (size_t)E * F1P_ST_MAX_REFINE < ((size_t)1 << 31))
            return gen ? stmpc_mixed(ctx, d_x0, d_ref, *gen, E, cfg, kf, lds_a, lds, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq)
                       : stmpc_mixed<StCtlStream>(ctx, d_x0, d_ref, d_controls, E, cfg, kf, lds_a, lds, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
    }
    return shoot("k_stmpc_shoot launch");
}

int launch_stmpc_shoot(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, int E, const f1p_stmpc_cfg* cfg,
                       double* d_steer, double* d_speed, int32_t* d_best_idx, double* d_best_cost, double* d_best_seq) {
    return stmpc_shoot_any(ctx, d_x0, d_ref, d_controls, nullptr, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
}

static StCtlGen make_st_gen(const f1p_stmpc_sampler* smp, float* d_warm, int wstride, const int32_t* d_ids) {
    StCtlGen g;
    g.k0 = (uint32_t)(smp->seed & 0xffffffffull); g.k1 = (uint32_t)(smp->seed >> 32); g.call = smp->call; g.ego_off = (uint32_t)smp->ego_offset;
    g.sig_dv = (float)smp->sigma_steer_v; g.sig_a = (float)smp->sigma_accel;
    g.warm = d_warm; g.ids = d_ids; g.wstride = wstride;
    return g;
}

// d_warm: rows of wstride floats, read as this plan's warm start (all zero = none) and overwritten with the next one
int launch_stmpc_plan_gen(f1p_ctx* ctx, const double* d_x0, const double* d_ref, int E, const f1p_stmpc_cfg* cfg, const f1p_stmpc_sampler* smp,
                          float* d_warm, int wstride, const int32_t* d_ids, double* d_steer, double* d_speed, int32_t* d_best_idx,
                          double* d_best_cost, double* d_best_seq) {
    const StCtlGen g = make_st_gen(smp, d_warm, wstride, d_ids);
    return stmpc_shoot_any(ctx, d_x0, d_ref, nullptr, &g, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
}

int launch_stmpc_gen_controls(f1p_ctx* ctx, float* d_controls, int E, const f1p_stmpc_cfg* cfg, const f1p_stmpc_sampler* smp, float* d_warm, int wstride) {
    const size_t n = (size_t)E * cfg->horizon * cfg->n_rollouts;
    if (n == 0) return F1P_OK;
    hipLaunchKernelGGL(k_stmpc_gen_controls, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_controls, E, cfg->horizon, cfg->n_rollouts,
                       make_st_gen(smp, d_warm, wstride, nullptr));
    return check_hip(ctx, hipGetLastError(), "k_stmpc_gen_controls launch");
}

int launch_stmpc_warm_zero(f1p_ctx* ctx, float* d_warm, const int32_t* d_rows, int n, int wstride) {
    if (n <= 0) return F1P_OK;
    const size_t m = (size_t)n * wstride;
    hipLaunchKernelGGL(k_stmpc_warm_zero, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, d_warm, d_rows, n, wstride);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_warm_zero launch");
}

int launch_stmpc_ref(f1p_ctx* ctx, const double* d_states, int E, int horizon, double dt, double dl, double* d_ref) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_stmpc_ref, dim3(E), dim3(256), 0, ctx->stream, d_states, E, horizon, dt, dl, ctx->d_wx, ctx->d_wy, ctx->d_wv,
                       ctx->d_wpsi, ctx->d_wbox, ctx->n_wp, d_ref);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_ref launch");
}

}  // namespace f1p
