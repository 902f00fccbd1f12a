// k_stmpc_shoot_text.h -- the text of the dynamic single-track shooting kernels, included by k_stmpc.hip once per control source:
// streamed controls (k_stmpc_shoot / _filter / _refine / _refine_tp / _decide: f1p_stmpc_shoot_*) and generated controls (the same names
// with _gen: f1p_stmpc_plan_*).  A text compiled twice rather than templates over a source type: the streamed kernels' code objects
// stay what they were, instruction for instruction (the preprocessed tokens of the streamed inclusion are the ones this file's text had
// in k_stmpc.hip), which the optimiser does not promise for a __global__ wrapper around an inlined template body.
//   F1P_ST_N(name)              name, or name_gen
//   F1P_ST_CTL_PARAM            the kernels' control parameter            F1P_ST_SRC_PARAM   the per-ego source parameter `ce` of the device functions
//   F1P_ST_SRC_DECL(ce, e)      declares ego e's source                   F1P_ST_SRC_EXPR(e) ... as an expression
//   F1P_ST_SRC_DECL_FILTER      ... in the filter (the generated source reads its warm start from LDS: F1P_ST_FILTER_WARM fills it)
//   F1P_ST_SRC_DECL_R(cp, e, r) / F1P_ST_DV_R / F1P_ST_A_R   the time-parallel refinement's source of ONE rollout
//   F1P_ST_DV(ce, t, r) / F1P_ST_A(ce, t, r)   the two controls of step t of rollout r (f32); F1P_ST_A follows F1P_ST_DV of the same step
//                                              (the generated source makes one Philox call in the first and keeps the accel for the second)
//   F1P_ST_EMIT_PRE(ce, bi)     before the winner's re-emission (every thread, bi known to all): nothing for streamed controls; the generated
//                               source regenerates the winner's T steps with one thread per step into LDS (the kernels' reference rows are
//                               free by then), so that the one emitting thread neither runs T Philox calls in sequence nor waits for a
//                               warm-start load per step behind its own warm-start stores
//   F1P_ST_EMIT_DV / _A(ce, t, bi)   the winner's controls of step t in the emission
//   F1P_ST_EMIT_TAIL(e, t, dv, a)   after step t of the winner's re-emission: streamed -- stop after step 0 when no best_seq is wanted;
//                                   generated -- write the next warm start
//   F1P_ST_COL                  1: the occupancy test of f1p_stmpc_set_collision -- the names get _col, the kernels a `KmpcCol col`
//                               parameter, the fp64 rollouts test each step as they take it, and F1P_ST_EMIT_BLOCKED(e) zeroes ego e's
//                               warm start in the "every rollout blocked" emission.  F1P_ST_COL_MIXED 1 also compiles the mixed schedule
//                               with the test (the generated source only: f1p_stmpc_shoot_* run the plain-fp64 kernel while the test is
//                               on): the filter looks its tested points up in the clearance map and lists FREE and UNSURE rollouts, the
//                               refinement marks a blocked item (cost +inf, listed index F1P_K4_NONE), the decision skips those.
//                               Everything the test adds sits inside #if F1P_ST_COL, so the two inclusions without it keep their
//                               preprocessed tokens.
// all rollouts of this thread, first-minimum argmin (objective :616-622, bounds :685-706 as a projection)
template <bool FAST>
__device__ __forceinline__ void F1P_ST_N(stmpc_rollouts)(F1P_ST_SRC_PARAM, const double* sref, const f1p_stmpc_cfg& cfg, const DynConst& k,
                                               const DynState& s0, int tid, double& bc, int& bi
#if F1P_ST_COL
                                               , const KmpcCol& col
#endif
                                               ) {
    const int T = cfg.horizon, R = cfg.n_rollouts;
    for (int r = tid; r < R; r += blockDim.x) {
        DynState s = s0;
        double cost = 0.0, pdv = 0.0, pa = 0.0;
#if F1P_ST_COL
        bool blocked = false;
#endif
        for (int t = 0; t < T; ++t) {
            double dv = clampd2((double)F1P_ST_DV(ce, t, r), -cfg.max_steer_v, cfg.max_steer_v);   // :701-703
            double a = clampd2((double)F1P_ST_A(ce, t, r), -cfg.max_accel, cfg.max_accel);        // :704-706
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);                         // :685
            const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + t]; q += cfg.q[j] * er * er; }   // :619
            cost += q;
            cost += cfg.r[0] * dv * dv + cfg.r[1] * a * a;                                                       // :616
            if (t > 0) { const double d0 = dv - pdv, d1 = a - pa; cost += cfg.rd[0] * d0 * d0 + cfg.rd[1] * d1 * d1; }   // :622
#if F1P_ST_COL
            const double px = s.x, py = s.y;
#endif
            dyn_step<FAST>(s, a, dv, cfg, k);
#if F1P_ST_COL
            if (col.seg(px, py, s.x, s.y)) { blocked = true; break; }   // the points of step t -> t + 1; a blocked rollout stops at its first occupied point
#endif
            pdv = dv; pa = a;
        }
#if F1P_ST_COL
        if (blocked) continue;                                        // takes no part in the argmin: (bc, bi) stays (+inf, F1P_K4_NONE) while nothing is free
#endif
        const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + T]; q += cfg.qf[j] * er * er; }
        cost += q;
        if (argmin_better(cost, r, bc, bi)) { bc = cost; bi = r; }
    }
}

__global__ __launch_bounds__(256) void F1P_ST_N(k_stmpc_shoot)(const double* __restrict__ x0, const double* __restrict__ ref,
                                                     F1P_ST_CTL_PARAM, int E, f1p_stmpc_cfg cfg,
#if F1P_ST_COL
                                                     KmpcCol col,
#endif
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
    F1P_ST_SRC_DECL(ce, e);
    double bc = __builtin_huge_val(); int bi = 0x7fffffff;
#if F1P_ST_COL
    if (fabs(cfg.max_steer) <= 1.0e4) F1P_ST_N(stmpc_rollouts)<true>(ce, sref, cfg, k, s0, tid, bc, bi, col);     // workgroup-uniform
    else F1P_ST_N(stmpc_rollouts)<false>(ce, sref, cfg, k, s0, tid, bc, bi, col);
    block_argmin(bc, bi, red_d, red_i);
    if (bi == F1P_K4_NONE) {                                          // every rollout blocked (workgroup-uniform): the lattice's ALL_BLOCKED outputs
        for (int q = tid; q < 2 * T; q += blockDim.x) {
            if (best_seq) best_seq[(size_t)e * T * 2 + q] = 0.0;
            F1P_ST_EMIT_BLOCKED(e, q)
        }
        if (tid == 0) {
            steer[e] = 0.0; speed[e] = 0.0; best_idx[e] = -1;
            if (best_cost) best_cost[e] = __builtin_huge_val();
        }
        return;
    }
#else
    if (fabs(cfg.max_steer) <= 1.0e4) F1P_ST_N(stmpc_rollouts)<true>(ce, sref, cfg, k, s0, tid, bc, bi);     // workgroup-uniform
    else F1P_ST_N(stmpc_rollouts)<false>(ce, sref, cfg, k, s0, tid, bc, bi);
    block_argmin(bc, bi, red_d, red_i);
#endif
    F1P_ST_EMIT_PRE(ce, bi)
    if (tid == 0) {
        double pdv = 0.0;
        for (int t = 0; t < T; ++t) {
            double dv = clampd2((double)F1P_ST_EMIT_DV(ce, t, bi), -cfg.max_steer_v, cfg.max_steer_v);
            const double a = clampd2((double)F1P_ST_EMIT_A(ce, t, bi), -cfg.max_accel, cfg.max_accel);
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
            if (t == 0) {
                steer[e] = s0.delta + dv * cfg.dt;   // :1112
                speed[e] = s0.v + a * cfg.dt;        // :1117
            }
            if (best_seq) { best_seq[((size_t)e * T + t) * 2] = dv; best_seq[((size_t)e * T + t) * 2 + 1] = a; }
            F1P_ST_EMIT_TAIL(e, t, dv, a)
            pdv = dv;
        }
        best_idx[e] = bi;
        if (best_cost) best_cost[e] = bc;
    }
}

#if !F1P_ST_COL || F1P_ST_COL_MIXED
// fp64 cost of ONE rollout: the body of F1P_ST_N(stmpc_rollouts) for a given r (same operations, same order)
template <bool FAST>
__device__ __forceinline__ double F1P_ST_N(stmpc_one_rollout)(F1P_ST_SRC_PARAM, const double* sref, const f1p_stmpc_cfg& cfg, const DynConst& k,
                                                    const DynState& s0, int r
#if F1P_ST_COL
                                                    , const KmpcCol& col, bool& blocked
#endif
                                                    ) {
    const int T = cfg.horizon, R = cfg.n_rollouts;
    DynState s = s0;
    double cost = 0.0, pdv = 0.0, pa = 0.0;
#if F1P_ST_COL
    blocked = false;
#endif
    for (int t = 0; t < T; ++t) {
        double dv = clampd2((double)F1P_ST_DV(ce, t, r), -cfg.max_steer_v, cfg.max_steer_v);
        double a = clampd2((double)F1P_ST_A(ce, t, r), -cfg.max_accel, cfg.max_accel);
        if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
        const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + t]; q += cfg.q[j] * er * er; }
        cost += q;
        cost += cfg.r[0] * dv * dv + cfg.r[1] * a * a;
        if (t > 0) { const double d0 = dv - pdv, d1 = a - pa; cost += cfg.rd[0] * d0 * d0 + cfg.rd[1] * d1 * d1; }
#if F1P_ST_COL
        const double px = s.x, py = s.y;
#endif
        dyn_step<FAST>(s, a, dv, cfg, k);
#if F1P_ST_COL
        if (col.seg(px, py, s.x, s.y)) { blocked = true; return __builtin_huge_val(); }
#endif
        pdv = dv; pa = a;
    }
    const double sv[7] = {s.x, s.y, s.delta, s.v, s.yaw, s.yr, s.beta};
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) { const double er = sv[j] - sref[j * (T + 1) + T]; q += cfg.qf[j] * er * er; }
    cost += q;
    return cost;
}

template <int QM>
__global__ __launch_bounds__(256) void F1P_ST_N(k_stmpc_filter)(const double* __restrict__ x0, const double* __restrict__ ref,
                                                      F1P_ST_CTL_PARAM, int E, int T, int R, double max_steer_d, DynF32 kf,
#if F1P_ST_COL
                                                      KmpcCol col,
#endif
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
#if F1P_ST_COL
    // the ego's cell (fp64) anchors the filter's cell coordinates; an ego without one is decided in fp64
    const double bxd = (sx - col.g.ox) * col.g.inv_res, byd = (sy - col.g.oy) * col.g.inv_res;
    const bool in_range = fabs(syaw) <= 1.0e4 && fabs(max_steer_d) <= 1.0e4 && fabs(sbeta) <= 100.0 && fabs(sdelta) <= 100.0 &&
                          fabs(bxd) < 1.0e6 && fabs(byd) < 1.0e6;   // workgroup-uniform
#else
    const bool in_range = fabs(syaw) <= 1.0e4 && fabs(max_steer_d) <= 1.0e4 && fabs(sbeta) <= 100.0 && fabs(sdelta) <= 100.0;   // workgroup-uniform
#endif
    if (!in_range) { if (tid == 0) nlist[e] = -1; return; }
    int bad_ref = 0;                                                 // a non-finite reference in an UNWEIGHTED row makes every fp64 cost NaN (0 * NaN): fp64 decides
    for (int q = tid; q < 7 * (T + 1); q += blockDim.x) {
        const double rv = ref[(size_t)e * 7 * (T + 1) + q];
        const int row = q / (T + 1), t = q - row * (T + 1);
        sref32[8 * t + row] = (float)(row == 0 ? rv - sx : (row == 1 ? rv - sy : (row == 4 ? rv - syaw : rv)));
        if (!((QM >> row) & 1) && !(fabs(rv) < __builtin_huge_val())) bad_ref = 1;
    }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    F1P_ST_FILTER_WARM(e)
    if (__syncthreads_or(bad_ref | ((QM != 0x7f && !(fabs(syr) < __builtin_huge_val())) ? 1 : 0))) { if (tid == 0) nlist[e] = -1; return; }
    F1P_ST_SRC_DECL_FILTER(ce, e);
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
#if F1P_ST_COL
    KmpcColF cf;                                                     // (the filter's positions are relative to the ego with the map's axes: unsure<false>)
    {
        const double ibx = __builtin_floor(bxd), iby = __builtin_floor(byd);
        cf.clear = col.clear; cf.wwords = col.g.wwords; cf.n_sub = col.n_sub; cf.inv_nsub = 1.0f / (float)col.n_sub;
        cf.ibx = __builtin_amdgcn_readfirstlane((int)ibx); cf.iby = __builtin_amdgcn_readfirstlane((int)iby);
        cf.bx = (float)(bxd - ibx); cf.by = (float)(byd - iby);
        cf.lox = (float)-cf.ibx; cf.hix = (float)(col.g.w - cf.ibx); cf.loy = (float)-cf.iby; cf.hiy = (float)(col.g.h - cf.iby);
        cf.inv_res = (float)col.g.inv_res; cf.c0 = 1.0f; cf.s0 = 0.0f;
    }
#endif
    // the odd polynomial of tan is good for |delta| <= 0.45: every later delta is clamped to max_steer, but step 0 evaluates tan(delta0)
    // UNCLAMPED (dyn_step does, like the reference) -- an out-of-range initial steering state takes the sin / cos path (workgroup-uniform)
    const bool poly = kf.max_steer <= 0.45f && fabs(sdelta) <= 0.45;
    float tmin = __builtin_huge_valf();
    constexpr int NR = F1P_ST_FILTER_NR;
    for (int rb = tid; rb < R; rb += NR * blockDim.x) {
        int rr[NR]; float c[NR]; bool trusted[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) rr[i] = rb + i * (int)blockDim.x < R ? rb + i * (int)blockDim.x : rb;   // past the end: a shadow of the first, not stored
#if F1P_ST_COL
        bool unsure[NR];                                             // a tested point near an occupied cell, off the image or NaN: not FREE
#ifdef F1P_ST_DBG_POS    // variant build: dbg_cost32 is [1 + 2 T][E][R] -- the costs, then the f32 (x, y) after every step (tools/stmpc_pos_error.py)
#define F1P_ST_POS_ARGS , dbg_cost32 ? dbg_cost32 + ((size_t)E + e) * R : nullptr, (size_t)E * R
#else
#define F1P_ST_POS_ARGS
#endif
        if (poly) F1P_ST_N(stmpc_rollout_f32)<true, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted, cf, unsure F1P_ST_POS_ARGS);
        else F1P_ST_N(stmpc_rollout_f32)<false, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted, cf, unsure F1P_ST_POS_ARGS);
#undef F1P_ST_POS_ARGS
#else
        if (poly) F1P_ST_N(stmpc_rollout_f32)<true, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted);
        else F1P_ST_N(stmpc_rollout_f32)<false, NR, QM>(ce, sref32, kk, T, R, rr, (float)sdelta, (float)sv, (float)syr, (float)sbeta, c, trusted);
#endif
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (i > 0 && rr[i] == rb) continue;
            float ci = c[i];
            if (!trusted[i] || !(ci == ci) || !(fabsf(ci) < 1e30f)) ci = -__builtin_huge_valf();      // untrusted / non-finite: fp64 decides
#if F1P_ST_COL
            else if (!unsure[i]) tmin = fminf(tmin, ci);            // the threshold comes from the FREE rollouts; an UNSURE one keeps its cost and is listed at or below it
#else
            else tmin = fminf(tmin, ci);
#endif
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

// ---- K-B: fp64 costs of the queued rollouts, one lane each, packed across egos (F1P_ST_N(stmpc_rollouts)' own arithmetic) ----------------
// ~1 rollout per ego survives the filter, so this kernel is a few dozen waves running 40 sequential fp64 steps: 1.3 us per step (34 us
// for a single wave of 17 rollouts, 52 us at 1024 egos), latency of the dependent fp64 chain and not throughput.  This kernel now only
// serves horizons > 63; F1P_ST_N(k_stmpc_refine_tp) below is what runs.  Measured and NOT kept
// (profiles/r03_stmpc_filter.md): splitting the step's independent chains over four waves with an LDS exchange per step, staging the
// controls in LDS and batching the reference loads -- each left the time where it was.
__global__ __launch_bounds__(64) void F1P_ST_N(k_stmpc_refine)(const double* __restrict__ x0, const double* __restrict__ ref, F1P_ST_CTL_PARAM,
                                                     f1p_stmpc_cfg cfg, const unsigned int* __restrict__ qcount, const StItem* __restrict__ items,
#if F1P_ST_COL
                                                     KmpcCol col, int32_t* __restrict__ rl,
#endif
                                                     double* __restrict__ rc) {
    const unsigned int count = *qcount;
    const int T = cfg.horizon, R = cfg.n_rollouts;
    const DynConst k = dyn_const(cfg);
    for (unsigned int i = blockIdx.x * 64u + threadIdx.x; i < count; i += gridDim.x * 64u) {
        const StItem it = items[i];
        const int e = it.es / F1P_ST_MAX_REFINE;
        DynState s0;
        s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
        s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
#if F1P_ST_COL
        bool blocked;
        rc[it.es] = F1P_ST_N(stmpc_one_rollout)<true>(F1P_ST_SRC_EXPR(e), ref + (size_t)e * 7 * (T + 1), cfg, k, s0, it.r, col, blocked);
        if (blocked) rl[it.es] = F1P_K4_NONE;                        // (its cost is +inf: the pair loses to every unblocked item)
#else
        rc[it.es] = F1P_ST_N(stmpc_one_rollout)<true>(F1P_ST_SRC_EXPR(e), ref + (size_t)e * 7 * (T + 1), cfg, k, s0, it.r);
#endif
    }
}

__global__ __launch_bounds__(256) void F1P_ST_N(k_stmpc_refine_tp)(const double* __restrict__ x0, const double* __restrict__ ref, F1P_ST_CTL_PARAM,
                                                        f1p_stmpc_cfg cfg, const unsigned int* __restrict__ qcount, const StItem* __restrict__ items,
#if F1P_ST_COL
                                                        KmpcCol col, int32_t* __restrict__ rl,
#endif
                                                        double* __restrict__ rc, float* __restrict__ dbg_ticks) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#ifdef F1P_ST_PHASES
    long long ph[12]; int nph = 0;
#define F1P_STPH() do { ph[nph++] = clock64(); } while (0)
#else
#define F1P_STPH() do {} while (0)
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
        F1P_ST_SRC_DECL_R(cp, e, it.r);                                   // [t][2][R], or regenerated: step t of rollout r is a pure function of (e, r, t)
        const double* sref = ref + (size_t)e * 7 * (T + 1);
        const float c_dv = act ? F1P_ST_DV_R(cp, t, it.r) : 0.0f, c_a = act ? F1P_ST_A_R(cp, t, it.r) : 0.0f;
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
#if F1P_ST_COL
        // ---- 5b. lane t tests the points of step t -> t + 1 (x_t, y_t are stmpc_rollouts' own values); a ballot ORs the verdicts --------
        bool blocked;
        {
            bool hit = false;
            if (act) { const StXY p = o6[t], q = o6[t + 1]; hit = col.seg(p.x, p.y, q.x, q.y); }
            blocked = __ballot(hit) != 0ull;
        }
#endif
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
        // ---- 7. the running sum, in F1P_ST_N(stmpc_rollouts)' order ---------------------------------------------------------------------------
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
#if F1P_ST_COL
            if (lane == 0) { rc[it.es] = blocked ? __builtin_huge_val() : cost; if (blocked) rl[it.es] = F1P_K4_NONE; }
#else
            if (lane == 0) rc[it.es] = cost;
#endif
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
__global__ __launch_bounds__(256) void F1P_ST_N(k_stmpc_decide)(const double* __restrict__ x0, const double* __restrict__ ref,
                                                      F1P_ST_CTL_PARAM, int E, f1p_stmpc_cfg cfg,
                                                      unsigned int* __restrict__ qcount, const int32_t* __restrict__ nlist, const int32_t* __restrict__ rl,
                                                      const double* __restrict__ rc,
#if F1P_ST_COL
                                                      KmpcCol col,
#endif
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
    if (e == 0 && tid == 0) *qcount = 0u;                             // re-arm the queue for the next plan (F1P_ST_N(k_stmpc_refine) has finished)
#if F1P_ST_COL
    int n = nlist[e];
#else
    const int n = nlist[e];
#endif
    DynState s0;
    s0.x = x0[7 * e]; s0.y = x0[7 * e + 1]; s0.delta = x0[7 * e + 2]; s0.v = x0[7 * e + 3]; s0.yaw = x0[7 * e + 4];
    s0.yr = x0[7 * e + 5]; s0.beta = x0[7 * e + 6];
    F1P_ST_SRC_DECL(ce, e);
    double bc = __builtin_huge_val(); int bi = 0x7fffffff;
#if F1P_ST_COL
    if (n >= 0) {                                                     // a blocked item is (+inf, F1P_K4_NONE): it loses to every unblocked one
        if (tid < n) {
            bc = rc[(size_t)e * F1P_ST_MAX_REFINE + tid];
            bi = rl[(size_t)e * F1P_ST_MAX_REFINE + tid];
        }
        block_argmin(bc, bi, red_d, red_i);
        // every listed rollout blocked: the list holds the FREE minimum, which the position bound proves unblocked, so this is not expected --
        // the ego is decided by the all-fp64 loop rather than declared blocked on the filter's word (workgroup-uniform)
        if (bi == F1P_K4_NONE) { n = -1; bc = __builtin_huge_val(); __syncthreads(); }
    }
    if (n < 0) {
        for (int q = tid; q < 7 * (T + 1); q += blockDim.x) sref[q] = ref[(size_t)e * 7 * (T + 1) + q];
        __syncthreads();
        const DynConst k = dyn_const(cfg);
        if (fabs(cfg.max_steer) <= 1.0e4) F1P_ST_N(stmpc_rollouts)<true>(ce, sref, cfg, k, s0, tid, bc, bi, col);
        else F1P_ST_N(stmpc_rollouts)<false>(ce, sref, cfg, k, s0, tid, bc, bi, col);
        block_argmin(bc, bi, red_d, red_i);
    }
    if (bi == F1P_K4_NONE) {                                          // every rollout blocked (workgroup-uniform)
        for (int q = tid; q < 2 * T; q += blockDim.x) {
            if (best_seq) best_seq[(size_t)e * T * 2 + q] = 0.0;
            F1P_ST_EMIT_BLOCKED(e, q)
        }
        if (tid == 0) {
            steer[e] = 0.0; speed[e] = 0.0; best_idx[e] = -1;
            if (best_cost) best_cost[e] = __builtin_huge_val();
            if (dbg_nref) dbg_nref[e] = n;
        }
        return;
    }
#else
    if (n < 0) {                                                      // workgroup-uniform
        for (int q = tid; q < 7 * (T + 1); q += blockDim.x) sref[q] = ref[(size_t)e * 7 * (T + 1) + q];
        __syncthreads();
        const DynConst k = dyn_const(cfg);
        if (fabs(cfg.max_steer) <= 1.0e4) F1P_ST_N(stmpc_rollouts)<true>(ce, sref, cfg, k, s0, tid, bc, bi);
        else F1P_ST_N(stmpc_rollouts)<false>(ce, sref, cfg, k, s0, tid, bc, bi);
    } else if (tid < n) {
        bc = rc[(size_t)e * F1P_ST_MAX_REFINE + tid];
        bi = rl[(size_t)e * F1P_ST_MAX_REFINE + tid];
    }
    block_argmin(bc, bi, red_d, red_i);
#endif
    F1P_ST_EMIT_PRE(ce, bi)
    if (tid == 0) {
        double pdv = 0.0;
        for (int t = 0; t < T; ++t) {
            double dv = clampd2((double)F1P_ST_EMIT_DV(ce, t, bi), -cfg.max_steer_v, cfg.max_steer_v);
            const double a = clampd2((double)F1P_ST_EMIT_A(ce, t, bi), -cfg.max_accel, cfg.max_accel);
            if (t > 0) dv = clampd2(dv, pdv - cfg.max_steer_v, pdv + cfg.max_steer_v);
            if (t == 0) {
                steer[e] = s0.delta + dv * cfg.dt;   // :1112
                speed[e] = s0.v + a * cfg.dt;        // :1117
            }
            if (best_seq) { best_seq[((size_t)e * T + t) * 2] = dv; best_seq[((size_t)e * T + t) * 2 + 1] = a; }
            F1P_ST_EMIT_TAIL(e, t, dv, a)
            pdv = dv;
        }
        best_idx[e] = bi;
        if (best_cost) best_cost[e] = bc;
        if (dbg_nref) dbg_nref[e] = n;
    }
}
#endif   // !F1P_ST_COL || F1P_ST_COL_MIXED
