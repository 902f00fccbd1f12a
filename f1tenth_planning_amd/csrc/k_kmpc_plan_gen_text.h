// k_kmpc_plan_gen_text.h -- the text of k_kmpc_plan_gen, included by k_kmpc.hip once per kernel it defines:
//   F1P_KPG_NAME   the kernel's name           F1P_KPG_EXTRA  parameters after `ga` (with their trailing comma), or nothing
//   F1P_KPG_EGO    the generator's ego word    F1P_KPG_WROW   first float of ego e's row in ga.warm_in / ga.warm_out
//   F1P_KPG_COL    1: the occupancy test of f1p_kmpc_set_collision (F1P_KPG_EXTRA then declares `KmpcCol col`; one workgroup per ego only).
//                  The filter marks each rollout FREE or UNSURE next to its f32 cost, the threshold comes from the FREE minimum, the
//                  FREE and UNSURE rollouts at or below it are refined in fp64 with the exact test.
// (A kernel text compiled twice, not a shared inlined body: k_kmpc_plan_gen's code object has to stay what it was, instruction for
// instruction, and the optimiser does not promise that for a __global__ wrapper around an inlined template.)
__global__ __launch_bounds__(256, F1P_K4_WAVES_GEN) void F1P_KPG_NAME(const double* __restrict__ x0, const double* __restrict__ ref, int E,
                                                       f1p_kmpc_cfg cfg, KmpcF32 kf, KmpcGenArgs ga, F1P_KPG_EXTRA
                                                       double* __restrict__ steer, double* __restrict__ speed,
                                                       int32_t* __restrict__ best_idx, double* __restrict__ best_cost,
                                                       double* __restrict__ best_seq, int32_t* __restrict__ n_refined,
                                                       const f1p_kmpc_cfg* __restrict__ dcfg) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int T = cfg.horizon, R = cfg.n_rollouts, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    float* sref32 = reinterpret_cast<float*>(lds_raw);                // [4][T+1] relative to the ego state, f32
    float* warm_s = sref32 + 4 * (T + 1);                             // [T][2] this ego's warm start
    float* red_f = warm_s + 2 * T;                                    // [4]
    int* list = reinterpret_cast<int*>(red_f + 4);                    // [F1P_K4_MAX_REFINE]
    int* cnt = list + F1P_K4_MAX_REFINE;                              // [2]: survivors, "this workgroup is the last one"
    double* sref = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(cnt + 2) + 7) & ~(uintptr_t)7);   // fp64 refinement scratch
    float* c32 = reinterpret_cast<float*>(sref + 4 * (T + 1) + 4 + 2);   // [R] filter costs (G == 1: LDS only)
    const int e = blockIdx.x / ga.G, g = blockIdx.x - e * ga.G;
    if (e >= E) return;
#ifdef F1P_K4_PHASES     // shader-clock stamps at the phase boundaries -> n_refined-shaped debug rows in ga.cost32 (tools/kmpc_phases.py)
    long long tph[8]; int nph = 0;
#define F1P_KPH() do { tph[nph++] = clock64(); } while (0)
#define F1P_KPH_OUT() do { F1P_KPH(); if (tid == 0 && ga.cost32 && ga.G == 1) { for (int k_ = 0; k_ + 1 < nph; ++k_) ga.cost32[(size_t)e * R + k_] = (float)(tph[k_ + 1] - tph[k_]); ga.cost32[(size_t)e * R + 7] = (float)(tph[0] & 0xffffff); ga.cost32[(size_t)e * R + 8] = (float)(tph[nph - 1] & 0xffffff); for (int k_ = 0; k_ < 11; ++k_) ga.cost32[(size_t)e * R + 24 + k_] = (float)(f1p_kst[k_ + 1] - f1p_kst[k_]); ga.cost32[(size_t)e * R + 35] = (float)(f1p_kst[0] - tph[nph - 2]); } if (lane == 0 && ga.cost32 && ga.G == 1) { ga.cost32[(size_t)e * R + 10 + wave] = (float)(__builtin_amdgcn_s_getreg(63492) & 0xffff); ga.cost32[(size_t)e * R + 14 + wave] = (float)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf); ga.cost32[(size_t)e * R + 18 + wave] = (float)(clock64() - tph[0]); } } while (0)
#else
#define F1P_KPH() do {} while (0)
#define F1P_KPH_OUT() do {} while (0)
#endif
    F1P_KPH();
    const double sx = x0[4 * e], sy = x0[4 * e + 1], sv = x0[4 * e + 2], syaw = x0[4 * e + 3];
    for (int q = tid; q < 2 * T; q += blockDim.x) warm_s[q] = ga.warm_in ? ga.warm_in[F1P_KPG_WROW + q] : 0.0f;
#if F1P_KPG_COL
    SrcColT<SrcGenT<true>> src;
    src.col = col; src.blocked = false;
#else
    SrcGenT<true> src;
#endif
    src.k0 = ga.k0; src.k1 = ga.k1; src.call = ga.call; src.ego = F1P_KPG_EGO; src.sig_a = ga.sig_a; src.sig_d = ga.sig_d;
    src.warm = warm_s;
    float* warm_out = ga.warm_out ? ga.warm_out + F1P_KPG_WROW : nullptr;
#if F1P_KPG_COL
    // the ego's cell (fp64) anchors the filter's cell coordinates; an ego without one, no clearance map or f1p_kmpc_set_mode(0): all in fp64
    const double bxd = (sx - col.g.ox) * col.g.inv_res, byd = (sy - col.g.oy) * col.g.inv_res;
    const bool col_ok = col.clear && !col.force64 && fabs(bxd) < 1.0e6 && fabs(byd) < 1.0e6;
    const bool in_range = fabs(syaw) <= 1.0e4 && fabs(cfg.max_steer) <= 1.0e4 && kf.w_ok && col_ok;
#else
    const bool in_range = fabs(syaw) <= 1.0e4 && fabs(cfg.max_steer) <= 1.0e4 && kf.w_ok;     // workgroup-uniform: the fast paths' ranges
#endif
    double s0d, c0d;
    sincos_core(in_range ? syaw : 0.0, &s0d, &c0d);
    const bool poly = kf.max_steer <= 0.45f;
    const bool iso = poly && kf.sq[0] == kf.sq[1] && kf.sqf[0] == kf.sqf[1];
    for (int q = tid; q < 4 * (T + 1); q += blockDim.x) {
        const double rv = ref[(size_t)e * 4 * (T + 1) + q];
        sref[q] = rv;                                                 // the fp64 rows the refinement reads (no second trip to memory at the kernel's tail)
        const int row = q / (T + 1), col = q - row * (T + 1);
        sref32[q] = kmpc_ref32(kf, row, col == T, kmpc_rel_ref(ref + (size_t)e * 4 * (T + 1), T, row, col, rv, sx, sy, syaw, iso, c0d, s0d));
    }
    if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
    __syncthreads();
    KmpcF32 k = kf;
    k.c0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)c0d)));
    k.s0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)s0d)));
    k.v0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, (float)sv)));

#if F1P_KPG_COL
    KmpcColF cf;
    {
        const double ibx = col_ok ? __builtin_floor(bxd) : 0.0, iby = col_ok ? __builtin_floor(byd) : 0.0;
        cf.clear = col.clear; cf.wwords = col.g.wwords; cf.n_sub = col.n_sub; cf.inv_nsub = 1.0f / (float)col.n_sub;
        cf.ibx = __builtin_amdgcn_readfirstlane((int)ibx); cf.iby = __builtin_amdgcn_readfirstlane((int)iby);
        cf.bx = (float)(bxd - ibx); cf.by = (float)(byd - iby);
        cf.lox = (float)-cf.ibx; cf.hix = (float)(col.g.w - cf.ibx); cf.loy = (float)-cf.iby; cf.hiy = (float)(col.g.h - cf.iby);
        cf.inv_res = (float)col.g.inv_res; cf.c0 = k.c0; cf.s0 = k.s0;
    }
#endif
    F1P_KPH();
    // ---- pass A: f32 filter over this workgroup's slice ---------------------------------------------------------------
    const int r_lo = g * ga.Rs, r_hi = min(R, r_lo + ga.Rs);
    float* cost_out = ga.G > 1 ? ga.cost32 + (size_t)e * R : c32;
    float fmin_ = __builtin_huge_valf();                              // G == 1: this thread's minimum, straight from the filter's registers
    if (in_range) {
        const int half = (r_hi - r_lo + 1) >> 1;                      // rollouts r and r + half share the packed lanes
        for (int q = tid; q < half; q += blockDim.x) {
            const int r = r_lo + q, r1 = r + half < r_hi ? r + half : r;
#if F1P_KPG_COL
            bool u0, u1;
            const f1p_f2 c = iso ? kmpc_rollout_cost_f32x2_col<true, true>(src, sref32, k, T, r, r1, cf, u0, u1)
                                 : (poly ? kmpc_rollout_cost_f32x2_col<true, false>(src, sref32, k, T, r, r1, cf, u0, u1)
                                         : kmpc_rollout_cost_f32x2_col<false, false>(src, sref32, k, T, r, r1, cf, u0, u1));
            cost_out[r] = c.x;
            if (r1 != r) cost_out[r1] = c.y;
            // the minimum over FREE rollouts only; the flags are not kept: the survivors are the FREE and the UNSURE rollouts at or below the threshold alike
            fmin_ = fminf(fmin_, fminf(u0 ? __builtin_huge_valf() : c.x, u1 ? __builtin_huge_valf() : c.y));
#else
            const f1p_f2 c = iso ? kmpc_rollout_cost_f32x2<true, true>(src, sref32, k, T, r, r1)
                                 : (poly ? kmpc_rollout_cost_f32x2<true, false>(src, sref32, k, T, r, r1) : kmpc_rollout_cost_f32x2<false, false>(src, sref32, k, T, r, r1));
            cost_out[r] = c.x;
            if (r1 != r) cost_out[r1] = c.y;
            fmin_ = fminf(fmin_, fminf(c.x, c.y));                     // NaN costs are ignored here and caught below (r1 == r: c.y repeats c.x)
#endif
#ifndef F1P_K4_PHASES
            if (ga.G == 1 && ga.cost32) { ga.cost32[(size_t)e * R + r] = c.x; if (r1 != r) ga.cost32[(size_t)e * R + r1] = c.y; }
#endif
        }
    }
    F1P_KPH();
    if (ga.G > 1) {
        __threadfence();                                              // this workgroup's costs are visible device-wide ...
        __syncthreads();
        if (tid == 0) {
            const unsigned int t_ = atomicAdd(&ga.tickets[e], 1u);    // ... before its ticket is
            cnt[1] = (t_ == (unsigned int)ga.G - 1u) ? 1 : 0;
            if (cnt[1]) ga.tickets[e] = 0u;                           // ready for the next launch (stream-ordered)
        }
        __syncthreads();
        if (!cnt[1]) return;
        __threadfence();
    } else {
        __syncthreads();
    }

    F1P_KPH();
    // ---- second stage (the ego's last workgroup): minimum -> near-minimum set -> fp64 refinement ------------------------
    // (round 5: ONE inlined copy of the refinement and one of the emission -- there were three and one; n_eff = -1: every rollout in fp64)
    int n_eff = -1;
    if (in_range) {
        if (ga.G > 1) {
            fmin_ = __builtin_huge_valf();
            for (int r = tid; r < R; r += blockDim.x)
                fmin_ = fminf(fmin_, __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const int*>(cost_out + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) fmin_ = fminf(fmin_, __shfl_xor(fmin_, m, 64));
        if (lane == 0) red_f[wave] = fmin_;
        __syncthreads();
        fmin_ = red_f[0];
        for (int w = 1; w < nwaves; ++w) fmin_ = fminf(fmin_, red_f[w]);
        const float thr = fmin_ + (fabsf(fmin_) * fminf(F1P_K4_MARGIN_REL * (float)T, 0.5f) + F1P_K4_MARGIN_ABS);
        for (int r = tid; r < R; r += blockDim.x) {
            float c;
            if (ga.G > 1) c = __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const int*>(cost_out + r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            else c = cost_out[r];
            if (!(c > thr)) {                                              // includes NaN
                const int pos = atomicAdd(cnt, 1);
                if (pos < F1P_K4_MAX_REFINE) list[pos] = r;
            }
        }
        __syncthreads();
        const int n = cnt[0];
        n_eff = (n > F1P_K4_MAX_REFINE || n < 1 || !isfinite(fmin_)) ? -1 : n;   // pathological inputs, degenerate ties (COL: no FREE rollout): all rollouts in fp64
    }
    F1P_KPH();
    const f1p_kmpc_cfg& s_cfg = *dcfg;                               // (the device copy: see k_kmpc_shoot_mixed)
    if (n_eff == 1 && !best_cost) {
        // a single survivor needs no fp64 cost unless it is asked for (COL: it is the FREE minimum, proved free)
        kmpc_emit_wave(src, s_cfg, sv, s_cfg.max_dsteer * s_cfg.dt, e, list[0], 0.0, steer, speed, best_idx, nullptr, best_seq, warm_out);
        if (tid == 0 && n_refined) n_refined[e] = 1;
    } else {
        // the survivors in ascending rollout order: the atomic list is in arrival order, the decision (first minimum) is by index
        kmpc_refine_block(ref, src, s_cfg, sx, sy, sv, syaw, e, n_eff, list, sref, steer, speed, best_idx, best_cost, best_seq, n_refined, warm_out, true);
    }
    F1P_KPH_OUT();
}

