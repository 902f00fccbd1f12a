// shoot_gen.h -- the control generator of the shooting MPCs with in-kernel controls (f1p_kmpc_plan_*, f1p_stmpc_plan_*): Philox4x32-10,
// the byte-sum variate and the per-ego control source built from them.  Shared by k_kmpc.hip and k_stmpc.hip; the description of the
// generator is in k_kmpc.hip ("Where a rollout's controls come from"), its CPU restatement oracle/f1p_oracle.c orc_kmpc_gen_controls.
// Channel 0 / 1 of a step come from word 0 / 1 (even step) or 2 / 3 (odd step) of the pair's Philox output: (accel, steer) for the
// kinematic model, (steering speed, accel) for the dynamic one -- the order of their [E][T][2][R] control buffers.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace f1p {

#define F1P_IH_MEAN 510.0f                     // 4 bytes x 127.5
#define F1P_IH_INV_STD 0.0067658765f           // 1 / sqrt(4 (256^2 - 1) / 12) = 1 / 147.80054, rounded to f32 (same literal in the oracle)

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& o0, uint32_t& o1, uint32_t& o2, uint32_t& o3) {
    // the 32 x 32 -> 64 products as ONE v_mad_u64_u32 each: the compiler's v_mul_lo_u32 + v_mul_hi_u32 pair costs 1.5x as much
    // (tools/microbench/intops.hip: 6.5 + 6.4 against 8.5 time units), and Philox is most of this kernel's instructions
    const uint32_t m0 = 0xD2511F53u, m1 = 0xCD9E8D57u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        unsigned long long p0, p1;
        asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(p0) : "s"(m0), "v"(c0) : "vcc");
        asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(p1) : "s"(m1), "v"(c2) : "vcc");
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;          // (gfx950 has no v_xor3_b32: two xors per word)
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1; o2 = c2; o3 = c3;
}

// WARM_SET: `warm` is never null (k_kmpc_plan_gen's LDS copy, zero-filled without a warm start) -- no null test, hence no branch
// around each of the filter's warm-start reads (each one used to end a basic block, and with it the scheduler's view)
template <bool WARM_SET>
struct SrcGenT {
    uint32_t k0, k1, call, ego;
    float sig_a, sig_d;
    const float* warm;          // [T][2] (accel, steer) of this ego, LDS or global; nullptr = no warm start (zeros)
    static constexpr int chunk = 6;               // six steps (three Philox calls per rollout) per basic block: 0.0467 ms against 0.048 with 2 or 4
    __device__ __forceinline__ void one(int t, int r, uint32_t xa, uint32_t xd, float& a, float& d) const {
        // sum of the word's 4 bytes minus 510, the mean folded into v_sad_u8's accumulator: integers of magnitude <= 510, exact in
        // f32 either way, so (float)(sum - 510) is the same value as (float)sum - 510.0f without the v_add_f32
        const float za = (float)(int)__builtin_amdgcn_sad_u8(xa, 0u, (uint32_t)-(int)F1P_IH_MEAN) * F1P_IH_INV_STD;
        const float zd = (float)(int)__builtin_amdgcn_sad_u8(xd, 0u, (uint32_t)-(int)F1P_IH_MEAN) * F1P_IH_INV_STD;
        const float wa = WARM_SET || warm ? warm[2 * t] : 0.0f, wd = WARM_SET || warm ? warm[2 * t + 1] : 0.0f;
        // rollout 0 = the warm start itself, rollout 1 = all zero, as per-lane FACTORS instead of two compares + two selects per
        // control (r is fixed per lane for the whole rollout, so the factors fold into loop-invariant registers): sigma -> 0 for
        // r < 2, warm -> 0 for r = 1.  fma(0, z, w) = w and fma(0, z, w * 0) = +-0 exactly: the same controls, bit for bit in value.
        const float fs = r < 2 ? 0.0f : 1.0f, fw = r == 1 ? 0.0f : 1.0f;
        a = __builtin_fmaf(sig_a * fs, za, wa * fw);
        d = __builtin_fmaf(sig_d * fs, zd, wd * fw);
    }
    __device__ __forceinline__ void get(int t, int r, float& a, float& d) const {
        uint32_t x0, x1, x2, x3;
        philox4x32_10((uint32_t)(t >> 1), (uint32_t)r, ego, call, k0, k1, x0, x1, x2, x3);
        one(t, r, (t & 1) ? x2 : x0, (t & 1) ? x3 : x1, a, d);
    }
    // steps te and te + 1 (te even) from ONE Philox call; steps >= T are generated like any other (and unused).  FULL: te + 1 < T
    template <bool FULL = false>
    __device__ __forceinline__ void get2(int te, int T, int r, float& a0, float& d0, float& a1, float& d1) const {
        uint32_t x0, x1, x2, x3;
        philox4x32_10((uint32_t)(te >> 1), (uint32_t)r, ego, call, k0, k1, x0, x1, x2, x3);
        const int tb = FULL || te + 1 < T ? te + 1 : te;              // warm[] has T rows
        one(FULL || te < T ? te : T - 1, r, x0, x1, a0, d0);
        one(FULL || tb < T ? tb : T - 1, r, x2, x3, a1, d1);
    }
};
typedef SrcGenT<false> SrcGen;

}  // namespace f1p
