// shoot_col.h -- the rollout tests of the shooting MPCs (f1p_kmpc_set_collision / _set_obstacles, f1p_stmpc_set_collision / _set_obstacles;
// DESIGN.md 5h - 5k), once for k_kmpc.hip and k_stmpc.hip.  fp64 side: KmpcCol (the occupancy bitmap, its point test and segment rule), KmpcObs
// (the moving discs on top of it), col_seg, obs_compact.  f32 filters' side: KmpcColF (the clearance look-up) and its set-up col_filter,
// KmpcObsF (the discs' f32 table), the packed-pair type f1p_f2, and ColTestNone / ColTestGrid / ColTestObs: what a filter's rollout tests
// after every step, the type both planners' tested f32 rollouts are templated on (ColTestNone: k_stmpc.hip only, whose plain generating
// rollout has the tested ones' shape; k_kmpc.hip's plain rollout runs in chunks and stays a function of its own).
#pragma once
#include <type_traits>
#include "f1p_device.h"

namespace f1p {

#define F1P_K4_NONE 0x7fffffff        // argmin index while no unblocked rollout has been seen
struct KmpcCol {
    GridDev g;                        // the active bitmap
    const uint32_t* clear;            // clearance map for the f32 filter (null: the filter proves nothing, every rollout in fp64)
    int n_sub;                        // tested points per time step, 1 .. 16
    int force64;                      // f1p_kmpc_set_mode(0): no filter
    __device__ __forceinline__ bool occupied(double x, double y) const {
        int gx, gy;
        if (!cell_of(g, x, y, gx, gy)) return true;
        return (g.bits[(size_t)gy * g.wwords + (gx >> 5)] >> (gx & 31)) & 1u;
    }
    // the tested points of the step p -> q
    __device__ __forceinline__ bool seg(double px, double py, double qx, double qy) const {
        bool hit = false;
        for (int j = 1; j < n_sub; ++j) {
            const double f = (double)j / (double)n_sub;
            hit |= occupied(px + (qx - px) * f, py + (qy - py) * f);
        }
        return hit | occupied(qx, qy);
    }
};
// The test is an OPTIONAL kernel argument: the shooting kernels are templates over a pack of optional arguments, a KmpcCol (or a struct
// derived from it) the last of them, and `if constexpr (has_col<Extra...>)` keeps every statement of the test out of an instantiation
// without it -- whose kernarg layout and instructions are those of a kernel written without the argument.
template <typename... X> constexpr bool has_col = (std::is_base_of_v<KmpcCol, X> || ...);
template <typename A> __device__ __forceinline__ const A& col_of(const A& c) { return c; }
template <typename A, typename B, typename... X> __device__ __forceinline__ const auto& col_of(const A&, const B& b, const X&... x) { return col_of(b, x...); }

// the f32 filters' side of the test: the tested points looked up in the CLEARANCE map, cell coordinates relative to the ego's cell
// (used through ColTestGrid / ColTestObs below)
#define F1P_K4_CLEAR_CELLS 2.0
// (guarded: the no-allowance variant build that shows tests/test_gpu_shoot_graze.py bites sets both to 0.0, DESIGN.md 5j "Tests")
#ifndef F1P_K4_POS_ERR_REL
#define F1P_K4_POS_ERR_REL 1.0e-4
#endif
#ifndef F1P_K4_OBS_ERR_REL
#define F1P_K4_OBS_ERR_REL 1.0e-6     // the roundings of the obstacle's side in obs_compact's FREE threshold, relative to S (>= 16 x 2^-24)
#endif
struct KmpcColF {
    const uint32_t* clear;
    int wwords, n_sub, ibx, iby;
    float inv_nsub, bx, by, lox, hix, loy, hiy, inv_res, c0, s0;
    // (x, y): the filter's position -- ego frame (ISO) or world axes relative to the ego
    template <bool ISO>
    __device__ __forceinline__ bool unsure(float x, float y) const {
        const float rx = ISO ? c0 * x - s0 * y : x, ry = ISO ? s0 * x + c0 * y : y;
        const float fx = floorf(bx + rx * inv_res), fy = floorf(by + ry * inv_res);
        const bool inside = (fx >= lox) & (fx < hix) & (fy >= loy) & (fy < hiy);      // NaN -> outside
#ifdef F1P_K4_COL_NOLOOKUP            // A/B build: the cell arithmetic without the map read (where the open-space time goes)
        return !inside;
#else
        const int gx = inside ? ibx + (int)fx : 0, gy = inside ? iby + (int)fy : 0;   // (inside: 0 <= gx < w, 0 <= gy < h)
        return !inside | (bool)((clear[(size_t)gy * wwords + (gx >> 5)] >> (gx & 31)) & 1u);
#endif
    }
};
// the filter's view of `col` for an ego whose position is cell (bxd, byd) of the map (fp64, fractional); ok: the ego has a cell (else the
// anchor is cell 0 and the launch's `in_range` keeps the filter from running).  (c0, s0): the rotation from the filter's frame to the
// map's axes (unsure<ISO = true>)
__device__ __forceinline__ KmpcColF col_filter(const KmpcCol& col, double bxd, double byd, bool ok, float c0, float s0) {
    KmpcColF cf;
    const double ibx = ok ? __builtin_floor(bxd) : 0.0, iby = ok ? __builtin_floor(byd) : 0.0;
    cf.clear = col.clear; cf.wwords = col.g.wwords; cf.n_sub = col.n_sub; cf.inv_nsub = 1.0f / (float)col.n_sub;
    cf.ibx = __builtin_amdgcn_readfirstlane((int)ibx); cf.iby = __builtin_amdgcn_readfirstlane((int)iby);
    cf.bx = (float)(bxd - ibx); cf.by = (float)(byd - iby);
    cf.lox = (float)-cf.ibx; cf.hix = (float)(col.g.w - cf.ibx); cf.loy = (float)-cf.iby; cf.hiy = (float)(col.g.h - cf.iby);
    cf.inv_res = (float)col.g.inv_res; cf.c0 = c0; cf.s0 = s0;
    return cf;
}

// two rollouts in the halves of one packed-f32 value (k_kmpc.hip's filter)
typedef float f1p_f2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------
// Moving obstacles (f1p_kmpc_set_obstacles): discs (x, y, vx, vy, r) per ego, map frame, at constant velocity.  The tested
// points are the occupancy test's; the point of step t at fraction f = j / n_sub has the time  tau = ((double)t + f) * dt,  a live slot's
// centre is there  c = (x + vx tau, y + vy tau),  and the point is blocked when  !(|P - c|^2 > r r)  -- touching blocks, a NaN blocks.
// KmpcObs IS a KmpcCol (has_col finds it, every decision path of the occupancy test serves it): a null bitmap means "no grid", with one
// the point is tested against both.  `obs` / `M` come from the launcher; `live` / `n_live` are filled in by the kernel, once per
// workgroup: the ego's live slots (r >= 0) that can be reached within the horizon, compacted into LDS as (x, y, vx, vy, r r).
// ---------------------------------------------------------------------------------------------------
struct KmpcObs : KmpcCol {
    const double* obs;                // [E][M][5]
    int M;
    const double* live;               // LDS [n_live][5]
    int n_live;
    __device__ __forceinline__ bool disc(double x, double y, double tau) const {
        bool hit = false;
        for (int m = 0; m < n_live; ++m) {
            const double* o = live + 5 * m;
            const double cx = o[0] + o[2] * tau, cy = o[1] + o[3] * tau;
            const double dx = x - cx, dy = y - cy, d2 = dx * dx + dy * dy;
            hit |= !(d2 > o[4]);
        }
        return hit;
    }
    // the tested points of step t, p -> q
    __device__ __forceinline__ bool seg_t(int t, double dt, double px, double py, double qx, double qy) const {
        bool hit = false;
        for (int j = 1; j <= n_sub; ++j) {
            const double f = (double)j / (double)n_sub;
            const bool end = j == n_sub;                              // (p_{t+1} itself, not p + (q - p) * 1.0)
            const double x = end ? qx : px + (qx - px) * f, y = end ? qy : py + (qy - py) * f;
            if (g.bits) hit |= occupied(x, y);
            hit |= disc(x, y, ((double)t + f) * dt);
        }
        return hit;
    }
};
template <typename... X> constexpr bool has_obs = (std::is_base_of_v<KmpcObs, X> || ...);
// the test's argument type in a pack of optional arguments (the last of them; KmpcCol when there is none)
template <typename... X> struct col_arg { using type = KmpcCol; };
template <typename A> struct col_arg<A> { using type = A; };
template <typename A, typename B, typename... X> struct col_arg<A, B, X...> : col_arg<B, X...> {};
// the points of step t, p -> q, against whichever test `c` is (the grid has no time axis)
__device__ __forceinline__ bool col_seg(const KmpcCol& c, int, double, double px, double py, double qx, double qy) { return c.seg(px, py, qx, qy); }
__device__ __forceinline__ bool col_seg(const KmpcObs& c, int t, double dt, double px, double py, double qx, double qy) { return c.seg_t(t, dt, px, py, qx, qy); }

// The ego's live slots -> LDS, by the workgroup's first wave (all of its lanes call; M <= 64).  A slot is dropped when even the
// fastest ego and the disc heading straight for each other cannot meet within the horizon:  |o - p_0| - r - |v_o| T dt > reach,  reach =
// max(|v_0|, |max_speed|, |min_speed|) T dt  (the first step runs at v_0, every later one inside the speed bounds; 1e-9 of slack for the
// roundings).  Only for tame operands: with a non-finite or beyond-1e100 value in the slot or in the ego's state (x, y, v, yaw: a NaN speed or
// heading makes every tested point NaN, which any live slot blocks) every live slot is kept.  live64: (x, y, vx, vy, r r).  live32 (nullable, the f32 filter's table): the centre relative to the ego and the
// velocity, in the filter's frame (iso: rotated by -yaw0), and the FREE threshold (r + eps)^2 rounded up, eps as DESIGN.md 5j derives it:
// F1P_K4_POS_ERR_REL x reach for the filter's position + 16 x 2^-24 x (|o_rel|_1 + |v|_1 T dt + r + reach) for the roundings of the
// obstacle's side.  pos_err >= 0 replaces the first term by an absolute bound [m]: the dynamic model's grows with T^2 (k_stmpc.hip
// st_pos_err_bound).  Returns nothing: *n_out holds the count after the caller's barrier.
__device__ __forceinline__ void obs_compact(const KmpcObs& ob, int e, double sx, double sy, double sv, double syaw, int T, double dt, double max_speed,
                                            double min_speed, bool iso, double c0, double s0, double* live64, float* live32, int* n_out, double pos_err = -1.0) {
    const int lane = threadIdx.x;
    bool keep = false;
    double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0, r = 0.0;
    const double Tdt = (double)T * dt, reach = fmax(fabs(sv), fmax(fabs(max_speed), fabs(min_speed))) * Tdt;
    if (lane < ob.M) {
        const double* o = ob.obs + ((size_t)e * ob.M + lane) * 5;
        x = o[0]; y = o[1]; vx = o[2]; vy = o[3]; r = o[4];
        if (r >= 0.0) {
            const double dx = x - sx, dy = y - sy;
            const bool tame = fabs(x) < 1.0e100 && fabs(y) < 1.0e100 && fabs(vx) < 1.0e100 && fabs(vy) < 1.0e100 && r < 1.0e100 && fabs(sx) < 1.0e100 && fabs(sy) < 1.0e100 &&
                              fabs(sv) < 1.0e100 && fabs(syaw) < 1.0e100;      // (a NaN fails every one of these)
            const bool far = tame && sqrt(dx * dx + dy * dy) - r - sqrt(vx * vx + vy * vy) * Tdt > reach * (1.0 + 1.0e-9) + 1.0e-9;
            keep = !far;
        }
    }
    const unsigned long long votes = __ballot(keep);
    if (keep) {
        const int pos = __popcll(votes & ((1ull << lane) - 1ull));
        live64[5 * pos] = x; live64[5 * pos + 1] = y; live64[5 * pos + 2] = vx; live64[5 * pos + 3] = vy; live64[5 * pos + 4] = r * r;
        if (live32) {
            const double dx = x - sx, dy = y - sy;
            const double rx = iso ? c0 * dx + s0 * dy : dx, ry = iso ? c0 * dy - s0 * dx : dy;
            const double wx = iso ? c0 * vx + s0 * vy : vx, wy = iso ? c0 * vy - s0 * vx : vy;
            const double S = (fabs(rx) + fabs(ry)) + (fabs(wx) + fabs(wy)) * Tdt + r + reach;
            const double rr = r + ((pos_err >= 0.0 ? pos_err : F1P_K4_POS_ERR_REL * reach) + F1P_K4_OBS_ERR_REL * S);
            live32[5 * pos] = (float)rx; live32[5 * pos + 1] = (float)ry; live32[5 * pos + 2] = (float)wx; live32[5 * pos + 3] = (float)wy;
            live32[5 * pos + 4] = (float)(rr * rr * (1.0 + 1.0e-6));               // (the rounding to f32 is inside the factor; NaN / inf: never FREE)
        }
    }
    if (lane == 0) *n_out = __popcll(votes);
}

// the f32 filter's side: a point is FREE against a slot only when its f32 distance from the f32 centre exceeds r + eps
// (used through ColTestObs below)
struct KmpcObsF {
    const float* live;                // LDS [n_live][5] (obs_compact)
    int n_live;
    int grid;                         // the occupancy test too (KmpcColF)
    float dt;
};

// What an f32 filter's rollout tests after every step (k_kmpc.hip kmpc_rollout_cost_f32x2_test, k_stmpc.hip stmpc_rollout_f32): nothing,
// the step's points in the clearance map, or the points against the discs and -- while of.grid -- in the map too.  The rollouts are
// templates over these; the two loops over a step's points stay in the rollouts' own text, once per value type (float / f1p_f2): handed
// to a function of these structs they come out with other instructions (LABNOTES.md R15).
struct ColTestNone {};
struct ColTestGrid { KmpcColF cf; };
struct ColTestObs { KmpcColF cf; KmpcObsF of; };       // (cf.n_sub / cf.inv_nsub are set with or without a grid)

}  // namespace f1p
