// shoot_col.h -- the occupancy test of the shooting MPCs' rollouts (f1p_kmpc_set_collision, f1p_stmpc_set_collision):
// one struct, one point test and one segment rule for k_kmpc.hip and k_stmpc.hip.
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
// (k_kmpc.hip kmpc_rollout_cost_f32x2_col, k_stmpc.hip stmpc_rollout_f32 with `cf`)
#define F1P_K4_CLEAR_CELLS 2.0
#define F1P_K4_POS_ERR_REL 1.0e-4
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

}  // namespace f1p
