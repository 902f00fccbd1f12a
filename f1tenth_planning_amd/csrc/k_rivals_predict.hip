// k_rivals_predict.hip -- the rivals' slots predicted ALONG THE COURSE each rival follows (include/f1p.h "Rivals, predicted along the course",
// DESIGN.md 5n): after k_rivals has chosen the vehicles and written the constant-velocity slots, (vx, vy, r) of every live slot become the chord
// of the rival's path along its polyline over the ego's horizon, and the radius optionally grows by the path's largest distance from that chord.
//
//   k_course_arc      one wave per course: the cumulative arc length cum [n] and the "usable" flag.  64 segment lengths are formed in parallel
//                     (coalesced), then added ONE BY ONE in index order (v_readlane of lane 0, 1, ... 63): the table is the sequential fp64 sum,
//                     whatever the launch shape.  Runs once per raceline / track set (generation counters on the context).
//   k_rivals_frenet   one wave per vehicle: nearest segment of ITS course with the scan, argmin and projection of k_nearest / k_nearest_tracks
//                     (the same device functions on the same operands: (b, t, q) are those calls' bits), then the record (s0, d, dir, b).
//                     A vehicle that cannot be predicted -- non-finite state, track id outside the set, unusable course -- gets a NaN record.
//   k_rivals_predict  one wave per ego.  The (slot, knot) pairs are spread over the lanes in groups of G = 16 (K + 1 <= 16) or 32 lanes per slot;
//                     a lane finds its knot's segment by BINARY search in cum, the group's knots 0 and K are fetched by ds_bpermute and the
//                     deviation is reduced by an xor butterfly inside the group; the group's lane 0 overwrites (vx, vy, r).  No LDS, no atomics;
//                     the loads sit in divergent code, every cross-lane operation in code the whole wave runs.  A slot that falls back is not
//                     touched: it keeps the bits k_rivals wrote, and nothing is indexed with a value that failed a test.
#include "f1p_internal.h"
#include "tracker_device.h"

namespace f1p {

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __builtin_huge_val(); }

__global__ __launch_bounds__(64) void k_course_arc(const double* __restrict__ x, const double* __restrict__ y, const int4* __restrict__ tab, int n,
                                                   double* __restrict__ cum, int32_t* __restrict__ ok) {
    const int k = blockIdx.x, lane = threadIdx.x;
    int off = 0, rows = n;
    if (tab) { const int4 t = tab[k]; off = __builtin_amdgcn_readfirstlane(t.x); rows = __builtin_amdgcn_readfirstlane(t.y); }
    x += off; y += off; cum += off;
    double acc = 0.0;
    bool good = true;
    if (lane == 0 && rows > 0) cum[0] = 0.0;
    for (int base = 0; base < rows - 1; base += 64) {                 // (wave-uniform)
        const int i = base + lane;
        double len = 0.0;                                             // past the end: + 0.0 leaves the sum's bits alone
        if (i < rows - 1) {
            const double dx = x[i + 1] - x[i], dy = y[i + 1] - y[i];
            len = __builtin_sqrt(dx * dx + dy * dy);
            if (!(len > 0.0)) good = false;                           // zero length, or NaN
        }
        const int lo = __double2loint(len), hi = __double2hiint(len);
        double mine = 0.0;
#pragma unroll 4
        for (int l = 0; l < 64; ++l) {                                // (a rolled loop: 128 hoisted v_readlane results would not fit the SGPRs)
            acc = acc + __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
            if (lane == l) mine = acc;
        }
        if (i < rows - 1) cum[i + 1] = mine;
    }
    const bool all_good = __ballot(!good) == 0ull;
    if (lane == 0) ok[k] = (rows >= 2 && all_good && acc > 0.0 && acc < __builtin_huge_val()) ? 1 : 0;
}

// the courses of a rivals call: track tid[j] of the set for vehicle j, or (tid null) the raceline for all
struct CourseDev {
    TrackSetDev ts;
    const int32_t* tid;
    const double *wx, *wy, *wbox;
    int n;
    const double* cum;                                                // k_course_arc's table, rows as the course arrays'
    const int32_t* ok;                                                // [K] / [1]
};

__global__ __launch_bounds__(256) void k_rivals_frenet(const double* __restrict__ st, int stride, int iv, int ih, int ib, int E, CourseDev c,
                                                       double* __restrict__ rec, double* __restrict__ frenet) {
    const int lane = threadIdx.x & 63;
    const int j = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (j >= E) return;                                               // (the whole wave)
    const double* s = st + (size_t)j * stride;
    const double x = s[0], y = s[1], v = s[iv];
    double h = s[ih];
    if (ib >= 0) h = h + s[ib];
    TrackView tv;
    const double* cum = nullptr;
    bool usable = false;
    if (c.tid) {
        if (track_of(c.ts, c.tid, j, tv)) {                           // (false: an id outside [0, K), nothing of the set is read)
            cum = c.cum + tv.off;
            usable = c.ok[__builtin_amdgcn_readfirstlane(c.tid[j])] != 0;
        }
    } else {
        tv.x = c.wx; tv.y = c.wy; tv.v = nullptr; tv.psi = nullptr; tv.kappa = nullptr; tv.box = c.wbox; tv.n = c.n; tv.off = 0;
        cum = c.cum;
        usable = c.ok[0] != 0;
    }
    const double nan = __builtin_nan("");
    double s0 = nan, d = nan, dir = nan, bb = -1.0;
    // every lane holds the same vehicle: the branch is taken by the whole wave or by none of it (the scan ballots)
    if (usable && finite_d(x) && finite_d(y) && finite_d(v) && finite_d(h)) {
        double bd; int bi;
        nearest_scan_boxed(x, y, tv.x, tv.y, tv.box, tv.n, lane, 64, bd, bi);
        wave_argmin(bd, bi);
        if (bi >= 0 && bi < tv.n - 1) {
            const double ax = tv.x[bi], ay = tv.y[bi], bx = tv.x[bi + 1], by = tv.y[bi + 1];
            const SegProj p = seg_project(x, y, ax, ay, bx, by);
            const double dx = bx - ax, dy = by - ay;
            const double len = __builtin_sqrt(dx * dx + dy * dy);
            const double ux = dx / len, uy = dy / len;
            double sn, cs;
            sincos(h, &sn, &cs);                                      // full range, as k_rivals
            s0 = cum[bi] + p.t * len;
            d = (x - p.qx) * (-uy) + (y - p.qy) * ux;
            dir = (v * (cs * ux + sn * uy) >= 0.0) ? 1.0 : -1.0;
            bb = (double)bi;
        }
    }
    if (lane == 0) {
        double* r = rec + 4 * (size_t)j;
        r[0] = s0; r[1] = d; r[2] = dir; r[3] = bb;
        if (frenet) { frenet[3 * (size_t)j] = s0; frenet[3 * (size_t)j + 1] = d; frenet[3 * (size_t)j + 2] = dir; }
    }
}

__global__ __launch_bounds__(256) void k_rivals_predict(const double* __restrict__ st, int stride, int iv, int E, int M, double radius, double min_speed,
                                                        double hs, double hm, int K, int inflate, int wrap, CourseDev c,
                                                        const double* __restrict__ rec, const int32_t* __restrict__ idx, double* __restrict__ obs) {
    const int lane = threadIdx.x & 63;
    const int e = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (e >= E) return;                                               // (the whole wave)
    double a = fabs(st[(size_t)e * stride + iv]);                     // the ego's pace, k_rivals' own expression
    if (!(a >= min_speed)) a = (a != a) ? a : min_speed;
    const double pace = 1.0 / a;
    const double H = hs + hm * pace;
    if (!(H > 0.0) || !(H < __builtin_huge_val())) return;            // (the whole wave: every slot of this ego stays constant-velocity)
    const int G = (K + 1 <= 16) ? 16 : 32, per = 64 / G;              // lanes per slot, slots per pass
    const int g = lane / G, kn = lane & (G - 1), base = lane & ~(G - 1);
    for (int m0 = 0; m0 < M; m0 += per) {                             // (wave-uniform)
        const int m = m0 + g;
        bool live = false;
        double cx = 0.0, cy = 0.0;
        if (m < M && kn <= K) {
            const int j = idx[(size_t)e * M + m];
            if (j >= 0 && j < E) {
                const double* r = rec + 4 * (size_t)j;
                const double dir = r[2];
                const double av = fabs(st[(size_t)j * stride + iv]);
                if (dir == dir && av * H < 1.0e9) {                   // (a NaN record: the vehicle falls back, its course is not looked up)
                    const double *px = c.wx, *py = c.wy, *cum = c.cum;
                    int n = c.n;
                    if (c.tid) {
                        const int4 t = c.ts.tab[c.tid[j]];            // (in [0, K): k_rivals_frenet wrote a record)
                        px = c.ts.x + t.x; py = c.ts.y + t.x; cum = c.cum + t.x; n = t.y;
                    }
                    const double L = cum[n - 1];
                    const double tau = (H * (double)kn) / (double)K;
                    double sa = r[0] + (dir * av) * tau;
                    if (wrap) sa = sa - L * floor(sa / L);
                    if (sa < 0.0) sa = 0.0;
                    if (sa > L) sa = L;
                    int lo = 0, hi = n - 2;                           // the largest k <= n - 2 with cum_k <= s (cum_0 = 0 <= s)
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (cum[mid] <= sa) lo = mid; else hi = mid - 1;
                    }
                    const double ax = px[lo], ay = py[lo];
                    const double dx = px[lo + 1] - ax, dy = py[lo + 1] - ay;
                    const double len = __builtin_sqrt(dx * dx + dy * dy);
                    const double ux = dx / len, uy = dy / len;
                    const double w = sa - cum[lo], d = r[1];
                    cx = ax + ux * w + (-uy) * d;
                    cy = ay + uy * w + ux * d;
                    live = true;
                }
            }
        }
        // every lane of the wave from here to the store
        const double c0x = shfl_d(cx, base), c0y = shfl_d(cy, base), cKx = shfl_d(cx, base + K), cKy = shfl_d(cy, base + K);
        double dev = 0.0;
        if (live && kn > 0 && kn < K) {
            const double f = (double)kn / (double)K;
            const double ex = (cx - c0x) - (cKx - c0x) * f, ey = (cy - c0y) - (cKy - c0y) * f;
            dev = __builtin_sqrt(ex * ex + ey * ey);
        }
        for (int mask = G >> 1; mask >= 1; mask >>= 1) dev = __builtin_fmax(dev, shfl_xor_d(dev, mask));
        if (live && kn == 0) {
            double* q = obs + ((size_t)e * M + m) * 5;
            q[2] = (cKx - c0x) / H;
            q[3] = (cKy - c0y) / H;
            if (inflate) q[4] = radius + dev;
        }
    }
}

// layout -> (stride, speed column, heading column, column added to the heading or -1), as launch_rivals
static void layout_columns(int layout, int* stride, int* iv, int* ih, int* ib) {
    *stride = layout == F1P_RIVALS_ST7 ? 7 : 4;
    *iv = layout == F1P_RIVALS_XYVYAW ? 2 : 3;
    *ih = layout == F1P_RIVALS_XYVYAW ? 3 : layout == F1P_RIVALS_POSE ? 2 : 4;
    *ib = layout == F1P_RIVALS_ST7 ? 6 : -1;
}

int launch_course_arc(f1p_ctx* ctx, bool tracks, double* d_cum, int32_t* d_ok) {
    if (tracks)
        hipLaunchKernelGGL(k_course_arc, dim3(ctx->trk_K), dim3(64), 0, ctx->stream, ctx->d_tx, ctx->d_ty, (const int4*)ctx->d_ttab, 0, d_cum, d_ok);
    else
        hipLaunchKernelGGL(k_course_arc, dim3(1), dim3(64), 0, ctx->stream, ctx->d_wx, ctx->d_wy, (const int4*)nullptr, ctx->n_wp, d_cum, d_ok);
    return check_hip(ctx, hipGetLastError(), "k_course_arc launch");
}

int launch_rivals_predict(f1p_ctx* ctx, const double* d_states, int layout, int E, int M, double radius, double min_speed,
                          const f1p_rivals_predict* pr, const int32_t* d_tid, const double* d_cum, const int32_t* d_ok, double* d_rec,
                          const int32_t* d_idx, double* d_obs, double* d_frenet) {
    if (E <= 0) return F1P_OK;
    int stride, iv, ih, ib;
    layout_columns(layout, &stride, &iv, &ih, &ib);
    CourseDev c;
    c.ts = track_set_dev(ctx);
    c.tid = d_tid;
    c.wx = ctx->d_wx; c.wy = ctx->d_wy; c.wbox = ctx->d_wbox; c.n = ctx->n_wp;
    c.cum = d_cum; c.ok = d_ok;
    hipLaunchKernelGGL(k_rivals_frenet, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, stride, iv, ih, ib, E, c, d_rec, d_frenet);
    if (const int rc = check_hip(ctx, hipGetLastError(), "k_rivals_frenet launch")) return rc;
    hipLaunchKernelGGL(k_rivals_predict, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, stride, iv, E, M, radius, min_speed, pr->horizon_s,
                       pr->horizon_m, (int)pr->knots, (int)pr->inflate, (int)pr->wrap, c, (const double*)d_rec, d_idx, d_obs);
    return check_hip(ctx, hipGetLastError(), "k_rivals_predict launch");
}

}  // namespace f1p
