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
//   k_course_time     (speed = profile) k_course_arc's sibling for the course's TIME coordinate tim [n] and the "profile-usable" flag;
//                     k_rivals_predict<CourseTime> then advances a rival in tim, scaled by its speed relative to the course's where it stands.
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

// The time coordinate of the same courses (include/f1p.h "Rivals, predicted with the course's speed profile"): tim_{k+1} = tim_k +
// len_k / c_k with c_k the mean of the two |speeds| of segment k, floored at vfloor.  k_course_arc's sibling: the 64 quotients are formed in parallel
// and added ONE BY ONE in index order, so the table is the sequential fp64 sum whatever the launch shape.  pok [k]: the course is usable (ok, written
// by k_course_arc earlier on the stream), every speed is finite, and the lap time is finite and positive.
__global__ __launch_bounds__(64) void k_course_time(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ w,
                                                    const int4* __restrict__ tab, int n, double vfloor, const int32_t* __restrict__ ok,
                                                    double* __restrict__ tim, int32_t* __restrict__ pok) {
    const int k = blockIdx.x, lane = threadIdx.x;
    int off = 0, rows = n;
    if (tab) { const int4 t = tab[k]; off = __builtin_amdgcn_readfirstlane(t.x); rows = __builtin_amdgcn_readfirstlane(t.y); }
    x += off; y += off; w += off; tim += off;
    double acc = 0.0;
    bool good = true;
    if (lane == 0 && rows > 0) tim[0] = 0.0;
    for (int base = 0; base < rows - 1; base += 64) {                 // (wave-uniform)
        const int i = base + lane;
        double q = 0.0;                                               // past the end: + 0.0 leaves the sum's bits alone
        if (i < rows - 1) {
            const double dx = x[i + 1] - x[i], dy = y[i + 1] - y[i];
            const double len = __builtin_sqrt(dx * dx + dy * dy);     // (k_course_arc's expression: the same bits)
            const double w0 = w[i], w1 = w[i + 1];
            if (!finite_d(w0) || !finite_d(w1)) good = false;
            double c = 0.5 * (fabs(w0) + fabs(w1));
            if (!(c >= vfloor)) c = vfloor;
            q = len / c;
        }
        const int lo = __double2loint(q), hi = __double2hiint(q);
        double mine = 0.0;
#pragma unroll 4
        for (int l = 0; l < 64; ++l) {
            acc = acc + __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
            if (lane == l) mine = acc;
        }
        if (i < rows - 1) tim[i + 1] = mine;
    }
    const bool all_good = __ballot(!good) == 0ull;
    if (lane == 0) pok[k] = (ok[k] != 0 && all_good && acc > 0.0 && acc < __builtin_huge_val()) ? 1 : 0;
}

// what the profile instantiation of k_rivals_predict reads on top of CourseDev: k_course_time's table (rows as the course arrays'), its flags
// [K] / [1], and the speed columns of the raceline and of the track set
struct CourseTime {
    const double* tim;
    const int32_t* pok;
    const double *wv, *tv;
};

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

// The start of vehicle j in the TIME coordinate of its course (cum, n), from its record r = (s0, d, dir, b): the table to search (tim), th0, rho and the
// course's speed column.  false, with nothing of the time table read and the outputs untouched: the course is not profile-usable.  b is a segment of
// this course (k_rivals_frenet wrote dir and b together, and dir is not NaN here); it is tested all the same, so that no load is indexed without a test.
__device__ __forceinline__ bool profile_start(const CourseTime& ct, const CourseDev& c, int j, const double* __restrict__ r, double av, double vfloor,
                                              const double* __restrict__ cum, int n, const double*& tab, double& th0, double& rho, const double*& spd) {
    const double *tim = ct.tim, *pw = ct.wv;
    int course = 0;
    if (c.tid) {
        course = c.tid[j];                                            // (in [0, K): k_rivals_frenet wrote a record)
        const int off = c.ts.tab[course].x;
        tim += off; pw = ct.tv + off;
    }
    if (ct.pok[course] == 0) return false;
    const int b = (int)r[3];
    if (b < 0 || b > n - 2) return false;
    double cb = 0.5 * (fabs(pw[b]) + fabs(pw[b + 1]));
    if (!(cb >= vfloor)) cb = vfloor;
    rho = av / cb;
    th0 = tim[b] + (r[0] - cum[b]) / cb;
    tab = tim; spd = pw;
    return true;
}

// k_rivals_predict<>: speed = constant, the kernel as it was.  k_rivals_predict<CourseTime>: speed = profile -- the same walk in another coordinate: a
// lane whose vehicle's course is profile-usable starts at th0, advances at rho and searches tim instead of (s0, |v_j|, cum), then turns the time on the
// segment into metres with that segment's c_k, recomputed from the two speeds it loads; a lane on any other course keeps (s0, |v_j|, cum), which are
// the constant instantiation's expressions on the same operands.
template <typename... Prof>
__global__ __launch_bounds__(256) void k_rivals_predict(const double* __restrict__ st, int stride, int iv, int E, int M, double radius, double min_speed,
                                                        double hs, double hm, int K, int inflate, int wrap, CourseDev c,
                                                        const double* __restrict__ rec, const int32_t* __restrict__ idx, double* __restrict__ obs,
                                                        Prof... prof) {
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
                    // the table the knot is searched in, and the start and the speed in its coordinate: (cum, s0, |v_j|), or (tim, th0, rho)
                    const double* tab = cum;
                    [[maybe_unused]] double th0 = 0.0, rho = 0.0;
                    [[maybe_unused]] const double* spd = nullptr;     // the course's speed column: this lane follows the profile
                    if constexpr (sizeof...(Prof) > 0) (profile_start(prof, c, j, r, av, min_speed, cum, n, tab, th0, rho, spd), ...);
                    const double L = tab[n - 1];
                    const double tau = (H * (double)kn) / (double)K;
                    double sa = r[0] + (dir * av) * tau;
                    if constexpr (sizeof...(Prof) > 0) {
                        if (spd) sa = th0 + (dir * rho) * tau;
                    }
                    if (wrap) sa = sa - L * floor(sa / L);
                    if (sa < 0.0) sa = 0.0;
                    if (sa > L) sa = L;
                    int lo = 0, hi = n - 2;                           // the largest k <= n - 2 with tab_k <= s (tab_0 = 0 <= s)
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (tab[mid] <= sa) lo = mid; else hi = mid - 1;
                    }
                    const double ax = px[lo], ay = py[lo];
                    const double dx = px[lo + 1] - ax, dy = py[lo + 1] - ay;
                    const double len = __builtin_sqrt(dx * dx + dy * dy);
                    const double ux = dx / len, uy = dy / len;
                    double w = sa - tab[lo];
                    const double d = r[1];
                    if constexpr (sizeof...(Prof) > 0) {
                        if (spd) {                                    // time on the segment -> metres: c_lo, recomputed from its two speeds
                            double cl = 0.5 * (fabs(spd[lo]) + fabs(spd[lo + 1]));
                            if (!(cl >= min_speed)) cl = min_speed;
                            w = w * cl;
                        }
                    }
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

int launch_course_time(f1p_ctx* ctx, bool tracks, double min_speed, const int32_t* d_ok, double* d_tim, int32_t* d_pok) {
    if (tracks)
        hipLaunchKernelGGL(k_course_time, dim3(ctx->trk_K), dim3(64), 0, ctx->stream, ctx->d_tx, ctx->d_ty, ctx->d_tv, (const int4*)ctx->d_ttab, 0, min_speed,
                           d_ok, d_tim, d_pok);
    else
        hipLaunchKernelGGL(k_course_time, dim3(1), dim3(64), 0, ctx->stream, ctx->d_wx, ctx->d_wy, ctx->d_wv, (const int4*)nullptr, ctx->n_wp, min_speed,
                           d_ok, d_tim, d_pok);
    return check_hip(ctx, hipGetLastError(), "k_course_time launch");
}

int launch_rivals_predict(f1p_ctx* ctx, const double* d_states, int layout, int E, int M, double radius, double min_speed,
                          const f1p_rivals_predict* pr, const int32_t* d_tid, const double* d_cum, const int32_t* d_ok, const double* d_tim,
                          const int32_t* d_pok, double* d_rec, const int32_t* d_idx, double* d_obs, double* d_frenet) {
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
    if (pr->speed == F1P_RIVALS_SPEED_PROFILE) {
        const CourseTime ct{d_tim, d_pok, ctx->d_wv, ctx->d_tv};
        hipLaunchKernelGGL(k_rivals_predict<CourseTime>, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, stride, iv, E, M, radius, min_speed,
                           pr->horizon_s, pr->horizon_m, (int)pr->knots, (int)pr->inflate, (int)pr->wrap, c, (const double*)d_rec, d_idx, d_obs, ct);
    } else {
        hipLaunchKernelGGL(k_rivals_predict<>, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, stride, iv, E, M, radius, min_speed, pr->horizon_s,
                           pr->horizon_m, (int)pr->knots, (int)pr->inflate, (int)pr->wrap, c, (const double*)d_rec, d_idx, d_obs);
    }
    return check_hip(ctx, hipGetLastError(), "k_rivals_predict launch");
}

}  // namespace f1p
