// k_tracks.hip -- the waypoint trackers over a TRACK SET: every ego follows its own polyline (f1p_set_track_set).
//
// The reference builds one planner per vehicle and hands each its own waypoints per call (PurePursuitPlanner.plan(..., waypoints),
// pure_pursuit.py:85; StanleyPlanner.plan, stanley.py:114; LQRPlanner.plan, lqr.py:156; KMPCPlanner.plan, kinematic_mpc.py:115;
// STMPCPlanner.plan, dynamic_mpc.py:133).
// Here K polylines are stored back to back, struct-of-arrays fp64 like the context's raceline, with a table int32 [K][4] =
// (first row, rows, first 64-segment chunk box, 0).  Each kernel is the single-raceline kernel's mapping (one wave per ego; one
// workgroup per ego for the MPC reference) with a prologue: the ego's track id, then its table entry -- wave-uniform values, kept in
// SGPRs with readfirstlane -- and the track's base pointers offset by them.  The scan, the projection, the pursuit, the front-axle
// errors, the Riccati iteration and the reference extraction are the SAME device functions on the same operands, so each ego's
// outputs are bit-identical to the single-raceline kernel run on a context whose raceline is that ego's track.
// A track id outside [0, K) reads nothing of the set: NaN steer / speed (NaN rows for the MPC reference), nearest index -1,
// status F1P_ST_BAD_TRACK; the other egos are unaffected.
#include "f1p_internal.h"
#include "tracker_device.h"

namespace f1p {

// k_nearest over the track set: one wave per query, 4 queries per workgroup
__global__ __launch_bounds__(256) void k_nearest_tracks(const double* __restrict__ pts, const int32_t* __restrict__ track_id, int E,
                                                        TrackSetDev ts, double* __restrict__ proj, double* __restrict__ dist,
                                                        double* __restrict__ tout, int32_t* __restrict__ idx) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    TrackView tv;
    if (!track_of(ts, track_id, e, tv)) {
        if (lane == 0) {
            if (proj) { proj[2 * e] = __builtin_nan(""); proj[2 * e + 1] = __builtin_nan(""); }
            if (dist) dist[e] = __builtin_nan("");
            if (tout) tout[e] = __builtin_nan("");
            if (idx) idx[e] = -1;
        }
        return;
    }
    const double px = pts[2 * e], py = pts[2 * e + 1];
    double bd; int bi;
    nearest_scan_boxed(px, py, tv.x, tv.y, tv.box, tv.n, lane, 64, bd, bi);
    wave_argmin(bd, bi);
    if (lane == 0) {
        const SegProj s = seg_project(px, py, tv.x[bi], tv.y[bi], tv.x[bi + 1], tv.y[bi + 1]);
        if (proj) { proj[2 * e] = s.qx; proj[2 * e + 1] = s.qy; }
        if (dist) dist[e] = s.d;
        if (tout) tout[e] = s.t;
        if (idx) idx[e] = bi;
    }
}

// k_pure_pursuit over the track set: one wave per ego, 4 egos per workgroup
__global__ __launch_bounds__(256) void k_pure_pursuit_tracks(const double* __restrict__ poses, const int32_t* __restrict__ track_id, int E,
                                                             double lookahead, double wheelbase, double max_reacquire, TrackSetDev ts,
                                                             double* __restrict__ steer, double* __restrict__ speed,
                                                             int32_t* __restrict__ near_idx, int32_t* __restrict__ la_idx,
                                                             int32_t* __restrict__ status) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    TrackView tv;
    if (!track_of(ts, track_id, e, tv)) {
        if (lane == 0) {
            steer[e] = __builtin_nan("");
            speed[e] = __builtin_nan("");
            if (near_idx) near_idx[e] = -1;
            if (la_idx) la_idx[e] = F1P_LA_NONE;
            if (status) status[e] = F1P_ST_BAD_TRACK;
        }
        return;
    }
    const double px = poses[3 * e], py = poses[3 * e + 1], th = poses[3 * e + 2];
    double bd; int bi;
    nearest_scan_boxed(px, py, tv.x, tv.y, tv.box, tv.n, lane, 64, bd, bi);
    wave_argmin(bd, bi);
    const SegProj s = seg_project(px, py, tv.x[bi], tv.y[bi], tv.x[bi + 1], tv.y[bi + 1]);
    const Track o = wave_pursuit(px, py, th, lookahead, wheelbase, max_reacquire, tv.x, tv.y, tv.v, 0.0, tv.n, bi, s.t, s.d);
    if (lane == 0) {
        steer[e] = o.steer;
        speed[e] = o.speed;
        if (near_idx) near_idx[e] = bi;
        if (la_idx) la_idx[e] = o.la_idx;
        if (status) status[e] = o.status;
    }
}

// k_stanley over the track set: one wave per ego
__global__ __launch_bounds__(256) void k_stanley_tracks(const double* __restrict__ states, const int32_t* __restrict__ track_id, int E,
                                                        double wheelbase, double k_path, TrackSetDev ts, double* __restrict__ steer,
                                                        double* __restrict__ speed, int32_t* __restrict__ near_idx) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    TrackView tv;
    if (!track_of(ts, track_id, e, tv)) {
        if ((threadIdx.x & 63) == 0) {
            steer[e] = __builtin_nan("");
            speed[e] = __builtin_nan("");
            if (near_idx) near_idx[e] = -1;
        }
        return;
    }
    const FrontErr fe = front_axle_errors(states[4 * e], states[4 * e + 1], states[4 * e + 2], wheelbase, tv.x, tv.y, tv.psi, tv.box, tv.n);
    if ((threadIdx.x & 63) == 0) {
        const double cte_front = atan2(k_path * fe.ef, states[4 * e + 3]);   // stanley.py:110
        steer[e] = cte_front + fe.theta_e;                                   // :111
        speed[e] = tv.v[fe.idx];
        if (near_idx) near_idx[e] = fe.idx;
    }
}

// k_lqr over the track set: phase 1 resolves the front-axle errors wave by wave (each ego on its own track), phase 2 iterates the
// Riccati recursion with one thread per ego.  An ego with a bad track id keeps its err untouched.
__global__ __launch_bounds__(256) void k_lqr_tracks(const double* __restrict__ states, const int32_t* __restrict__ track_id, double* __restrict__ err,
                                                    int E, LqrParams p, TrackSetDev ts, double* __restrict__ steer,
                                                    double* __restrict__ speed, int32_t* __restrict__ near_idx) {
    __shared__ double s_ef[256], s_te[256];
    __shared__ int s_idx[256], s_row[256];
    const int e_base = blockIdx.x * 256, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < 64; ++q) {                           // phase 1: each wave resolves 64 egos, one after the other
        const int k = wave * 64 + q, eq = e_base + k;
        if (eq >= E) break;                                  // wave-uniform
        TrackView tv;
        if (!track_of(ts, track_id, eq, tv)) {
            if (lane == 0) { s_ef[k] = 0.0; s_te[k] = 0.0; s_idx[k] = -1; s_row[k] = 0; }
            continue;
        }
        const FrontErr f = front_axle_errors(states[4 * eq], states[4 * eq + 1], states[4 * eq + 2], p.wheelbase, tv.x, tv.y, tv.psi, tv.box, tv.n);
        if (lane == 0) { s_ef[k] = f.ef; s_te[k] = f.theta_e; s_idx[k] = f.idx; s_row[k] = tv.off + f.idx; }
    }
    __syncthreads();
    const int e = e_base + threadIdx.x;                      // phase 2: one thread per ego
    if (e < E) {
        if (s_idx[threadIdx.x] < 0) {
            steer[e] = __builtin_nan("");
            speed[e] = __builtin_nan("");
            if (near_idx) near_idx[e] = -1;
            return;
        }
        FrontErr fe;
        fe.ef = s_ef[threadIdx.x]; fe.theta_e = s_te[threadIdx.x]; fe.idx = s_idx[threadIdx.x];
        const int row = s_row[threadIdx.x];                  // the nearest row in the concatenated set
        const double v = states[4 * e + 3];
        const double e_old = err[2 * e], th_old = err[2 * e + 1];                               // lqr.py:136-137
        const double A[16] = {1.0, p.ts, 0, 0, 0, 0, v, 0, 0, 0, 1.0, p.ts, 0, 0, 0, 0};      // update_matrix utils.py:227-233
        const double B[4] = {0, 0, 0, v / p.wheelbase};                                         // :236-237
        double K[4];
        solve_lqr4(A, B, p.q, p.r, p.eps, p.max_iter, K);
        const double s0 = fe.ef, s1 = (fe.ef - e_old) / p.ts, s2 = fe.theta_e, s3 = (fe.theta_e - th_old) / p.ts;   // :150-153
        const double fb = ((K[0] * s0 + K[1] * s1) + K[2] * s2) + K[3] * s3;                   // :155
        steer[e] = fb + ts.kappa[row] * p.wheelbase;                                           // :158-161
        speed[e] = ts.v[row];
        err[2 * e] = fe.ef; err[2 * e + 1] = fe.theta_e;                                        // :100-101
        if (near_idx) near_idx[e] = fe.idx;
    }
}

// k_kmpc_ref over the track set: one workgroup per ego.  states [E][4] = (x, y, v, yaw) -> ref [E][4][T+1]
__global__ __launch_bounds__(256) void k_kmpc_ref_tracks(const double* __restrict__ states, const int32_t* __restrict__ track_id, int E, int T,
                                                         double dt, double dl, TrackSetDev ts, int yaw_fixup, double* __restrict__ ref) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int e = blockIdx.x;
    if (e >= E) return;
    TrackView tv;
    if (!track_of(ts, track_id, e, tv)) {                    // workgroup-uniform
        double* r = ref + (size_t)e * 4 * (T + 1);
        for (int j = threadIdx.x; j < 4 * (T + 1); j += blockDim.x) r[j] = __builtin_nan("");
        return;
    }
    const double px = states[4 * e], py = states[4 * e + 1], v = states[4 * e + 2], yaw = states[4 * e + 3];
    double bd; int ind;
    nearest_scan_boxed(px, py, tv.x, tv.y, tv.box, tv.n, threadIdx.x, blockDim.x, bd, ind);   // :180
    block_argmin(bd, ind, sd, si);
    kmpc_ref_rows(v, yaw, ind, e, T, dt, dl, tv.x, tv.y, tv.v, tv.psi, tv.n, yaw_fixup, ref);   // :189-205
}

// k_stmpc_ref over the track set: one workgroup per ego.  states [E][4] = (x, y, v, yaw) -> ref [E][7][T+1] rows x, y, 0, v, yaw, 0, 0
// (calc_ref_trajectory dynamic_mpc.py:195-233; with (TK, DTK, dlk) STMPC's calc_ref_trajectory_kinematic :237-276, rows 0, 1, 3, 4).
// The statements of k_stmpc_ref (k_stmpc.hip) on the ego's track; that kernel keeps its own copy.
__global__ __launch_bounds__(256) void k_stmpc_ref_tracks(const double* __restrict__ states, const int32_t* __restrict__ track_id, int E, int T,
                                                          double dt, double dl, TrackSetDev ts, double* __restrict__ ref) {
    __shared__ double sd[4];
    __shared__ int si[4];
    const int e = blockIdx.x;
    if (e >= E) return;
    double* r = ref + (size_t)e * 7 * (T + 1);
    TrackView tv;
    if (!track_of(ts, track_id, e, tv)) {                    // workgroup-uniform
        for (int j = threadIdx.x; j < 7 * (T + 1); j += blockDim.x) r[j] = __builtin_nan("");
        return;
    }
    const double px = states[4 * e], py = states[4 * e + 1], v = states[4 * e + 2], yaw = states[4 * e + 3];
    double bd; int ind;
    nearest_scan_boxed(px, py, tv.x, tv.y, tv.box, tv.n, threadIdx.x, blockDim.x, bd, ind);
    block_argmin(bd, ind, sd, si);
    const int n = tv.n;
    const double dind = (fabs(v) * dt) / dl;
    for (int j = threadIdx.x; j <= T; j += blockDim.x) {
        double cum = 0.0;
        for (int q = 0; q < j; ++q) cum += dind;
        int il = ind + (int)cum;
        if (il >= n) il -= n;
        if (il < 0 || il >= n) il = il < 0 ? 0 : n - 1;
        double cyw = tv.psi[il];
        if (cyw - yaw > 5) cyw = fabs(cyw - (2 * F1P_PI));      // :227
        if (cyw - yaw < -5) cyw = fabs(cyw + (2 * F1P_PI));     // :228
        r[0 * (T + 1) + j] = tv.x[il];
        r[1 * (T + 1) + j] = tv.y[il];
        r[2 * (T + 1) + j] = 0.0;
        r[3 * (T + 1) + j] = tv.v[il];
        r[4 * (T + 1) + j] = cyw;
        r[5 * (T + 1) + j] = 0.0;
        r[6 * (T + 1) + j] = 0.0;
    }
}

TrackSetDev track_set_dev(const f1p_ctx* ctx) {
    TrackSetDev ts;
    ts.x = ctx->d_tx; ts.y = ctx->d_ty; ts.v = ctx->d_tv;
    ts.psi = ctx->trk_has_psi ? ctx->d_tpsi : nullptr;
    ts.kappa = ctx->trk_has_kappa ? ctx->d_tkappa : nullptr;
    ts.box = ctx->d_tbox;
    ts.tab = (const int4*)ctx->d_ttab;
    ts.K = ctx->trk_K;
    return ts;
}

int launch_nearest_tracks(f1p_ctx* ctx, const double* d_pts, const int32_t* d_tid, int E, double* d_proj, double* d_dist, double* d_t,
                          int32_t* d_idx) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_nearest_tracks, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_pts, d_tid, E, track_set_dev(ctx), d_proj, d_dist,
                       d_t, d_idx);
    return check_hip(ctx, hipGetLastError(), "k_nearest_tracks launch");
}

int launch_pure_pursuit_tracks(f1p_ctx* ctx, const double* d_poses, const int32_t* d_tid, int E, double lookahead, double wheelbase,
                               double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near, int32_t* d_la, int32_t* d_status) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_pure_pursuit_tracks, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_poses, d_tid, E, lookahead, wheelbase,
                       max_reacquire, track_set_dev(ctx), d_steer, d_speed, d_near, d_la, d_status);
    return check_hip(ctx, hipGetLastError(), "k_pure_pursuit_tracks launch");
}

int launch_stanley_tracks(f1p_ctx* ctx, const double* d_states, const int32_t* d_tid, int E, double wheelbase, double k_path,
                          double* d_steer, double* d_speed, int32_t* d_near) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_stanley_tracks, dim3((E + 3) / 4), dim3(256), 0, ctx->stream, d_states, d_tid, E, wheelbase, k_path,
                       track_set_dev(ctx), d_steer, d_speed, d_near);
    return check_hip(ctx, hipGetLastError(), "k_stanley_tracks launch");
}

int launch_lqr_tracks(f1p_ctx* ctx, const double* d_states, const int32_t* d_tid, double* d_err, int E, double wheelbase, double ts,
                      const double* q, double r, int max_iter, double eps, double* d_steer, double* d_speed, int32_t* d_near) {
    if (E <= 0) return F1P_OK;
    LqrParams p;
    p.wheelbase = wheelbase; p.ts = ts; p.r = r; p.eps = eps; p.max_iter = max_iter;
    for (int i = 0; i < 4; ++i) p.q[i] = q[i];
    hipLaunchKernelGGL(k_lqr_tracks, dim3((E + 255) / 256), dim3(256), 0, ctx->stream, d_states, d_tid, d_err, E, p, track_set_dev(ctx),
                       d_steer, d_speed, d_near);
    return check_hip(ctx, hipGetLastError(), "k_lqr_tracks launch");
}

int launch_kmpc_ref_tracks(f1p_ctx* ctx, const double* d_states, const int32_t* d_tid, int E, int horizon, double dt, double dl, double* d_ref) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_kmpc_ref_tracks, dim3(E), dim3(256), 0, ctx->stream, d_states, d_tid, E, horizon, dt, dl, track_set_dev(ctx),
                       ctx->kmpc_yaw_fixup, d_ref);
    return check_hip(ctx, hipGetLastError(), "k_kmpc_ref_tracks launch");
}

int launch_stmpc_ref_tracks(f1p_ctx* ctx, const double* d_states, const int32_t* d_tid, int E, int horizon, double dt, double dl, double* d_ref) {
    if (E <= 0) return F1P_OK;
    hipLaunchKernelGGL(k_stmpc_ref_tracks, dim3(E), dim3(256), 0, ctx->stream, d_states, d_tid, E, horizon, dt, dl, track_set_dev(ctx), d_ref);
    return check_hip(ctx, hipGetLastError(), "k_stmpc_ref_tracks launch");
}

}  // namespace f1p
