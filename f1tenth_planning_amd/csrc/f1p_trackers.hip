// f1p_trackers.hip -- the host-pointer and device-pointer entry points of the trackers (nearest point, intersection, pure pursuit, Stanley, LQR),
// on the context's raceline and on its track set.  Each raceline / track-set pair of exported names has ONE body: `tracks` selects the track
// set, whose ids are one more staged array (right behind the states, where the *_tracks_batch calls always put it) and whose presence is
// tested with need_tracks instead of the raceline's waypoint test.  The error texts are each exported name's own.
#include "f1p_host.h"

using namespace f1p;

static int nearest_point_impl(f1p_ctx* ctx, const double* pts, const int32_t* track_id, bool tracks, int32_t E, double* proj, double* dist,
                              double* t, int32_t* idx) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!pts || (tracks && !track_id)))) return set_error(ctx, F1P_EINVAL, tracks ? "bad pts / track_id / E" : "bad pts / E");
    int rc;
    if (tracks) { if ((rc = need_tracks(ctx, false, false))) return rc; }
    else if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "waypoints not set");
    Stage s(ctx);
    s.need(sizeof(double) * 2 * E); s.need(sizeof(int32_t) * E, tracks); s.need(sizeof(double) * 2 * E, proj); s.need(sizeof(double) * E, dist);
    s.need(sizeof(double) * E, t); s.need(sizeof(int32_t) * E, idx);
    if ((rc = s.begin())) return rc;
    const double* d_pts; const int32_t* d_tid = nullptr;
    if ((rc = s.in(pts, (size_t)2 * E, &d_pts))) return rc;
    if (tracks && (rc = s.in(track_id, (size_t)E, &d_tid))) return rc;
    double* d_proj = s.out(proj, (size_t)2 * E); double* d_dist = s.out(dist, E); double* d_t = s.out(t, E);
    int32_t* d_idx = s.out(idx, E);
    if ((rc = tracks ? launch_nearest_tracks(ctx, d_pts, d_tid, E, d_proj, d_dist, d_t, d_idx)
                     : launch_nearest(ctx, d_pts, E, d_proj, d_dist, d_t, d_idx))) return rc;
    return s.finish();
}

// the checks and the launch of f1p_pure_pursuit[_tracks]_dev, behind F1P_ENTER (the *_batch body below has made its own)
static int pure_pursuit_dev_impl(f1p_ctx* ctx, const double* d_poses, const int32_t* d_track_id, bool tracks, int32_t E, double lookahead,
                                 double wheelbase, double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near_idx,
                                 int32_t* d_la_idx, int32_t* d_status) {
    if (E < 0 || (E > 0 && (!d_poses || (tracks && !d_track_id) || !d_steer || !d_speed)))
        return set_error(ctx, F1P_EINVAL, tracks ? "poses, track_id, steer and speed are required" : "poses, steer and speed are required");
    if (tracks) {
        const int rc = need_tracks(ctx, false, false); if (rc) return rc;
        return launch_pure_pursuit_tracks(ctx, d_poses, d_track_id, E, lookahead, wheelbase, max_reacquire, d_steer, d_speed, d_near_idx, d_la_idx,
                                          d_status);
    }
    if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "Please set waypoints to track during planner instantiation or when calling plan()");
    return launch_pure_pursuit(ctx, d_poses, E, lookahead, wheelbase, max_reacquire, d_steer, d_speed, d_near_idx, d_la_idx, d_status);
}

static int pure_pursuit_batch_impl(f1p_ctx* ctx, const double* poses, const int32_t* track_id, bool tracks, int32_t E, double lookahead,
                                   double wheelbase, double max_reacquire, double* steer, double* speed, int32_t* near_idx, int32_t* la_idx,
                                   int32_t* status) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!poses || (tracks && !track_id) || !steer || !speed)))
        return set_error(ctx, F1P_EINVAL, tracks ? "poses, track_id, steer and speed are required" : "poses, steer and speed are required");
    int rc;
    // a missing track set is reported before anything is staged; missing waypoints by pure_pursuit_dev_impl, behind the staging (the order
    // in which the two exported names have always made these tests)
    if (tracks && (rc = need_tracks(ctx, false, false))) return rc;
    Stage s(ctx);
    s.need(sizeof(double) * 3 * E); s.need(sizeof(int32_t) * E, tracks); s.need(sizeof(double) * E); s.need(sizeof(double) * E);
    s.need(sizeof(int32_t) * E, near_idx); s.need(sizeof(int32_t) * E, la_idx); s.need(sizeof(int32_t) * E, status);
    if ((rc = s.begin())) return rc;
    const double* d_poses; const int32_t* d_tid = nullptr;
    if ((rc = s.in(poses, (size_t)3 * E, &d_poses))) return rc;
    if (tracks && (rc = s.in(track_id, (size_t)E, &d_tid))) return rc;
    double* d_steer = s.out(steer, E); double* d_speed = s.out(speed, E);
    int32_t* d_n = s.out(near_idx, E); int32_t* d_l = s.out(la_idx, E); int32_t* d_s = s.out(status, E);
    if ((rc = pure_pursuit_dev_impl(ctx, d_poses, d_tid, tracks, E, lookahead, wheelbase, max_reacquire, d_steer, d_speed, d_n, d_l, d_s))) return rc;
    return s.finish();
}

static int stanley_impl(f1p_ctx* ctx, const double* states, const int32_t* track_id, bool tracks, int32_t E, double wheelbase, double k_path,
                        double* steer, double* speed, int32_t* near_idx) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!states || (tracks && !track_id) || !steer || !speed)))
        return set_error(ctx, F1P_EINVAL, tracks ? "states, track_id, steer and speed are required" : "states, steer and speed are required");
    int rc;
    if (tracks) { if ((rc = need_tracks(ctx, true, false))) return rc; }
    else {
        if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "Please set waypoints to track during planner instantiation or when calling plan()");
        if (!ctx->has_psi) return set_error(ctx, F1P_EINVAL, "Waypoints needs to be a (Nxm), m >= 4, numpy array!");   // stanley.py:131-132
    }
    Stage s(ctx);
    s.need(8 * 4 * (size_t)E); s.need(4 * (size_t)E, tracks); s.need(8 * (size_t)E); s.need(8 * (size_t)E); s.need(4 * (size_t)E, near_idx);
    if ((rc = s.begin())) return rc;
    const double* d_st; const int32_t* d_tid = nullptr;
    if ((rc = s.in(states, (size_t)4 * E, &d_st))) return rc;
    if (tracks && (rc = s.in(track_id, (size_t)E, &d_tid))) return rc;
    double* d_steer = s.out(steer, E); double* d_speed = s.out(speed, E); int32_t* d_n = s.out(near_idx, E);
    if ((rc = tracks ? launch_stanley_tracks(ctx, d_st, d_tid, E, wheelbase, k_path, d_steer, d_speed, d_n)
                     : launch_stanley(ctx, d_st, E, wheelbase, k_path, d_steer, d_speed, d_n))) return rc;
    return s.finish();
}

static int lqr_impl(f1p_ctx* ctx, const double* states, const int32_t* track_id, bool tracks, double* err, int32_t E, double wheelbase,
                    double timestep, const double q[4], double r, int32_t max_iter, double eps, double* steer, double* speed, int32_t* near_idx) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!states || (tracks && !track_id) || !err || !steer || !speed)) || !q)
        return set_error(ctx, F1P_EINVAL, tracks ? "states, track_id, err, q, steer and speed are required" : "states, err, q, steer and speed are required");
    if (!(timestep > 0.0) || !(wheelbase > 0.0) || max_iter < 0) return set_error(ctx, F1P_EINVAL, "timestep and wheelbase must be > 0, max_iter >= 0");
    int rc;
    if (tracks) { if ((rc = need_tracks(ctx, true, true))) return rc; }
    else {
        if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "Please set waypoints to track during planner instantiation or when calling plan()");
        if (!ctx->has_psi || !ctx->has_kappa) return set_error(ctx, F1P_EINVAL, "Waypoints needs to be a (Nxm), m >= 5, numpy array!");   // lqr.py:195-196
    }
    Stage s(ctx);
    s.need(8 * 4 * (size_t)E); s.need(4 * (size_t)E, tracks); s.need(8 * 2 * (size_t)E); s.need(8 * (size_t)E); s.need(8 * (size_t)E);
    s.need(4 * (size_t)E, near_idx);
    if ((rc = s.begin())) return rc;
    const double* d_st; const int32_t* d_tid = nullptr;
    if ((rc = s.in(states, (size_t)4 * E, &d_st))) return rc;
    if (tracks && (rc = s.in(track_id, (size_t)E, &d_tid))) return rc;
    const double* d_err_in;
    if ((rc = s.in((const double*)err, (size_t)2 * E, &d_err_in))) return rc;
    double* d_err = const_cast<double*>(d_err_in);
    if (E > 0) s.outs.push_back({(void*)err, (void*)d_err, sizeof(double) * 2 * (size_t)E});   // in/out
    double* d_steer = s.out(steer, E); double* d_speed = s.out(speed, E); int32_t* d_n = s.out(near_idx, E);
    if ((rc = tracks ? launch_lqr_tracks(ctx, d_st, d_tid, d_err, E, wheelbase, timestep, q, r, max_iter, eps, d_steer, d_speed, d_n)
                     : launch_lqr(ctx, d_st, d_err, E, wheelbase, timestep, q, r, max_iter, eps, d_steer, d_speed, d_n))) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------------
int f1p_nearest_point_batch(f1p_ctx* ctx, const double* pts, int32_t E, double* proj, double* dist, double* t, int32_t* idx) {
    return nearest_point_impl(ctx, pts, nullptr, false, E, proj, dist, t, idx);
}

int f1p_nearest_point_tracks_batch(f1p_ctx* ctx, const double* pts, const int32_t* track_id, int32_t E, double* proj, double* dist, double* t,
                                   int32_t* idx) {
    return nearest_point_impl(ctx, pts, track_id, true, E, proj, dist, t, idx);
}

int f1p_intersect_point_batch(f1p_ctx* ctx, const double* pts, const double* start_t, int32_t E, double radius,
                              int32_t wrap, double* first_p, int32_t* first_i, double* first_t, int32_t* found) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!pts || !start_t))) return set_error(ctx, F1P_EINVAL, "bad pts / start_t / E");
    if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "waypoints not set");
    for (int i = 0; i < E; ++i)
        if (!(start_t[i] >= 0.0) || !(start_t[i] <= (double)ctx->n_wp)) return set_error(ctx, F1P_EINVAL, "start_t must be in [0, n]");
    Stage s(ctx);
    s.need(sizeof(double) * 2 * E); s.need(sizeof(double) * E); s.need(sizeof(double) * 2 * E, first_p);
    s.need(sizeof(int32_t) * E, first_i); s.need(sizeof(double) * E, first_t); s.need(sizeof(int32_t) * E, found);
    int rc = s.begin(); if (rc) return rc;
    const double *d_pts, *d_st;
    if ((rc = s.in(pts, (size_t)2 * E, &d_pts))) return rc;
    if ((rc = s.in(start_t, (size_t)E, &d_st))) return rc;
    double* d_p = s.out(first_p, (size_t)2 * E); int32_t* d_i = s.out(first_i, E); double* d_t = s.out(first_t, E);
    int32_t* d_f = s.out(found, E);
    if ((rc = launch_intersect(ctx, d_pts, d_st, E, radius, wrap, d_p, d_i, d_t, d_f))) return rc;
    return s.finish();
}

int f1p_pure_pursuit_dev(f1p_ctx* ctx, const double* d_poses, int32_t E, double lookahead, double wheelbase,
                         double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near_idx,
                         int32_t* d_la_idx, int32_t* d_status) {
    F1P_ENTER(ctx);
    return pure_pursuit_dev_impl(ctx, d_poses, nullptr, false, E, lookahead, wheelbase, max_reacquire, d_steer, d_speed, d_near_idx, d_la_idx, d_status);
}

int f1p_pure_pursuit_tracks_dev(f1p_ctx* ctx, const double* d_poses, const int32_t* d_track_id, int32_t E, double lookahead, double wheelbase,
                                double max_reacquire, double* d_steer, double* d_speed, int32_t* d_near_idx, int32_t* d_la_idx,
                                int32_t* d_status) {
    F1P_ENTER(ctx);
    return pure_pursuit_dev_impl(ctx, d_poses, d_track_id, true, E, lookahead, wheelbase, max_reacquire, d_steer, d_speed, d_near_idx, d_la_idx, d_status);
}

int f1p_pure_pursuit_batch(f1p_ctx* ctx, const double* poses, int32_t E, double lookahead, double wheelbase,
                           double max_reacquire, double* steer, double* speed, int32_t* near_idx, int32_t* la_idx,
                           int32_t* status) {
    return pure_pursuit_batch_impl(ctx, poses, nullptr, false, E, lookahead, wheelbase, max_reacquire, steer, speed, near_idx, la_idx, status);
}

int f1p_pure_pursuit_tracks_batch(f1p_ctx* ctx, const double* poses, const int32_t* track_id, int32_t E, double lookahead, double wheelbase,
                                  double max_reacquire, double* steer, double* speed, int32_t* near_idx, int32_t* la_idx, int32_t* status) {
    return pure_pursuit_batch_impl(ctx, poses, track_id, true, E, lookahead, wheelbase, max_reacquire, steer, speed, near_idx, la_idx, status);
}

int f1p_pure_pursuit_set_form(f1p_ctx* ctx, int32_t egos_per_wave) {
    if (!ctx) return F1P_EINVAL;
    if (egos_per_wave != 0 && egos_per_wave != 1 && egos_per_wave != 4 && egos_per_wave != 8 && egos_per_wave != 16)
        return set_error(ctx, F1P_EINVAL, "egos per wave must be 0 (by batch size), 1, 4, 8 or 16");
    ctx->pursuit_form = egos_per_wave;
    return F1P_OK;
}

// ---------------------------------------------------------------------------------------------------
int f1p_stanley_batch(f1p_ctx* ctx, const double* states, int32_t E, double wheelbase, double k_path, double* steer,
                      double* speed, int32_t* near_idx) {
    return stanley_impl(ctx, states, nullptr, false, E, wheelbase, k_path, steer, speed, near_idx);
}

int f1p_stanley_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, double wheelbase, double k_path,
                             double* steer, double* speed, int32_t* near_idx) {
    return stanley_impl(ctx, states, track_id, true, E, wheelbase, k_path, steer, speed, near_idx);
}

int f1p_lqr_batch(f1p_ctx* ctx, const double* states, double* err, int32_t E, double wheelbase, double timestep,
                  const double q[4], double r, int32_t max_iter, double eps, double* steer, double* speed,
                  int32_t* near_idx) {
    return lqr_impl(ctx, states, nullptr, false, err, E, wheelbase, timestep, q, r, max_iter, eps, steer, speed, near_idx);
}

int f1p_lqr_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, double* err, int32_t E, double wheelbase, double timestep,
                         const double q[4], double r, int32_t max_iter, double eps, double* steer, double* speed, int32_t* near_idx) {
    return lqr_impl(ctx, states, track_id, true, err, E, wheelbase, timestep, q, r, max_iter, eps, steer, speed, near_idx);
}
