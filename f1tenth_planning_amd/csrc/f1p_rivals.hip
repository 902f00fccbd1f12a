// f1p_rivals.hip -- the rivals entry points of include/f1p.h: the races' member lists on the context, the asynchronous device call and its
// host-array wrapper (kernel: k_rivals.hip), and the same pair with the rivals predicted along their courses (kernels: k_rivals_predict.hip)
#include <numeric>

#include "f1p_host.h"

using namespace f1p;

int f1p_rivals_set_groups(f1p_ctx* ctx, const int32_t* group, int32_t E) {
    F1P_ENTER(ctx);
    if (!group) { ctx->riv_E = 0; return F1P_OK; }                     // one race of all, whatever E (the buffers are kept)
    if (E < 1) return set_error(ctx, F1P_EINVAL, "rivals: E must be >= 1");
    // members sorted by (group, ego), the ungrouped (negative id) left out; each ego's [begin, end) in that list -- empty for an ungrouped one
    std::vector<int32_t> mem((size_t)E), rng((size_t)2 * E, 0);
    std::iota(mem.begin(), mem.end(), 0);
    mem.erase(std::remove_if(mem.begin(), mem.end(), [&](int32_t e) { return group[e] < 0; }), mem.end());
    std::stable_sort(mem.begin(), mem.end(), [&](int32_t a, int32_t b) { return group[a] < group[b]; });
    for (size_t b = 0; b < mem.size();) {
        size_t e = b;
        while (e < mem.size() && group[mem[e]] == group[mem[b]]) ++e;
        for (size_t k = b; k < e; ++k) { rng[2 * (size_t)mem[k]] = (int32_t)b; rng[2 * (size_t)mem[k] + 1] = (int32_t)e; }
        b = e;
    }
    mem.resize((size_t)E, 0);                                         // (the tail is never read: every end <= the number of members)
    ctx->riv_E = 0;
    if (E > ctx->riv_cap) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));              // no launch in flight reads the old lists
        if (ctx->d_riv_mem) (void)hipFree(ctx->d_riv_mem);
        if (ctx->d_riv_rng) (void)hipFree(ctx->d_riv_rng);
        ctx->d_riv_mem = ctx->d_riv_rng = nullptr; ctx->riv_cap = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_riv_mem, sizeof(int32_t) * (size_t)E));
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_riv_rng, sizeof(int32_t) * 2 * (size_t)E));
        ctx->riv_cap = E;
    }
    StreamDrain drain{ctx};
    int rc;
    if ((rc = drain.copy(ctx->d_riv_mem, mem.data(), sizeof(int32_t) * (size_t)E, hipMemcpyHostToDevice))) return rc;
    if ((rc = drain.copy(ctx->d_riv_rng, rng.data(), sizeof(int32_t) * 2 * (size_t)E, hipMemcpyHostToDevice))) return rc;
    if ((rc = drain.finish())) return rc;
    ctx->riv_E = E;
    return F1P_OK;
}

// the argument checks both entry points share; nothing is launched when one fails
static int rivals_check(f1p_ctx* ctx, const void* states, int layout, int E, int M, double radius, double reach, double min_speed, const void* obs) {
    if (layout != F1P_RIVALS_XYVYAW && layout != F1P_RIVALS_POSE && layout != F1P_RIVALS_ST7)
        return set_error(ctx, F1P_EINVAL, "rivals: layout must be F1P_RIVALS_XYVYAW, F1P_RIVALS_POSE or F1P_RIVALS_ST7");
    if (M < 1 || M > F1P_RIVALS_MAX) return set_error(ctx, F1P_EINVAL, "rivals: M must be in [1, 16]");
    if (!(radius >= 0.0)) return set_error(ctx, F1P_EINVAL, "rivals: radius must be >= 0");
    if (!(reach >= 0.0)) return set_error(ctx, F1P_EINVAL, "rivals: reach must be >= 0 (+inf: no limit)");
    if (!(min_speed > 0.0)) return set_error(ctx, F1P_EINVAL, "rivals: min_speed must be > 0");
    if (E < 1) return set_error(ctx, F1P_EINVAL, "rivals: E must be >= 1");
    if (!states || !obs) return set_error(ctx, F1P_EINVAL, "rivals: states or obs is NULL");
    if (ctx->riv_E > 0 && ctx->riv_E != E)
        return set_error(ctx, F1P_ESTATE, "rivals: the groups were set for " + std::to_string(ctx->riv_E) + " egos, this call has " + std::to_string(E) +
                                              " (f1p_rivals_set_groups)");
    return F1P_OK;
}

static int rivals_launch(f1p_ctx* ctx, const double* d_states, int layout, int E, int M, double radius, double reach, double min_speed, double* d_obs,
                         double* d_pace, int32_t* d_idx) {
    const bool grouped = ctx->riv_E > 0;
    return launch_rivals(ctx, d_states, layout, E, M, radius, reach * reach, min_speed, grouped ? ctx->d_riv_mem : nullptr,
                         grouped ? ctx->d_riv_rng : nullptr, d_obs, d_pace, d_idx);
}

int f1p_rivals_dev(f1p_ctx* ctx, const double* d_states, int32_t layout, int32_t E, int32_t M, double radius, double reach, double min_speed,
                   double* d_obs, double* d_pace, int32_t* d_idx) {
    F1P_ENTER(ctx);
    if (const int rc = rivals_check(ctx, d_states, layout, E, M, radius, reach, min_speed, d_obs)) return rc;
    return rivals_launch(ctx, d_states, layout, E, M, radius, reach, min_speed, d_obs, d_pace, d_idx);
}

int f1p_rivals_batch(f1p_ctx* ctx, const double* states, int32_t layout, int32_t E, int32_t M, double radius, double reach, double min_speed,
                     double* obs, double* pace, int32_t* idx) {
    F1P_ENTER(ctx);
    int rc;
    if ((rc = rivals_check(ctx, states, layout, E, M, radius, reach, min_speed, obs))) return rc;
    const size_t ncol = layout == F1P_RIVALS_ST7 ? 7 : 4;
    Stage s(ctx);
    s.need(sizeof(double) * ncol * E); s.need(sizeof(double) * 5 * (size_t)E * M); s.need(sizeof(double) * E, pace != nullptr);
    s.need(sizeof(int32_t) * (size_t)E * M, idx != nullptr);
    if ((rc = s.begin())) return rc;
    const double* d_s;
    if ((rc = s.in(states, ncol * E, &d_s))) return rc;
    double* d_obs = s.out(obs, (size_t)5 * E * M);
    double* d_pace = s.out(pace, (size_t)E);
    int32_t* d_idx = s.out(idx, (size_t)E * M);
    if ((rc = rivals_launch(ctx, d_s, layout, E, M, radius, reach, min_speed, d_obs, d_pace, d_idx))) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------------
// rivals predicted along their courses (kernels: k_rivals_predict.hip; the rule: include/f1p.h)
int f1p_rivals_set_course(f1p_ctx* ctx, const int32_t* track_id, int32_t E) {
    F1P_ENTER(ctx);
    if (!track_id) { ctx->riv_course_E = 0; return F1P_OK; }           // every vehicle on the raceline, whatever E (the buffer is kept)
    if (E < 1) return set_error(ctx, F1P_EINVAL, "rivals: E must be >= 1");
    ctx->riv_course_E = 0;
    if (E > ctx->riv_tid_cap) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));              // no launch in flight reads the old ids
        if (ctx->d_riv_tid) (void)hipFree(ctx->d_riv_tid);
        ctx->d_riv_tid = nullptr; ctx->riv_tid_cap = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_riv_tid, sizeof(int32_t) * (size_t)E));
        ctx->riv_tid_cap = E;
    }
    StreamDrain drain{ctx};                                           // (the caller's array is the source: drained before it returns)
    int rc;
    if ((rc = drain.copy(ctx->d_riv_tid, track_id, sizeof(int32_t) * (size_t)E, hipMemcpyHostToDevice))) return rc;
    if ((rc = drain.finish())) return rc;
    ctx->riv_course_E = E;
    return F1P_OK;
}

static int predict_check(f1p_ctx* ctx, const f1p_rivals_predict* pr, int E) {
    if (!pr) return set_error(ctx, F1P_EINVAL, "rivals: the prediction's parameters are NULL");
    if (pr->knots < 1 || pr->knots > F1P_RIVALS_KNOTS_MAX) return set_error(ctx, F1P_EINVAL, "rivals: knots must be in [1, 16]");
    if (!(pr->horizon_s >= 0.0) || !(pr->horizon_m >= 0.0)) return set_error(ctx, F1P_EINVAL, "rivals: horizon_s and horizon_m must be >= 0");
    if (pr->horizon_s == 0.0 && pr->horizon_m == 0.0) return set_error(ctx, F1P_EINVAL, "rivals: horizon_s and horizon_m are both zero");
    if (pr->speed != F1P_RIVALS_SPEED_CONSTANT && pr->speed != F1P_RIVALS_SPEED_PROFILE)
        return set_error(ctx, F1P_EINVAL, "rivals: speed must be F1P_RIVALS_SPEED_CONSTANT or F1P_RIVALS_SPEED_PROFILE");
    if (ctx->riv_course_E > 0) {
        if (ctx->riv_course_E != E)
            return set_error(ctx, F1P_ESTATE, "rivals: the courses were set for " + std::to_string(ctx->riv_course_E) + " vehicles, this call has " +
                                                  std::to_string(E) + " (f1p_rivals_set_course)");
        if (ctx->trk_K < 1) return set_error(ctx, F1P_ESTATE, "rivals: the vehicles follow tracks of a track set, and none is loaded (f1p_set_track_set)");
    } else if (ctx->n_wp < 2) {
        return set_error(ctx, F1P_ESTATE, "rivals: the vehicles follow the raceline, and none is loaded (f1p_set_waypoints)");
    }
    return F1P_OK;
}

// the arc table of the course in force, rebuilt (one launch) when the raceline / track set has changed since it was built
static int ensure_arc(f1p_ctx* ctx, bool tracks, f1p_ctx::ArcTab** out) {
    f1p_ctx::ArcTab& a = tracks ? ctx->arc_trk : ctx->arc_wp;
    const unsigned long long gen = tracks ? ctx->trk_gen : ctx->wp_gen;
    *out = &a;
    if (a.gen == gen) return F1P_OK;
    const size_t rows = tracks ? (size_t)ctx->trk_rows : (size_t)ctx->n_wp;
    const int K = tracks ? ctx->trk_K : 1;
    if (rows > a.rows || K > a.K) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (a.cum) (void)hipFree(a.cum);
        if (a.ok) (void)hipFree(a.ok);
        a.cum = nullptr; a.ok = nullptr; a.rows = 0; a.K = 0; a.gen = 0;
        F1P_HIP(ctx, hipMalloc((void**)&a.cum, sizeof(double) * rows));
        F1P_HIP(ctx, hipMalloc((void**)&a.ok, sizeof(int32_t) * (size_t)K));
        a.rows = rows; a.K = K;
    }
    a.gen = 0;
    if (const int rc = launch_course_arc(ctx, tracks, a.cum, a.ok)) return rc;
    a.gen = gen;
    return F1P_OK;
}

// the time table next to it (speed = profile only; after ensure_arc: k_course_time reads the arc table's flags), rebuilt (one launch) when the course
// has changed since it was built or the call's min_speed, the floor of the segment speeds, is another one
static int ensure_time(f1p_ctx* ctx, bool tracks, double min_speed, f1p_ctx::ArcTab& a) {
    if (a.tgen == a.gen && a.min_speed == min_speed) return F1P_OK;
    if (a.rows > a.trows || a.K > a.tK) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (a.tim) (void)hipFree(a.tim);
        if (a.pok) (void)hipFree(a.pok);
        a.tim = nullptr; a.pok = nullptr; a.trows = 0; a.tK = 0; a.tgen = 0;
        F1P_HIP(ctx, hipMalloc((void**)&a.tim, sizeof(double) * a.rows));
        F1P_HIP(ctx, hipMalloc((void**)&a.pok, sizeof(int32_t) * (size_t)a.K));
        a.trows = a.rows; a.tK = a.K;
    }
    a.tgen = 0;
    if (const int rc = launch_course_time(ctx, tracks, min_speed, a.ok, a.tim, a.pok)) return rc;
    a.tgen = a.gen; a.min_speed = min_speed;
    return F1P_OK;
}

static int predict_launch(f1p_ctx* ctx, const double* d_states, int layout, int E, int M, double radius, double reach, double min_speed,
                          const f1p_rivals_predict* pr, double* d_obs, double* d_pace, int32_t* d_idx, double* d_frenet) {
    if (E > ctx->riv_scr_cap) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_riv_rec) (void)hipFree(ctx->d_riv_rec);
        if (ctx->d_riv_idx) (void)hipFree(ctx->d_riv_idx);
        ctx->d_riv_rec = nullptr; ctx->d_riv_idx = nullptr; ctx->riv_scr_cap = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_riv_rec, sizeof(double) * 4 * (size_t)E));
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_riv_idx, sizeof(int32_t) * F1P_RIVALS_MAX * (size_t)E));
        ctx->riv_scr_cap = E;
    }
    const bool tracks = ctx->riv_course_E > 0;
    f1p_ctx::ArcTab* arc;
    int rc;
    if ((rc = ensure_arc(ctx, tracks, &arc))) return rc;
    if (pr->speed == F1P_RIVALS_SPEED_PROFILE && (rc = ensure_time(ctx, tracks, min_speed, *arc))) return rc;
    int32_t* idx = d_idx ? d_idx : ctx->d_riv_idx;
    if ((rc = rivals_launch(ctx, d_states, layout, E, M, radius, reach, min_speed, d_obs, d_pace, idx))) return rc;
    return launch_rivals_predict(ctx, d_states, layout, E, M, radius, min_speed, pr, tracks ? ctx->d_riv_tid : nullptr, arc->cum, arc->ok, arc->tim,
                                 arc->pok, ctx->d_riv_rec, idx, d_obs, d_frenet);
}

int f1p_rivals_predict_dev(f1p_ctx* ctx, const double* d_states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                           double min_speed, const f1p_rivals_predict* pr, double* d_obs, double* d_pace, int32_t* d_idx, double* d_frenet) {
    F1P_ENTER(ctx);
    int rc;
    if ((rc = rivals_check(ctx, d_states, layout, E, M, radius, reach, min_speed, d_obs))) return rc;
    if ((rc = predict_check(ctx, pr, E))) return rc;
    return predict_launch(ctx, d_states, layout, E, M, radius, reach, min_speed, pr, d_obs, d_pace, d_idx, d_frenet);
}

int f1p_rivals_predict_batch(f1p_ctx* ctx, const double* states, int32_t layout, int32_t E, int32_t M, double radius, double reach,
                             double min_speed, const f1p_rivals_predict* pr, double* obs, double* pace, int32_t* idx, double* frenet) {
    F1P_ENTER(ctx);
    int rc;
    if ((rc = rivals_check(ctx, states, layout, E, M, radius, reach, min_speed, obs))) return rc;
    if ((rc = predict_check(ctx, pr, E))) return rc;
    const size_t ncol = layout == F1P_RIVALS_ST7 ? 7 : 4;
    Stage s(ctx);
    s.need(sizeof(double) * ncol * E); s.need(sizeof(double) * 5 * (size_t)E * M); s.need(sizeof(double) * E, pace != nullptr);
    s.need(sizeof(int32_t) * (size_t)E * M, idx != nullptr); s.need(sizeof(double) * 3 * (size_t)E, frenet != nullptr);
    if ((rc = s.begin())) return rc;
    const double* d_s;
    if ((rc = s.in(states, ncol * E, &d_s))) return rc;
    double* d_obs = s.out(obs, (size_t)5 * E * M);
    double* d_pace = s.out(pace, (size_t)E);
    int32_t* d_idx = s.out(idx, (size_t)E * M);
    double* d_frenet = s.out(frenet, (size_t)3 * E);
    if ((rc = predict_launch(ctx, d_s, layout, E, M, radius, reach, min_speed, pr, d_obs, d_pace, d_idx, d_frenet))) return rc;
    return s.finish();
}
