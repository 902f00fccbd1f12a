// f1p_lattice.hip -- the lattice planner's entry points: plan (device and host pointers, fp64 and f32 rows, raceline and track set), the
// closed-loop mode and the one-call control step, the schedule's modes and debug hooks, the clothoid helpers
#include "f1p_host.h"

using namespace f1p;

#ifndef F1P_TRAJ_ZEROCOPY
#define F1P_TRAJ_ZEROCOPY 1
#endif
#ifndef F1P_IO_ZEROCOPY
#define F1P_IO_ZEROCOPY 1       // f1p_lattice_plan_batch: page-locked poses / result columns are read / written by the kernels themselves (0: copies, A/B)
#endif
#define F1P_PLAN_CHUNK_MIN_EGOS 2048
#ifndef F1P_ZEROCOPY_MIN_EGOS
#define F1P_ZEROCOPY_MIN_EGOS 32       // batches from this size hand page-locked caller arrays to the kernels (measured p50 plan(), fp64 rows, copies -> in place: 64 egos 0.075 -> 0.061 ms, 256: 0.090 -> 0.068, 1024: 0.126 -> 0.103, 4096: 0.236 -> 0.218; below 32 the small-call bounce block is as fast)
#endif
#define F1P_PLAN_CHUNKS_MAX 8          // = number of slice events in f1p_ctx

static int ensure_copy_stream(f1p_ctx* ctx) {
    if (ctx->copy_stream) return F1P_OK;
    F1P_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (auto& ev : ctx->ev_chunk) F1P_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return F1P_OK;
}

// tracks: a track plan (f1p_lattice_*_tracks_*) reads the track set instead of the raceline
static int validate_lattice(f1p_ctx* ctx, const f1p_lattice_cfg* cfg, int E, bool device_goals, bool need_outputs_ok, bool tracks = false) {
    if (!cfg) return set_error(ctx, F1P_EINVAL, "cfg is NULL");
    if (E < 0) return set_error(ctx, F1P_EINVAL, "E must be >= 0");
    if (!need_outputs_ok) return set_error(ctx, F1P_EINVAL, "steer, speed and best_idx outputs are required");
    if (cfg->n_stations < 2 || cfg->n_stations > 1024) return set_error(ctx, F1P_EINVAL, "n_stations must be in [2, 1024]");
    if (cfg->n_lookahead < 1 || cfg->n_lookahead > F1P_MAX_LOOKAHEADS || cfg->n_width < 1 || cfg->n_width > F1P_MAX_WIDTHS)
        return set_error(ctx, F1P_EINVAL, "n_lookahead / n_width out of range [1, 64]");
    if (cfg->n_shift < 0 || cfg->n_cull < 0) return set_error(ctx, F1P_EINVAL, "n_shift and n_cull must be >= 0");
    const int C = cfg->n_lookahead * cfg->n_width;
    if (cfg->cand_begin < 0 || cfg->cand_count < 0 || cfg->cand_begin + cfg->cand_count > C || (cfg->cand_count == 0 && cfg->cand_begin != 0))
        return set_error(ctx, F1P_EINVAL, "candidate shard [cand_begin, cand_begin+cand_count) outside [0, C)");
    if (cfg->generator != F1P_GEN_CLOTHOID && cfg->generator != F1P_GEN_CUBIC) return set_error(ctx, F1P_EINVAL, "unknown trajectory generator");
    if (tracks) {
        if (ctx->trk_K < 1) return set_error(ctx, F1P_ESTATE, "no track set: call f1p_set_track_set first");
        if (device_goals && !ctx->trk_has_psi) return set_error(ctx, F1P_ESTATE, "device goal sampling needs a heading column in the track set (col_psi >= 0)");
        if (cfg->cand_count > 0) return set_error(ctx, F1P_EINVAL, "track plans take whole egos: cfg.cand_count must be 0");
        return F1P_OK;
    }
    if (ctx->n_wp < 2) return set_error(ctx, F1P_ESTATE, "waypoints not set: call f1p_set_waypoints first");
    if (device_goals && !ctx->has_psi) return set_error(ctx, F1P_ESTATE, "device goal sampling needs a heading column (col_psi >= 0)");
    return F1P_OK;
}

// f1p_lattice_set_obstacles' preconditions, checked by every entry point that plans: the batch size the discs were set for, whole egos
static int lattice_obs_check(f1p_ctx* ctx, const f1p_lattice_cfg* cfg, int E) {
    if (!ctx->lat_obs.cur) return F1P_OK;
    if (E != ctx->lat_obs.E)
        return set_error(ctx, F1P_ESTATE, "lattice obstacles were set for " + std::to_string(ctx->lat_obs.E) + " egos, this plan has " + std::to_string(E) + ": set them again or clear them (f1p_lattice_set_obstacles)");
    if (cfg->cand_count > 0) return set_error(ctx, F1P_ESTATE, "lattice obstacles are set and cover whole egos: a candidate shard (cfg.cand_count > 0) is not tested, clear them first");
    return F1P_OK;
}

// a slice of a batch (or the audit's window) plans with the per-ego obstacle arrays offset to its first ego; back to 0 on every way out
struct LatObsSlice {
    f1p_ctx* c;
    explicit LatObsSlice(f1p_ctx* ctx, size_t e0) : c(ctx) { c->lat_obs_e0 = (int)e0; }
    ~LatObsSlice() { c->lat_obs_e0 = 0; }
};

int f1p_lattice_set_obstacles(f1p_ctx* ctx, const double* obs, const double* pace, int32_t E, int32_t M) {
    F1P_ENTER(ctx);
    if (!obs || M == 0) { ctx->lat_pace_cur = nullptr; return set_obstacles(ctx, ctx->lat_obs, "lattice", false, nullptr, 0, 0, false); }
    if (!pace) return set_error(ctx, F1P_EINVAL, "lattice obstacles: pace is NULL");
    if (ctx->lattice_split > 0) return set_error(ctx, F1P_ESTATE, "lattice obstacle test runs one workgroup per ego: f1p_lattice_set_split(0)");
    int rc = set_obstacles(ctx, ctx->lat_obs, "lattice", false, obs, E, M, false);
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)E;
    auto fail = [&]() { ctx->lat_obs.cur = nullptr; ctx->lat_obs.E = 0; ctx->lat_obs.M = 0; ctx->lat_pace_cur = nullptr; };
    if (bytes > ctx->lat_pace_bytes) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { fail(); return check_hip(ctx, hipGetLastError(), "hipStreamSynchronize"); }
        if (ctx->d_lat_pace) (void)hipFree(ctx->d_lat_pace);
        ctx->d_lat_pace = nullptr; ctx->lat_pace_bytes = 0;
        const hipError_t er = hipMalloc((void**)&ctx->d_lat_pace, bytes);
        if (er != hipSuccess) { fail(); return check_hip(ctx, er, "hipMalloc (lattice paces)"); }
        ctx->lat_pace_bytes = bytes;
    }
    hipError_t er = hipMemcpyAsync(ctx->d_lat_pace, pace, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(ctx->stream);
    if (er != hipSuccess) { fail(); return check_hip(ctx, er, "copy of the lattice paces"); }
    ctx->lat_pace_cur = ctx->d_lat_pace;
    return F1P_OK;
}

int f1p_lattice_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, const double* d_pace, int32_t E, int32_t M) {
    F1P_ENTER(ctx);
    if (!d_obs || M == 0) { ctx->lat_pace_cur = nullptr; return set_obstacles(ctx, ctx->lat_obs, "lattice", false, nullptr, 0, 0, true); }
    if (!d_pace) return set_error(ctx, F1P_EINVAL, "lattice obstacles: pace is NULL");
    if (ctx->lattice_split > 0) return set_error(ctx, F1P_ESTATE, "lattice obstacle test runs one workgroup per ego: f1p_lattice_set_split(0)");
    const int rc = set_obstacles(ctx, ctx->lat_obs, "lattice", false, d_obs, E, M, true);
    if (rc) return rc;
    ctx->lat_pace_cur = d_pace;
    return F1P_OK;
}

void f1p_lattice_cfg_default(f1p_lattice_cfg* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->n_stations = 100;                                   // lattice_planner.py:197
    cfg->n_lookahead = 4;                                    // :228
    cfg->n_width = 7;                                        // :229
    const double la[4] = {0.4, 0.6, 0.8, 1.0};
    for (int i = 0; i < 4; ++i) cfg->lookahead[i] = la[i];
    for (int i = 0; i < 7; ++i) cfg->width[i] = -1.0 + (2.0 / 6.0) * i;   // np.linspace(-1, 1, 7)
    cfg->width[6] = 1.0;
    cfg->n_shift = 1; cfg->n_cull = 1;
    cfg->check_collision = 1;
    cfg->w_length = 1.0;                                     // the only example cost that runs (:268-271)
    cfg->track_lookahead = 0.8;                              // :211
    cfg->wheelbase = 0.33;                                   // :55 (tracker default)
    cfg->max_reacquire = 20.0;                               // pure_pursuit.py:52
}

// ---------------------------------------------------------------------------------------------------
// Closed-loop mode (f1p_lattice_set_closed_loop): every plan leaves its winners' heading column on the device, [E][S] fp64 in one of two
// ctx-owned buffers used alternately, and the next plan of the same shape that passes prev_theta == NULL takes it as its previous path
// (get_similarity_cost, lattice_planner.py:287-296: the reference compares with the previous plan's best trajectory).  Nothing crosses PCIe.
struct ClosedLoop {
    const double* prev = nullptr;      // the plan's prev_theta (the caller's, or the kept headings, or null = first plan)
    double* out = nullptr;             // where its winners' headings go (null: closed loop off)
    bool from_ctx = false;
};

static int cl_begin(f1p_ctx* ctx, const double* d_prev_caller, int E, int S, bool writes, ClosedLoop* cl) {
    cl->prev = d_prev_caller; cl->out = nullptr; cl->from_ctx = false;
    if (!ctx->lattice_closed_loop || E <= 0) return F1P_OK;
    const size_t need = sizeof(double) * (size_t)E * S;
    if (need > ctx->cl_bytes) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (auto& b : ctx->d_cl_theta) { if (b) (void)hipFree(b); b = nullptr; }
        ctx->cl_bytes = 0; ctx->cl_valid = false;
        for (auto& b : ctx->d_cl_theta) {
            if (hipMalloc((void**)&b, need) != hipSuccess) {         // both buffers or none (a failed second allocation left the first behind with cl_bytes = 0)
                (void)hipGetLastError();
                for (auto& q : ctx->d_cl_theta) { if (q) (void)hipFree(q); q = nullptr; }
                return set_error(ctx, F1P_ENOMEM, "closed-loop heading buffers: out of device memory");
            }
        }
        ctx->cl_bytes = need;
    }
    if (ctx->cl_valid && (ctx->cl_E != E || ctx->cl_S != S)) ctx->cl_valid = false;   // another batch shape: a first plan again
    if (!d_prev_caller && ctx->cl_valid) { cl->prev = ctx->d_cl_theta[ctx->cl_cur]; cl->from_ctx = true; }
    if (writes) cl->out = ctx->d_cl_theta[ctx->cl_valid ? ctx->cl_cur ^ 1 : 0];
    return F1P_OK;
}

static void cl_commit(f1p_ctx* ctx, const ClosedLoop& cl, int E, int S) {
    if (!cl.out) return;
    ctx->cl_cur = cl.out == ctx->d_cl_theta[0] ? 0 : 1;
    ctx->cl_valid = true; ctx->cl_E = E; ctx->cl_S = S;
}

static int lattice_plan_dev_impl(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                                 int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                                 int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                                 double* d_best_traj, double* d_all_cost, double* d_all_traj, float* d_best_traj32, double* d_theta_out = nullptr,
                                 double* d_pose_copy = nullptr, const int32_t* d_track_id = nullptr, bool tracks = false) {
    int rc = validate_lattice(ctx, cfg, E, d_goals == nullptr, E == 0 || (d_poses && d_best_idx && (cfg && cfg->cand_count > 0 ? true : (d_steer && d_speed))), tracks);
    if (rc) return rc;
    if (tracks && E > 0 && !d_track_id) return set_error(ctx, F1P_EINVAL, "track_id is NULL");
    // a candidate shard evaluates only (cost + index); the emit half runs after the cross-rank argmin
    const int mode = cfg->cand_count > 0 ? LATTICE_EVAL : LATTICE_FULL;
    return launch_lattice(ctx, mode, d_poses, d_goals, d_prev_theta, E, cfg, nullptr, nullptr, d_steer, d_speed, d_best_idx,
                          d_best_cost, d_status, d_near_idx, d_best_traj, d_all_cost, d_all_traj, d_best_traj32, d_theta_out, d_pose_copy, d_track_id);
}

// the *_dev entry points in closed-loop mode: prev_theta == NULL means "the headings the previous plan left on the device"
static int lattice_plan_dev_cl(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                               int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                               int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                               double* d_best_traj, double* d_all_cost, double* d_all_traj, float* d_best_traj32,
                               const int32_t* d_track_id = nullptr, bool tracks = false) {
    ClosedLoop cl;
    // the configuration is validated BEFORE cl_begin touches the kept headings (an invalid cfg -- a huge n_stations -- used to free
    // them and fail in hipMalloc instead of returning F1P_EINVAL); lattice_plan_dev_impl validates again, with the output pointers
    if (const int rcv = validate_lattice(ctx, cfg, E, d_goals == nullptr, true, tracks)) return rcv;
    if (tracks && E > 0 && !d_track_id) return set_error(ctx, F1P_EINVAL, "track_id is NULL");
    if (const int rco = lattice_obs_check(ctx, cfg, E)) return rco;
    if (cfg && E > 0 && cfg->n_stations >= 2) {
        const int rc0 = cl_begin(ctx, d_prev_theta, E, cfg->n_stations, cfg->cand_count == 0, &cl);
        if (rc0) return rc0;
    } else cl.prev = d_prev_theta;
    const int rc = lattice_plan_dev_impl(ctx, d_poses, d_goals, cl.prev, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx,
                                         d_best_traj, d_all_cost, d_all_traj, d_best_traj32, cl.out, nullptr, d_track_id, tracks);
    if (rc == F1P_OK) cl_commit(ctx, cl, E, cfg->n_stations);
    return rc;
}

int f1p_lattice_plan_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                         int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                         int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                         double* d_best_traj, double* d_all_cost, double* d_all_traj) {
    F1P_ENTER(ctx);
    return lattice_plan_dev_cl(ctx, d_poses, d_goals, d_prev_theta, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx,
                               d_best_traj, d_all_cost, d_all_traj, nullptr);
}

int f1p_lattice_plan_dev_f32(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta,
                             int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                             int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx, float* d_best_traj32) {
    F1P_ENTER(ctx);
    return lattice_plan_dev_cl(ctx, d_poses, d_goals, d_prev_theta, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx,
                               nullptr, nullptr, nullptr, d_best_traj32);
}

int f1p_lattice_plan_tracks_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, const double* d_prev_theta, const int32_t* d_track_id,
                                int32_t E, const f1p_lattice_cfg* cfg, double* d_steer, double* d_speed,
                                int32_t* d_best_idx, double* d_best_cost, int32_t* d_status, int32_t* d_near_idx,
                                double* d_best_traj, double* d_all_cost, double* d_all_traj) {
    F1P_ENTER(ctx);
    return lattice_plan_dev_cl(ctx, d_poses, d_goals, d_prev_theta, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_status, d_near_idx,
                               d_best_traj, d_all_cost, d_all_traj, nullptr, d_track_id, true);
}

int f1p_lattice_emit_dev(f1p_ctx* ctx, const double* d_poses, const double* d_goals, int32_t E,
                         const f1p_lattice_cfg* cfg, const int32_t* d_cand_idx, const double* d_cand_cost,
                         double* d_steer, double* d_speed, int32_t* d_status, int32_t* d_near_idx, double* d_best_traj) {
    F1P_ENTER(ctx);
    int rc = validate_lattice(ctx, cfg, E, d_goals == nullptr, E == 0 || (d_poses && d_cand_idx && d_steer && d_speed));
    if (rc) return rc;
    if (ctx->lat_obs.cur) return set_error(ctx, F1P_ESTATE, "lattice obstacles are set: the emit half of a sharded plan is not tested against them, clear them first (f1p_lattice_set_obstacles)");
    ClosedLoop cl;                                                 // the emitted winners are this plan's previous path for the next one
    if (E > 0 && (rc = cl_begin(ctx, nullptr, E, cfg->n_stations, true, &cl))) return rc;
    rc = launch_lattice(ctx, LATTICE_EMIT, d_poses, d_goals, nullptr, E, cfg, d_cand_idx, d_cand_cost, d_steer, d_speed,
                        nullptr, nullptr, d_status, d_near_idx, d_best_traj, nullptr, nullptr, nullptr, cl.out);
    if (rc == F1P_OK) cl_commit(ctx, cl, E, cfg->n_stations);
    return rc;
}

int f1p_lattice_set_closed_loop(f1p_ctx* ctx, int32_t on) {
    if (!ctx) return F1P_EINVAL;
    ctx->lattice_closed_loop = on != 0;
    ctx->cl_valid = false;                                         // (re)armed: the next plan is a first plan
    ctx->step_chain = false;
    return F1P_OK;
}

int f1p_lattice_closed_loop_state(f1p_ctx* ctx, const double** d_prev_theta, int32_t* E, int32_t* S) {
    if (!ctx) return F1P_EINVAL;
    const bool v = (ctx->lattice_closed_loop || ctx->step_chain) && ctx->cl_valid;   // (the headings the next plan -- or, for a step chain, the next STEP -- would use)
    if (d_prev_theta) *d_prev_theta = v ? ctx->d_cl_theta[ctx->cl_cur] : nullptr;
    if (E) *E = v ? ctx->cl_E : 0;
    if (S) *S = v ? ctx->cl_S : 0;
    return F1P_OK;
}

// TRAJ = double (the reference's fp64 rows) or float (f1p_lattice_plan_batch_f32: the same rows rounded once on the device)
// tracks: a track plan, ego e on track track_id[e] (host array; every slice passes its own part of it)
template <typename TRAJ>
static int lattice_plan_batch_impl(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                                   int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                                   double* best_cost, int32_t* status, int32_t* near_idx, TRAJ* best_traj,
                                   double* all_cost, double* all_traj, const int32_t* track_id = nullptr, bool tracks = false) {
    constexpr bool F32 = sizeof(TRAJ) == 4;
    int rc = validate_lattice(ctx, cfg, E, goals == nullptr, E == 0 || (poses && best_idx && ((cfg && cfg->cand_count > 0) || (steer && speed))), tracks);
    if (rc) return rc;
    if (tracks && E > 0 && !track_id) return set_error(ctx, F1P_EINVAL, "track_id is NULL");
    if ((rc = lattice_obs_check(ctx, cfg, E))) return rc;
    if (cfg->cand_count > 0 && (steer || speed || status || best_traj))
        return set_error(ctx, F1P_EINVAL, "a candidate shard (cfg.cand_count > 0) only evaluates: it produces best_idx, best_cost and near_idx; "
                                          "pass NULL for steer / speed / status / best_traj and emit the global winner with f1p_lattice_emit_dev");
    const size_t C = (size_t)cfg->n_lookahead * cfg->n_width, S = cfg->n_stations, e = E;
    // (page-locked best_traj: see below -- decided here so that the arena does not reserve bytes nobody uses)
    TRAJ* bt_dev = (best_traj && !all_cost && !all_traj && E >= F1P_ZEROCOPY_MIN_EGOS)
                       ? (TRAJ*)pinned_device_ptr(ctx, best_traj, sizeof(TRAJ) * e * S * 4) : nullptr;
    const bool pinned = bt_dev != nullptr;
    const bool zero_copy_traj = F1P_TRAJ_ZEROCOPY && pinned && E < 8192;
    // Round 6: with the trajectories going straight into the caller's page-locked array, the poses and the per-ego result columns do too when
    // THEY are page-locked -- k_lattice_prologue reads the poses out of host memory and leaves a device copy (f1p_lattice_step_batch's scheme), the selection
    // kernel stores steer / speed / index / cost / status / nearest segment where the caller reads them: no hipMemcpy in either direction, each of which is
    // ~10 us of submission and DMA start-up in front of / behind a 65 us plan.  (All-fp64 mode keeps the copies: k_lattice re-reads the pose per thread.)
    const double* zp = nullptr; double *zs = nullptr, *zv = nullptr, *zc_ = nullptr; int32_t *zi = nullptr, *zt = nullptr, *zn = nullptr;
    bool zc_io = F1P_IO_ZEROCOPY && (best_traj ? zero_copy_traj : (E >= F1P_ZEROCOPY_MIN_EGOS && E < 8192 && !all_cost && !all_traj)) && !goals && !prev_theta &&
                 ctx->lattice_mixed != 0 && cfg->cand_count == 0;
    if (zc_io) {
        zp = (const double*)pinned_device_ptr(ctx, poses, 32 * e);
        zs = (double*)pinned_device_ptr(ctx, steer, 8 * e); zv = (double*)pinned_device_ptr(ctx, speed, 8 * e);
        zi = (int32_t*)pinned_device_ptr(ctx, best_idx, 4 * e);
        zc_ = best_cost ? (double*)pinned_device_ptr(ctx, best_cost, 8 * e) : nullptr;
        zt = status ? (int32_t*)pinned_device_ptr(ctx, status, 4 * e) : nullptr;
        zn = near_idx ? (int32_t*)pinned_device_ptr(ctx, near_idx, 4 * e) : nullptr;
        zc_io = zp && zs && zv && zi && (!best_cost || zc_) && (!status || zt) && (!near_idx || zn);
    }
    // track ids: read in place when page-locked, else staged like the poses
    const int32_t* ztid = (zc_io && tracks) ? (const int32_t*)pinned_device_ptr(ctx, track_id, 4 * e) : nullptr;
    Stage s(ctx);
    if (zc_io) {
        s.need(8 * 4 * e);                                      // the device copy of the poses
        s.need(4 * e, tracks && !ztid);
        if ((rc = s.begin())) return rc;
        double* d_pose_copy = (double*)arena_take(ctx, 8 * 4 * e);
        if (tracks && !ztid && (rc = s.in(track_id, e, &ztid))) return rc;
        ClosedLoop cl;
        if ((rc = cl_begin(ctx, nullptr, E, (int)S, true, &cl))) return rc;
        struct HostDst { f1p_ctx* c; ~HostDst() { c->traj_dst_host = false; } } host_dst{ctx};
        ctx->traj_dst_host = best_traj != nullptr;
        double* bt64 = nullptr; float* bt32 = nullptr;
        if (best_traj) { if (F32) bt32 = reinterpret_cast<float*>(bt_dev); else bt64 = reinterpret_cast<double*>(bt_dev); }
        if ((rc = lattice_plan_dev_impl(ctx, zp, nullptr, cl.prev, E, cfg, zs, zv, zi, zc_, zt, zn, bt64, nullptr, nullptr, bt32, cl.out, d_pose_copy, ztid, tracks)))
            return rc;
        cl_commit(ctx, cl, E, (int)S);
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return F1P_OK;
    }
    s.need(8 * 4 * e); s.need(8 * e * C * 3, goals); s.need(8 * e * S, prev_theta); s.need(4 * e, tracks);
    s.need(8 * e, steer); s.need(8 * e, speed); s.need(4 * e); s.need(8 * e, best_cost); s.need(4 * e, status); s.need(4 * e, near_idx);
    s.need(sizeof(TRAJ) * e * S * 4, best_traj && !zero_copy_traj); s.need(8 * e * C, all_cost); s.need(8 * e * C * S * 4, all_traj);
    if ((rc = s.begin())) return rc;
    const double *d_poses, *d_goals, *d_prev;
    if ((rc = s.in(poses, 4 * e, &d_poses))) return rc;
    if ((rc = s.in(goals, e * C * 3, &d_goals))) return rc;
    if ((rc = s.in(prev_theta, e * S, &d_prev))) return rc;
    const int32_t* d_tid = nullptr;
    if (tracks && (rc = s.in(track_id, e, &d_tid))) return rc;
    ClosedLoop cl;                                             // closed-loop mode: prev_theta == NULL = the headings the previous plan left on the device
    if (E > 0 && (rc = cl_begin(ctx, d_prev, E, (int)S, cfg->cand_count == 0, &cl))) return rc;
    d_prev = cl.prev;
    double* d_steer = s.out(steer, e); double* d_speed = s.out(speed, e); int32_t* d_bi = s.out(best_idx, e);
    double* d_bc = s.out(best_cost, e); int32_t* d_st = s.out(status, e); int32_t* d_ni = s.out(near_idx, e);
    // Trajectories into PAGE-LOCKED host memory (f1p_host_alloc / hipHostRegister), F1P_ZEROCOPY_MIN_EGOS <= E < 8192: the selection kernel writes
    // them straight into the caller's array (it is device-visible), so the PCIe writes stream while the kernel still runs and no
    // copy is submitted at all -- measured at 4096 egos, p50 host to host: fp64 rows 0.277 ms (0.287 with one hipMemcpyAsync behind
    // the plan, 0.294 with the plan in two slices and the copies on a second stream, the round-2 scheme), f32 rows 0.214 (0.230 /
    // 0.233); slicing only the selection kernel was worse still (0.30 / 0.24: every cross-stream edge costs ~10 us).
    // From 8192 egos the batch is planned in slices of >= 4096 egos whose results travel on a second stream while the next slice
    // is planned (only into page-locked memory: copies into pageable memory block the calling thread and would serialise the slices).
    TRAJ* d_bt = zero_copy_traj ? bt_dev : s.out(best_traj, e * S * 4);
    struct HostDst { f1p_ctx* c; ~HostDst() { c->traj_dst_host = false; } } host_dst{ctx};   // (reset on every way out)
    ctx->traj_dst_host = zero_copy_traj;
    double* d_ac = s.out(all_cost, e * C); double* d_at = s.out(all_traj, e * C * S * 4);
    auto plan = [&](size_t e0, size_t n) {
        LatObsSlice obs_slice(ctx, e0);                             // (the moving discs' per-ego arrays: from this slice's first ego)
        double* bt64 = nullptr; float* bt32 = nullptr;
        if (d_bt) { if (F32) bt32 = reinterpret_cast<float*>(d_bt) + e0 * S * 4; else bt64 = reinterpret_cast<double*>(d_bt) + e0 * S * 4; }
        return lattice_plan_dev_impl(ctx, d_poses + 4 * e0, d_goals ? d_goals + e0 * C * 3 : nullptr, d_prev ? d_prev + e0 * S : nullptr,
                                     (int32_t)n, cfg, d_steer ? d_steer + e0 : nullptr, d_speed ? d_speed + e0 : nullptr, d_bi + e0, d_bc ? d_bc + e0 : nullptr,
                                     d_st ? d_st + e0 : nullptr, d_ni ? d_ni + e0 : nullptr, bt64, e0 == 0 && n == e ? d_ac : nullptr,
                                     e0 == 0 && n == e ? d_at : nullptr, bt32, cl.out ? cl.out + e0 * S : nullptr, nullptr, d_tid ? d_tid + e0 : nullptr, tracks);
    };
    const int K = (pinned && E >= 8192) ? (E / 4096 < F1P_PLAN_CHUNKS_MAX ? E / 4096 : F1P_PLAN_CHUNKS_MAX) : 1;
    if (K > 1 && (rc = ensure_copy_stream(ctx))) return rc;
    if (K == 1) {
        if ((rc = plan(0, e))) return rc;
        cl_commit(ctx, cl, E, (int)S);
        return s.finish();
    }
    for (int k = 0; k < K; ++k) {
        const size_t e0 = e * k / K, e1 = e * (k + 1) / K, n = e1 - e0;
        if ((rc = plan(e0, n))) return rc;
        F1P_HIP(ctx, hipEventRecord(ctx->ev_chunk[k], ctx->stream));
        F1P_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_chunk[k], 0));
        F1P_HIP(ctx, hipMemcpyAsync(best_traj + e0 * S * 4, d_bt + e0 * S * 4, n * S * 4 * sizeof(TRAJ), hipMemcpyDeviceToHost, ctx->copy_stream));
    }
    cl_commit(ctx, cl, E, (int)S);
    rc = s.gather(best_traj);                                  // the per-ego scalars of every slice: one copy + scatter, on the planning stream
    F1P_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    return rc;
}

int f1p_lattice_plan_batch(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                           int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                           double* best_cost, int32_t* status, int32_t* near_idx, double* best_traj,
                           double* all_cost, double* all_traj) {
    F1P_ENTER(ctx);
    return lattice_plan_batch_impl<double>(ctx, poses, goals, prev_theta, E, cfg, steer, speed, best_idx, best_cost, status, near_idx, best_traj, all_cost, all_traj);
}

int f1p_lattice_plan_batch_f32(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta,
                               int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                               double* best_cost, int32_t* status, int32_t* near_idx, float* best_traj32) {
    F1P_ENTER(ctx);
    return lattice_plan_batch_impl<float>(ctx, poses, goals, prev_theta, E, cfg, steer, speed, best_idx, best_cost, status, near_idx, best_traj32, nullptr, nullptr);
}

int f1p_lattice_plan_tracks_batch(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta, const int32_t* track_id,
                                  int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                                  double* best_cost, int32_t* status, int32_t* near_idx, double* best_traj,
                                  double* all_cost, double* all_traj) {
    F1P_ENTER(ctx);
    return lattice_plan_batch_impl<double>(ctx, poses, goals, prev_theta, E, cfg, steer, speed, best_idx, best_cost, status, near_idx, best_traj, all_cost, all_traj,
                                           track_id, true);
}

int f1p_lattice_plan_tracks_batch_f32(f1p_ctx* ctx, const double* poses, const double* goals, const double* prev_theta, const int32_t* track_id,
                                      int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed, int32_t* best_idx,
                                      double* best_cost, int32_t* status, int32_t* near_idx, float* best_traj32) {
    F1P_ENTER(ctx);
    return lattice_plan_batch_impl<float>(ctx, poses, goals, prev_theta, E, cfg, steer, speed, best_idx, best_cost, status, near_idx, best_traj32, nullptr, nullptr,
                                          track_id, true);
}

// ---------------------------------------------------------------------------------------------------
// One closed-loop control step: poses in, (steer, speed, status) out, nothing else across PCIe.  No copy is submitted in either
// direction: k_lattice_prologue reads the poses straight out of page-locked host memory (one 32-byte read per ego-wave, hidden by
// the other waves) and leaves a device copy for the kernels behind it; the selection kernel stores the three result columns straight
// into page-locked host memory.  The caller's own arrays are used when they are page-locked (f1p_host_alloc / hipHostRegister), the
// context's block otherwise (one memcpy each way on the host).  Previous headings (similarity term) and -- on request -- the winners'
// rows stay in HBM.
static int ensure_step(f1p_ctx* ctx, int E, int S, bool keep_traj) {
    const size_t hb = al256(32 * (size_t)E) + 2 * al256(8 * (size_t)E) + al256(4 * (size_t)E);
    if (hb > ctx->step_host_bytes) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->h_step) (void)hipHostFree(ctx->h_step);
        ctx->h_step = nullptr; ctx->step_host_bytes = 0; ctx->h_step_dev = nullptr;
        F1P_HIP(ctx, hipHostMalloc((void**)&ctx->h_step, hb, hipHostMallocDefault));
        ctx->step_host_bytes = hb;
        void* dev = nullptr;
        ctx->h_step_dev = (hipHostGetDevicePointer(&dev, ctx->h_step, 0) == hipSuccess) ? (char*)dev : nullptr;
        if (!ctx->h_step_dev) (void)hipGetLastError();
    }
    const size_t db = al256(32 * (size_t)E) + 2 * al256(4 * (size_t)E) + (keep_traj ? al256(32 * (size_t)E * S) : 0);
    if (db > ctx->step_dev_bytes) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_step) (void)hipFree(ctx->d_step);
        ctx->d_step = nullptr; ctx->step_dev_bytes = 0; ctx->step_traj_E = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_step, db));
        ctx->step_dev_bytes = db;
    }
    return F1P_OK;
}

// tracks: f1p_lattice_step_tracks_batch, ego e on track track_id[e] (host array)
static int lattice_step_impl(f1p_ctx* ctx, const double* poses, int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                             int32_t* status, int32_t keep_traj, const int32_t* track_id, bool tracks) {
    int rc = validate_lattice(ctx, cfg, E, true, E == 0 || (poses && steer && speed), tracks);
    if (rc) return rc;
    if (cfg->cand_count > 0) return set_error(ctx, F1P_EINVAL, "f1p_lattice_step_batch plans whole egos: cfg.cand_count must be 0");
    if (tracks && E > 0 && !track_id) return set_error(ctx, F1P_EINVAL, "track_id is NULL");
    if ((rc = lattice_obs_check(ctx, cfg, E))) return rc;
    if (E == 0) return F1P_OK;
    const int S = cfg->n_stations;
    const size_t e = (size_t)E;
    if ((rc = ensure_step(ctx, E, S, keep_traj != 0))) return rc;
    char* hb = ctx->h_step;
    double* h_poses = (double*)hb; double* h_steer = (double*)(hb + al256(32 * e)); double* h_speed = (double*)((char*)h_steer + al256(8 * e));
    int32_t* h_status = (int32_t*)((char*)h_speed + al256(8 * e));
    char* db = ctx->d_step;
    double* d_pose_copy = (double*)db; int32_t* d_idx = (int32_t*)(db + al256(32 * e)); int32_t* d_near = (int32_t*)((char*)d_idx + al256(4 * e));
    double* d_traj = keep_traj ? (double*)((char*)d_near + al256(4 * e)) : nullptr;
    // the caller's arrays when page-locked, the context's block otherwise
    const double* k_poses = (const double*)pinned_device_ptr(ctx, poses, 32 * e);
    if (!k_poses) { memcpy(h_poses, poses, 32 * e); k_poses = (const double*)pinned_device_ptr(ctx, h_poses, 32 * e); }
    double* k_steer = (double*)pinned_device_ptr(ctx, steer, 8 * e); double* k_speed = (double*)pinned_device_ptr(ctx, speed, 8 * e);
    int32_t* k_status = status ? (int32_t*)pinned_device_ptr(ctx, status, 4 * e) : nullptr;
    const bool own_steer = !k_steer, own_speed = !k_speed, own_status = status && !k_status;
    if (own_steer) k_steer = (double*)pinned_device_ptr(ctx, h_steer, 8 * e);
    if (own_speed) k_speed = (double*)pinned_device_ptr(ctx, h_speed, 8 * e);
    if (own_status) k_status = (int32_t*)pinned_device_ptr(ctx, h_status, 4 * e);
    if (!k_poses || !k_steer || !k_speed || (status && !k_status)) return set_error(ctx, F1P_ESTATE, "page-locked step block is not device-visible");
    // track ids: read in place when page-locked, else one copy into the arena
    const int32_t* k_tid = tracks ? (const int32_t*)pinned_device_ptr(ctx, track_id, 4 * e) : nullptr;
    if (tracks && !k_tid) {
        if ((rc = arena_reset(ctx, al256(4 * e)))) return rc;
        int32_t* d = (int32_t*)arena_take(ctx, 4 * e);
        F1P_HIP(ctx, hipMemcpyAsync(d, track_id, 4 * e, hipMemcpyHostToDevice, ctx->stream));
        k_tid = d;
    }
    // a step IS a link of a closed loop -- for the duration of the step.  The mode the caller set with f1p_lattice_set_closed_loop is restored
    // afterwards (the step used to arm it for good, and a later f1p_lattice_plan_* with prev_theta == NULL and the same batch shape
    // silently picked up -- and overwrote -- the step chain's headings).  The chain's headings stay in the context between steps.
    const bool was_armed = ctx->lattice_closed_loop;
    if (!was_armed && !ctx->step_chain) ctx->cl_valid = false;      // the first step of a chain of its own
    ctx->lattice_closed_loop = true;
    ClosedLoop cl;
    rc = cl_begin(ctx, nullptr, E, S, true, &cl);
    if (rc == F1P_OK)
        rc = launch_lattice(ctx, LATTICE_FULL, k_poses, nullptr, cl.prev, E, cfg, nullptr, nullptr, k_steer, k_speed, d_idx, nullptr, k_status, d_near,
                            d_traj, nullptr, nullptr, nullptr, cl.out, d_pose_copy, k_tid);
    ctx->lattice_closed_loop = was_armed;
    if (rc) return rc;
    cl_commit(ctx, cl, E, S);
    ctx->step_chain = !was_armed;
    ctx->step_traj_E = keep_traj ? E : 0; ctx->step_traj_S = S;
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (own_steer) memcpy(steer, h_steer, 8 * e);
    if (own_speed) memcpy(speed, h_speed, 8 * e);
    if (own_status) memcpy(status, h_status, 4 * e);
    return F1P_OK;
}

int f1p_lattice_step_batch(f1p_ctx* ctx, const double* poses, int32_t E, const f1p_lattice_cfg* cfg, double* steer, double* speed,
                           int32_t* status, int32_t keep_traj) {
    F1P_ENTER(ctx);
    return lattice_step_impl(ctx, poses, E, cfg, steer, speed, status, keep_traj, nullptr, false);
}

int f1p_lattice_step_tracks_batch(f1p_ctx* ctx, const double* poses, const int32_t* track_id, int32_t E, const f1p_lattice_cfg* cfg, double* steer,
                                  double* speed, int32_t* status, int32_t keep_traj) {
    F1P_ENTER(ctx);
    return lattice_step_impl(ctx, poses, E, cfg, steer, speed, status, keep_traj, track_id, true);
}

int f1p_lattice_fetch_traj(f1p_ctx* ctx, double* best_traj, int32_t E, int32_t S) {
    F1P_ENTER(ctx);
    if (!best_traj) return set_error(ctx, F1P_EINVAL, "best_traj is NULL");
    if (ctx->step_traj_E <= 0 || !ctx->d_step) return set_error(ctx, F1P_ESTATE, "no trajectories kept: call f1p_lattice_step_batch with keep_traj = 1 first");
    if (E != ctx->step_traj_E || S != ctx->step_traj_S) return set_error(ctx, F1P_EINVAL, "E / S differ from the last f1p_lattice_step_batch");
    const size_t e = (size_t)E;
    const char* d_traj = ctx->d_step + al256(32 * e) + 2 * al256(4 * e);
    F1P_HIP(ctx, hipMemcpyAsync(best_traj, d_traj, 32 * e * S, hipMemcpyDeviceToHost, ctx->stream));
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F1P_OK;
}

int f1p_lattice_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_state) {
    if (!ctx) return F1P_EINVAL;
    if (mixed < 0 || mixed > 3) return set_error(ctx, F1P_EINVAL, "mixed must be 0 (all fp64), 1 (f32 filter, the default), 2 (f32 filter at any batch size) or 3 (as 2, one ego per wave in the per-ego kernels)");
    ctx->lattice_mixed = mixed;
    ctx->d_dbg_lat_cost32 = d_cost32;
    ctx->d_dbg_lat_state = d_state;
    return F1P_OK;
}

int f1p_lattice_set_split(f1p_ctx* ctx, int32_t groups) {
    if (!ctx) return F1P_EINVAL;
    if (groups < 0 || groups > 16) return set_error(ctx, F1P_EINVAL, "groups must be in [0, 16]");
    if (groups > 0 && ctx->lat_obs.cur) return set_error(ctx, F1P_ESTATE, "lattice obstacles are set and run one workgroup per ego: clear them first (f1p_lattice_set_obstacles)");
    ctx->lattice_split = groups;
    return F1P_OK;
}

int f1p_lattice_set_clearance(f1p_ctx* ctx, int32_t stations_each_side) {
    if (!ctx) return F1P_EINVAL;
    if (stations_each_side < 0 || stations_each_side > 2) return set_error(ctx, F1P_EINVAL, "stations_each_side must be 0, 1 or 2");
    ctx->lattice_clear_r = stations_each_side;
    return F1P_OK;
}

int f1p_lattice_debug_queue(f1p_ctx* ctx, int32_t* entries_per_ego, int32_t E) {
    F1P_ENTER(ctx);
    if (!entries_per_ego || E < 1) return set_error(ctx, F1P_EINVAL, "entries_per_ego is NULL or E < 1");
    if (!ctx->d_mix_scratch || ctx->mix_last_E != E) return set_error(ctx, F1P_ESTATE, "no mixed-schedule plan of this batch size has run");
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    F1P_HIP(ctx, hipMemcpy(entries_per_ego, ctx->d_mix_scratch + ctx->mix_ego_n_off, sizeof(int32_t) * (size_t)E, hipMemcpyDeviceToHost));
    return F1P_OK;
}

int f1p_lattice_debug_bound(f1p_ctx* ctx, float* d_bound) {
    if (!ctx) return F1P_EINVAL;
    ctx->d_dbg_lat_bound = d_bound;
    return F1P_OK;
}

int f1p_lattice_debug_slack(f1p_ctx* ctx, const f1p_lattice_cfg* cfg, int32_t tracks, double* slack, float* slack_f) {
    if (!ctx || !cfg || !slack || !slack_f) return F1P_EINVAL;
    lookahead_slack(cfg, tracks ? ctx->trk_absmax : ctx->wp_absmax, slack, slack_f);
    return F1P_OK;
}

int f1p_lattice_set_order(f1p_ctx* ctx, int32_t heavy_first) {
    if (!ctx) return F1P_EINVAL;
    if (heavy_first < 0 || heavy_first > 1) return set_error(ctx, F1P_EINVAL, "heavy_first must be 0 or 1");
    ctx->lattice_order = heavy_first;
    return F1P_OK;
}

int f1p_lattice_debug_pass(f1p_ctx* ctx, int32_t* d_pass) {
    if (!ctx) return F1P_EINVAL;
    ctx->d_dbg_lat_pass = d_pass;
    return F1P_OK;
}

int f1p_lattice_debug_margins(f1p_ctx* ctx, int32_t enable, float margin_rel, float margin_abs) {
    if (!ctx) return F1P_EINVAL;
    ctx->dbg_margins = enable != 0; ctx->dbg_margin_rel = margin_rel; ctx->dbg_margin_abs = margin_abs;
    return F1P_OK;
}

int f1p_lattice_set_audit(f1p_ctx* ctx, int32_t every_n, int32_t n_egos) {
    if (!ctx) return F1P_EINVAL;
    if (every_n < 0 || n_egos < 0 || (every_n > 0 && n_egos < 1)) return set_error(ctx, F1P_EINVAL, "every_n >= 0 and, when auditing, n_egos >= 1");
    ctx->audit_every = every_n; ctx->audit_egos = n_egos;
    return F1P_OK;
}

int f1p_lattice_audit_read(f1p_ctx* ctx, uint64_t out[3], int32_t reset) {
    F1P_ENTER(ctx);
    if (!out) return set_error(ctx, F1P_EINVAL, "out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (!ctx->d_audit) return F1P_OK;
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[3];
    F1P_HIP(ctx, hipMemcpy(h, ctx->d_audit, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
    if (reset) F1P_HIP(ctx, hipMemset(ctx->d_audit, 0, sizeof(h)));
    return F1P_OK;
}

int f1p_lattice_set_pipeline(f1p_ctx* ctx, int32_t chunks) {
    if (!ctx) return F1P_EINVAL;
    if (chunks < 0 || chunks > 8) return set_error(ctx, F1P_EINVAL, "chunks must be in [0, 8]");
    ctx->lattice_chunks = chunks;
    return F1P_OK;
}

int f1p_lattice_profile(f1p_ctx* ctx, int32_t enable, float kernel_ms[4]) {
    F1P_ENTER(ctx);
    if (kernel_ms) {
        if (!ctx->lattice_profile || !ctx->lattice_profile_valid) return set_error(ctx, F1P_ESTATE, "no profiled mixed-schedule plan has run");
        F1P_HIP(ctx, hipEventSynchronize(ctx->ev_prof[4]));
        for (int k = 0; k < 4; ++k) F1P_HIP(ctx, hipEventElapsedTime(&kernel_ms[k], ctx->ev_prof[k], ctx->ev_prof[k + 1]));
    }
    if (enable && !ctx->ev_prof[0])
        for (auto& ev : ctx->ev_prof) F1P_HIP(ctx, hipEventCreate(&ev));
    ctx->lattice_profile = enable != 0;
    if (!enable) ctx->lattice_profile_valid = false;
    return F1P_OK;
}

int f1p_clothoid_sample_batch(f1p_ctx* ctx, const double* params, int32_t n, int32_t npts, double* rows) {
    F1P_ENTER(ctx);
    if (n < 0 || (n > 0 && (!params || !rows))) return set_error(ctx, F1P_EINVAL, "bad params / rows / n");
    if (npts < 1 || npts > 65536) return set_error(ctx, F1P_EINVAL, "npts must be in [1, 65536]");
    Stage s(ctx);
    s.need(8 * 3 * (size_t)n); s.need(8 * 4 * (size_t)n * npts);
    int rc = s.begin(); if (rc) return rc;
    const double* d_p;
    if ((rc = s.in(params, (size_t)3 * n, &d_p))) return rc;
    double* d_rows = s.out(rows, (size_t)4 * n * npts);
    if ((rc = launch_clothoid_sample(ctx, d_p, n, npts, d_rows))) return rc;
    return s.finish();
}

int f1p_clothoid_g1_batch(f1p_ctx* ctx, const double* goals, int32_t n, double* kappa0, double* dkappa, double* length, int32_t* ok) {
    F1P_ENTER(ctx);
    if (n < 0 || (n > 0 && !goals)) return set_error(ctx, F1P_EINVAL, "bad goals / n");
    Stage s(ctx);
    s.need(8 * 3 * (size_t)n); s.need(8 * (size_t)n, kappa0); s.need(8 * (size_t)n, dkappa); s.need(8 * (size_t)n, length); s.need(4 * (size_t)n, ok);
    int rc = s.begin(); if (rc) return rc;
    const double* d_g;
    if ((rc = s.in(goals, (size_t)3 * n, &d_g))) return rc;
    double* d_k0 = s.out(kappa0, n); double* d_dk = s.out(dkappa, n); double* d_L = s.out(length, n); int32_t* d_ok = s.out(ok, n);
    if ((rc = launch_clothoid_g1(ctx, d_g, n, d_k0, d_dk, d_L, d_ok))) return rc;
    return s.finish();
}
