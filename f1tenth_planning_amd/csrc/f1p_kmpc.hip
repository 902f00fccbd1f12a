// f1p_kmpc.hip -- the kinematic MPC: the shooting solver on given and on generated controls with its device-resident warm start, the reference's
// linearised QP with its own, and the reference extraction (whose *_batch body also serves the dynamic MPC's 7-column rows)
#include "f1p_host.h"

using namespace f1p;

namespace f1p {

// opts (nullable: the defaults) into *o, range-checked; `what` prefixes the error message
int qp_opts(f1p_ctx* ctx, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o, const char* what) {
    f1p_kmpc_qp_opts_default(o);
    if (opts) *o = *opts;
    if (o->max_iter < 0 || o->max_iter > 1000 || !(o->tol > 0) || !isfinite(o->tol))
        return set_error(ctx, F1P_EINVAL, std::string(what) + ": max_iter must be in [0, 1000] and tol finite and > 0");
    return F1P_OK;
}

// the cfg checks of the shooting path, the diagonal weights' and bounds' sanity, horizon <= 32 (n = 2T inputs, one lane each); opts
int validate_kmpc_qp(f1p_ctx* ctx, const f1p_kmpc_cfg* cfg, int E, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o) {
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if (cfg->horizon > 32) return set_error(ctx, F1P_EINVAL, "kmpc qp: horizon must be <= 32");
    if (cfg->horizon < 2) return set_error(ctx, F1P_EINVAL, "kmpc qp: horizon must be >= 2");
    for (int k = 0; k < 4; ++k)
        if (!(cfg->q[k] >= 0) || !(cfg->qf[k] >= 0) || !isfinite(cfg->q[k]) || !isfinite(cfg->qf[k]))
            return set_error(ctx, F1P_EINVAL, "kmpc qp: state weights must be finite and >= 0");
    for (int k = 0; k < 2; ++k)
        if (!(cfg->r[k] > 0) || !(cfg->rd[k] >= 0) || !isfinite(cfg->r[k]) || !isfinite(cfg->rd[k]))
            return set_error(ctx, F1P_EINVAL, "kmpc qp: input weights must be finite, r > 0 (strict convexity), rd >= 0");
    if (!(cfg->max_accel > 0) || !(cfg->max_steer > 0) || !(cfg->max_dsteer > 0) || !(cfg->max_speed >= cfg->min_speed))
        return set_error(ctx, F1P_EINVAL, "kmpc qp: bounds must be > 0 and max_speed >= min_speed");
    return qp_opts(ctx, opts, o, "kmpc qp");
}

int validate_ref(f1p_ctx* ctx, const void* states, const int32_t* track_id, bool tracks, int E, int horizon, double dt, double dl, const void* ref) {
    if (E < 0 || (E > 0 && (!states || (tracks && !track_id) || !ref)))
        return set_error(ctx, F1P_EINVAL, tracks ? "bad states / track_id / ref / E" : "bad states / ref / E");
    if (horizon < 1 || !(dt > 0) || !(dl > 0)) return set_error(ctx, F1P_EINVAL, "horizon, dt and dl must be positive");
    if (tracks) return need_tracks(ctx, true, false);
    if (ctx->n_wp < 2 || !ctx->has_psi) return set_error(ctx, F1P_ESTATE, "waypoints with a heading column are required");
    return F1P_OK;
}

int ref_batch_impl(f1p_ctx* ctx, int ncol, const double* states, const int32_t* track_id, bool tracks, int32_t E, int32_t horizon, double dt, double dl,
                   double* ref) {
    F1P_ENTER(ctx);
    int rc = validate_ref(ctx, states, track_id, tracks, E, horizon, dt, dl, ref); if (rc) return rc;
    Stage s(ctx);
    s.need(8 * 4 * (size_t)E); s.need(4 * (size_t)E, tracks); s.need(8 * (size_t)E * ncol * (horizon + 1));
    if ((rc = s.begin())) return rc;
    const double* d_s; const int32_t* d_tid = nullptr;
    if ((rc = s.in(states, (size_t)4 * E, &d_s))) return rc;
    if (tracks && (rc = s.in(track_id, (size_t)E, &d_tid))) return rc;
    double* d_ref = s.out(ref, (size_t)E * ncol * (horizon + 1));
    if (ncol == 4) rc = tracks ? launch_kmpc_ref_tracks(ctx, d_s, d_tid, E, horizon, dt, dl, d_ref) : launch_kmpc_ref(ctx, d_s, E, horizon, dt, dl, d_ref);
    else rc = tracks ? launch_stmpc_ref_tracks(ctx, d_s, d_tid, E, horizon, dt, dl, d_ref) : launch_stmpc_ref(ctx, d_s, E, horizon, dt, dl, d_ref);
    if (rc) return rc;
    return s.finish();
}

int collision_check(f1p_ctx* ctx, const ObsState& st, bool on, int n_sub, int n_sub_k, const char* who, bool kinematic, int E) {
    const std::string w = who;
    const bool split = kinematic && ctx->kmpc_groups > 0;
    if (st.cur) {                                                     // the discs: with or without the grid
        if (E != st.E)
            return set_error(ctx, F1P_ESTATE, w + " obstacles were set for " + std::to_string(st.E) + " egos, this plan has " + std::to_string(E) + " (f1p_" + w + "_set_obstacles)");
        if (split) return set_error(ctx, F1P_ESTATE, w + " obstacle test runs one workgroup per ego: f1p_kmpc_set_groups(0)");
    }
    if (!on) return F1P_OK;
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, w + " collision test is on but no occupancy grid is loaded (f1p_set_grid)");
    if (ctx->n_disc > 0)
        return set_error(ctx, F1P_ESTATE, w + " collision test is a point / disc test: remove the oriented footprint (f1p_set_footprint) and use f1p_inflate_grid");
    if (split) return set_error(ctx, F1P_ESTATE, w + " collision test runs one workgroup per ego: f1p_kmpc_set_groups(0)");
    const auto bad = [](int n) { return n < 1 || n > 16; };
    const bool two = n_sub_k != F1P_NO_NSUB_K;
    if (bad(n_sub) || (two && bad(n_sub_k)))
        return set_error(ctx, F1P_EINVAL, w + (two ? " collision test: n_sub and n_sub_k must be in [1, 16]" : " collision test: n_sub must be in [1, 16]"));
    return F1P_OK;
}

int set_obstacles(f1p_ctx* ctx, ObsState& st, const char* who, bool groups_matter, const double* obs, int32_t E, int32_t M, bool dev) {
    F1P_ENTER(ctx);
    const std::string w = who;
    if (!obs || M == 0) { st.cur = nullptr; st.E = 0; st.M = 0; return F1P_OK; }
    if (M < 1 || M > F1P_KMPC_MAX_OBS) return set_error(ctx, F1P_EINVAL, w + " obstacles: M must be in [1, 16]");
    if (E < 1) return set_error(ctx, F1P_EINVAL, w + " obstacles: E must be >= 1");
    if (groups_matter && ctx->kmpc_groups > 0) return set_error(ctx, F1P_ESTATE, w + " obstacle test runs one workgroup per ego: f1p_kmpc_set_groups(0)");
    if (dev) { st.cur = obs; st.E = E; st.M = M; return F1P_OK; }
    const size_t bytes = sizeof(double) * 5 * (size_t)E * M;
    if (bytes > st.bytes) {
        st.cur = nullptr; st.E = 0; st.M = 0;
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));              // no launch in flight reads the old copy
        if (st.d) (void)hipFree(st.d);
        st.d = nullptr; st.bytes = 0;
        F1P_HIP(ctx, hipMalloc((void**)&st.d, bytes));
        st.bytes = bytes;
    }
    // (pageable host memory: the copy has left the caller's array when this returns; stream order puts it after the plans already queued)
    F1P_HIP(ctx, hipMemcpyAsync(st.d, obs, bytes, hipMemcpyHostToDevice, ctx->stream));
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    st.cur = st.d; st.E = E; st.M = M;
    return F1P_OK;
}

}  // namespace f1p

// f1p_kmpc_set_collision's / f1p_kmpc_set_obstacles' preconditions, checked by every entry point that would launch the tested kernels
static int kmpc_collision_check(f1p_ctx* ctx, int E) { return collision_check(ctx, ctx->kmpc_obs, ctx->kmpc_collision, ctx->kmpc_col_nsub, F1P_NO_NSUB_K, "kmpc", true, E); }

int f1p_kmpc_set_collision(f1p_ctx* ctx, int32_t on, int32_t n_sub) {
    F1P_ENTER(ctx);
    if (n_sub < 1 || n_sub > 16) return set_error(ctx, F1P_EINVAL, "kmpc collision test: n_sub must be in [1, 16]");
    ctx->kmpc_collision = on != 0;
    ctx->kmpc_col_nsub = n_sub;
    return F1P_OK;
}

int f1p_kmpc_set_obstacles(f1p_ctx* ctx, const double* obs, int32_t E, int32_t M) { return set_obstacles(ctx, ctx->kmpc_obs, "kmpc", true, obs, E, M, false); }
int f1p_kmpc_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, int32_t E, int32_t M) { return set_obstacles(ctx, ctx->kmpc_obs, "kmpc", true, d_obs, E, M, true); }

void f1p_kmpc_cfg_default(f1p_kmpc_cfg* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->horizon = 8; cfg->n_rollouts = 512;
    cfg->dt = 0.1; cfg->wheelbase = 0.33; cfg->max_steer = 0.4189; cfg->max_dsteer = 3.141592653589793;
    cfg->max_speed = 6.0; cfg->min_speed = 0.0; cfg->max_accel = 3.0;
    const double q[4] = {13.5, 13.5, 5.5, 13.0};
    for (int i = 0; i < 4; ++i) { cfg->q[i] = q[i]; cfg->qf[i] = q[i]; }
    cfg->r[0] = 0.01; cfg->r[1] = 100.0; cfg->rd[0] = 0.01; cfg->rd[1] = 100.0;
}

// ---------------------------------------------------------------------------------------------------
int f1p_kmpc_shoot_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, int32_t E,
                       const f1p_kmpc_cfg* cfg, double* d_steer, double* d_speed, int32_t* d_best_idx,
                       double* d_best_cost, double* d_best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if (E > 0 && (!d_x0 || !d_ref || !d_controls || !d_steer || !d_speed || !d_best_idx))
        return set_error(ctx, F1P_EINVAL, "x0, ref, controls, steer, speed and best_idx are required");
    if ((rc = kmpc_collision_check(ctx, E))) return rc;
    return launch_kmpc_shoot(ctx, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
}

int f1p_kmpc_shoot_batch(f1p_ctx* ctx, const double* x0, const double* ref, const float* controls, int32_t E,
                         const f1p_kmpc_cfg* cfg, double* steer, double* speed, int32_t* best_idx, double* best_cost,
                         double* best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if (E > 0 && (!x0 || !ref || !controls || !steer || !speed || !best_idx))
        return set_error(ctx, F1P_EINVAL, "x0, ref, controls, steer, speed and best_idx are required");
    if ((rc = kmpc_collision_check(ctx, E))) return rc;
    const size_t T = cfg->horizon, R = cfg->n_rollouts, e = E;
    Stage s(ctx);
    s.need(8 * 4 * e); s.need(8 * e * 4 * (T + 1)); s.need(4 * e * T * 2 * R);
    s.need(8 * e); s.need(8 * e); s.need(4 * e); s.need(8 * e, best_cost); s.need(8 * e * T * 2, best_seq);
    if ((rc = s.begin())) return rc;
    const double *d_x0, *d_ref; const float* d_c;
    if ((rc = s.in(x0, 4 * e, &d_x0))) return rc;
    if ((rc = s.in(ref, e * 4 * (T + 1), &d_ref))) return rc;
    if ((rc = s.in(controls, e * T * 2 * R, &d_c))) return rc;
    double* d_steer = s.out(steer, e); double* d_speed = s.out(speed, e); int32_t* d_bi = s.out(best_idx, e);
    double* d_bc = s.out(best_cost, e); double* d_bs = s.out(best_seq, e * T * 2);
    if ((rc = launch_kmpc_shoot(ctx, d_x0, d_ref, d_c, E, cfg, d_steer, d_speed, d_bi, d_bc, d_bs))) return rc;
    return s.finish();
}

int f1p_kmpc_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_n_refined) {
    if (!ctx) return F1P_EINVAL;
    ctx->kmpc_mixed = mixed != 0;
    ctx->d_dbg_cost32 = d_cost32;
    ctx->d_dbg_nref = d_n_refined;
    return F1P_OK;
}

int f1p_kmpc_predict_batch(f1p_ctx* ctx, const double* x0, const double* oa, const double* od, int32_t E,
                           const f1p_kmpc_cfg* cfg, double* path) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if (E > 0 && (!x0 || !oa || !od || !path)) return set_error(ctx, F1P_EINVAL, "x0, oa, od and path are required");
    const size_t T = cfg->horizon, e = E;
    Stage s(ctx);
    s.need(8 * 4 * e); s.need(8 * e * T); s.need(8 * e * T); s.need(8 * e * 4 * (T + 1));
    if ((rc = s.begin())) return rc;
    const double *d_x0, *d_oa, *d_od;
    if ((rc = s.in(x0, 4 * e, &d_x0))) return rc;
    if ((rc = s.in(oa, e * T, &d_oa))) return rc;
    if ((rc = s.in(od, e * T, &d_od))) return rc;
    double* d_path = s.out(path, e * 4 * (T + 1));
    if ((rc = launch_kmpc_predict(ctx, d_x0, d_oa, d_od, E, cfg, d_path))) return rc;
    return s.finish();
}

int f1p_kmpc_ref_batch(f1p_ctx* ctx, const double* states, int32_t E, int32_t horizon, double dt, double dl, double* ref) {
    return ref_batch_impl(ctx, 4, states, nullptr, false, E, horizon, dt, dl, ref);
}

int f1p_kmpc_ref_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, int32_t horizon, double dt, double dl,
                              double* ref) {
    return ref_batch_impl(ctx, 4, states, track_id, true, E, horizon, dt, dl, ref);
}

int f1p_kmpc_ref_tracks_dev(f1p_ctx* ctx, const double* d_states, const int32_t* d_track_id, int32_t E, int32_t horizon, double dt, double dl,
                            double* d_ref) {
    F1P_ENTER(ctx);
    const int rc = validate_ref(ctx, d_states, d_track_id, true, E, horizon, dt, dl, d_ref); if (rc) return rc;
    return launch_kmpc_ref_tracks(ctx, d_states, d_track_id, E, horizon, dt, dl, d_ref);
}

int f1p_kmpc_sample_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_kmpc_cfg* cfg, uint64_t seed,
                                 double sigma_accel, double sigma_steer) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if (E > 0 && !d_controls) return set_error(ctx, F1P_EINVAL, "controls is NULL");
    return launch_kmpc_sample(ctx, d_controls, E, cfg, seed, sigma_accel, sigma_steer);
}

// ---------------------------------------------------------------------------------------------------
// shooting MPC with in-kernel control generation and a device-resident warm start
// ---------------------------------------------------------------------------------------------------
static int validate_sampler(f1p_ctx* ctx, const f1p_kmpc_sampler* smp) {
    if (!smp) return set_error(ctx, F1P_EINVAL, "sampler is NULL");
    if (!(smp->sigma_accel >= 0.0) || !(smp->sigma_steer >= 0.0) || !isfinite(smp->sigma_accel) || !isfinite(smp->sigma_steer))
        return set_error(ctx, F1P_EINVAL, "sampler sigmas must be finite and >= 0");
    return F1P_OK;
}

// one of the ctx's two kinematic warm buffers (shooting: f32, QP: fp64) for (E, T); a change of shape drops the old contents
static int ensure_kin_warm(f1p_ctx* ctx, WarmBuf* w, bool* valid, size_t elem_bytes, int E, int T) {
    bool fresh = false;
    const int rc = warm_ensure(ctx, w, elem_bytes * 2 * (size_t)E * T, E, T, 0, false, &fresh);
    if (fresh) *valid = false;
    return rc;
}
static int ensure_warm(f1p_ctx* ctx, int E, int T) { return ensure_kin_warm(ctx, &ctx->kmpc_warm, &ctx->kmpc_warm_valid, sizeof(float), E, T); }
static int ensure_qp_warm(f1p_ctx* ctx, int E, int T) { return ensure_kin_warm(ctx, &ctx->kmpc_qp_warm, &ctx->kmpc_qp_warm_valid, sizeof(double), E, T); }

int f1p_kmpc_plan_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, int32_t E, const f1p_kmpc_cfg* cfg,
                      const f1p_kmpc_sampler* smp, double* d_steer, double* d_speed, int32_t* d_best_idx,
                      double* d_best_cost, double* d_best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = validate_sampler(ctx, smp))) return rc;
    if (E == 0) return F1P_OK;
    if (!d_x0 || !d_ref || !d_steer || !d_speed || !d_best_idx) return set_error(ctx, F1P_EINVAL, "x0, ref, steer, speed and best_idx are required");
    if (cfg->n_rollouts > 8192) return set_error(ctx, F1P_EINVAL, "at most 8192 rollouts per plan");
    if ((rc = kmpc_collision_check(ctx, E))) return rc;
    if ((rc = ensure_warm(ctx, E, cfg->horizon))) return rc;
    float* warm = ctx->kmpc_warm.as<float>();
    const float* warm_in = (smp->use_warm && ctx->kmpc_warm_valid) ? warm : nullptr;
    rc = launch_kmpc_plan_gen(ctx, d_x0, d_ref, E, cfg, smp, warm_in, warm, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
    if (rc == F1P_OK) ctx->kmpc_warm_valid = true;
    return rc;
}

int f1p_kmpc_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_kmpc_cfg* cfg, double dl,
                        const f1p_kmpc_sampler* smp, double* steer, double* speed, int32_t* best_idx, double* best_cost,
                        double* best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = validate_sampler(ctx, smp))) return rc;
    if (E > 0 && (!x0 || !steer || !speed || !best_idx)) return set_error(ctx, F1P_EINVAL, "x0, steer, speed and best_idx are required");
    if (!(dl > 0)) return set_error(ctx, F1P_EINVAL, "dl must be > 0");
    if (ctx->n_wp < 2 || !ctx->has_psi) return set_error(ctx, F1P_ESTATE, "waypoints with a heading column are required");
    if ((rc = kmpc_collision_check(ctx, E))) return rc;
    const size_t T = cfg->horizon, e = E;
    Stage s(ctx);
    s.need(8 * 4 * e); s.need(8 * e * 4 * (T + 1));
    s.need(8 * e); s.need(8 * e); s.need(4 * e); s.need(8 * e, best_cost); s.need(8 * e * T * 2, best_seq);
    if ((rc = s.begin())) return rc;
    const double* d_x0;
    if ((rc = s.in(x0, 4 * e, &d_x0))) return rc;
    double* d_ref = (double*)arena_take(ctx, 8 * e * 4 * (T + 1));
    double* d_steer = s.out(steer, e); double* d_speed = s.out(speed, e); int32_t* d_bi = s.out(best_idx, e);
    double* d_bc = s.out(best_cost, e); double* d_bs = s.out(best_seq, e * T * 2);
    if ((rc = launch_kmpc_ref(ctx, d_x0, E, cfg->horizon, cfg->dt, dl, d_ref))) return rc;            // calc_ref_trajectory_kinematic :162-206
    if ((rc = f1p_kmpc_plan_dev(ctx, d_x0, d_ref, E, cfg, smp, d_steer, d_speed, d_bi, d_bc, d_bs))) return rc;
    return s.finish();
}

int f1p_kmpc_gen_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_kmpc_cfg* cfg, const f1p_kmpc_sampler* smp) {
    F1P_ENTER(ctx);
    int rc = validate_kmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = validate_sampler(ctx, smp))) return rc;
    if (E > 0 && !d_controls) return set_error(ctx, F1P_EINVAL, "controls is NULL");
    const bool warm = smp->use_warm && ctx->kmpc_warm_valid && ctx->kmpc_warm.is(E, cfg->horizon);
    return launch_kmpc_gen_controls(ctx, d_controls, E, cfg, smp, warm ? ctx->kmpc_warm.as<float>() : nullptr);
}

int f1p_kmpc_warm_reset(f1p_ctx* ctx) {
    if (!ctx) return F1P_EINVAL;
    ctx->kmpc_warm_valid = false;
    ctx->kmpc_warm_nonfinite = false;
    return F1P_OK;
}

int f1p_kmpc_warm_get(f1p_ctx* ctx, float* warm, int32_t E, int32_t T) {
    F1P_ENTER(ctx);
    if (!warm) return set_error(ctx, F1P_EINVAL, "warm is NULL");
    if (!ctx->kmpc_warm_valid || !ctx->kmpc_warm.is(E, T)) return set_error(ctx, F1P_ESTATE, "no warm start of this shape is held");
    return warm_download(ctx, &ctx->kmpc_warm, warm, sizeof(float) * 2 * (size_t)E * T);
}

int f1p_kmpc_warm_set(f1p_ctx* ctx, const float* warm, int32_t E, int32_t T) {
    F1P_ENTER(ctx);
    if (!warm || E < 1 || T < 1) return set_error(ctx, F1P_EINVAL, "bad warm / E / T");
    int rc = ensure_warm(ctx, E, T); if (rc) return rc;
    if ((rc = warm_upload(ctx, &ctx->kmpc_warm, warm, sizeof(float) * 2 * (size_t)E * T))) return rc;
    ctx->kmpc_warm_valid = true;
    // the only way a non-finite value enters a warm start (the kernels write clamped controls, or a NaN they were handed here)
    ctx->kmpc_warm_nonfinite = false;
    for (size_t q = 0; q < 2 * (size_t)E * T; ++q) if (!isfinite(warm[q])) { ctx->kmpc_warm_nonfinite = true; break; }
    return F1P_OK;
}

int f1p_kmpc_set_yaw_fixup(f1p_ctx* ctx, int32_t on) {
    F1P_ENTER(ctx);
    ctx->kmpc_yaw_fixup = on ? 1 : 0;
    return F1P_OK;
}

int f1p_kmpc_set_groups(f1p_ctx* ctx, int32_t groups) {
    if (!ctx) return F1P_EINVAL;
    if (groups < 0 || groups > 64) return set_error(ctx, F1P_EINVAL, "groups must be in [0, 64]");
    if (groups > 0 && ctx->kmpc_obs.cur) return set_error(ctx, F1P_ESTATE, "kmpc obstacles are set and run one workgroup per ego: clear them first (f1p_kmpc_set_obstacles)");
    ctx->kmpc_groups = groups;
    return F1P_OK;
}

// ---------------------------------------------------------------------------------------------------
// the reference's linearised QP (k_kmpc_qp.hip)
// ---------------------------------------------------------------------------------------------------
void f1p_kmpc_qp_opts_default(f1p_kmpc_qp_opts* opts) {
    if (!opts) return;
    memset(opts, 0, sizeof(*opts));
    opts->max_iter = 50; opts->tol = 1e-10;
}

// the kinematic QP as qp_call's model (f1p_host.h)
struct KinQp {
    using Cfg = f1p_kmpc_cfg;
    static constexpr int NX = 4, DUALS = 8, AVOID_MAX_T = 31;
    static constexpr const char *who = "kmpc", *avoid_cap = " qp avoid: horizon must be <= 31 (2T + 1 inputs, one lane each)";
    static constexpr bool EMPTY_RETURNS = false;
    static int validate(f1p_ctx* ctx, const Cfg* cfg, int E, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o) { return validate_kmpc_qp(ctx, cfg, E, opts, o); }
    static int launch(f1p_ctx* ctx, int E, const Cfg* cfg, int max_iter, double tol, const QpIo& io, const QpAvoidArgs* avoid, const QpWallArgs* walls) {
        return launch_kmpc_qp(ctx, E, cfg, max_iter, tol, io, avoid, walls);
    }
    static const ObsState& obs(const f1p_ctx* ctx) { return ctx->kmpc_obs; }
    static const f1p_kmpc_qp_avoid& av(const f1p_ctx* ctx) { return ctx->kmpc_qp_av; }
};

int f1p::validate_qp_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* a) {     // (f1p_stmpc_qp_avoid_* checks its numbers with it too)
    if (!(a->rho > 0) || !isfinite(a->rho) || !(a->lin >= 0) || !isfinite(a->lin) || !isfinite(a->margin))
        return set_error(ctx, F1P_EINVAL, "kmpc qp avoid: rho must be finite and > 0, lin finite and >= 0, margin finite");
    return F1P_OK;
}

int f1p::qp_set_avoid(f1p_ctx* ctx, f1p_kmpc_qp_avoid* state, const f1p_kmpc_qp_avoid* avoid) {
    F1P_ENTER(ctx);
    if (!avoid || !avoid->on) { state->on = 0; return F1P_OK; }
    const int rc = validate_qp_avoid(ctx, avoid); if (rc) return rc;
    *state = *avoid;
    state->on = 1; state->pad = 0;
    return F1P_OK;
}

// ---- wall rows (k_kmpc_qp.hip WALL) -------------------------------------------------------------------------------------
// (validate_qp_walls / qp_wall_args / qp_set_walls / qp_walls_call: f1p_host.h, one body with the dynamic QP)

int f1p_kmpc_qp_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                    const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* d_steer, double* d_speed, int32_t* d_status,
                    double* d_u, double* d_xk, double* d_obj, double* d_duals, int32_t* d_iters) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_xk; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    if (ctx && ctx->kmpc_qp_walls.on) return qp_walls_call<KinQp>(ctx, false, E, cfg, opts, io, nullptr, nullptr, &ctx->kmpc_qp_walls);
    return qp_call<KinQp>(ctx, false, E, cfg, opts, io, nullptr, nullptr);
}

int f1p_kmpc_qp_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                      const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status, double* u,
                      double* xk, double* obj, double* duals, int32_t* iters) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = xk; io.obj = obj; io.duals = duals; io.iters = iters;
    return qp_call<KinQp>(ctx, true, E, cfg, opts, io, nullptr, nullptr);
}

int f1p_kmpc_qp_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_kmpc_cfg* cfg, double dl, const f1p_kmpc_qp_opts* opts,
                           double* steer, double* speed, int32_t* status, double* u, double* obj) {
    F1P_ENTER(ctx);
    f1p_kmpc_qp_opts o;
    int rc = validate_kmpc_qp(ctx, cfg, E, opts, &o); if (rc) return rc;
    if (E > 0 && (!x0 || !steer || !speed || !status)) return set_error(ctx, F1P_EINVAL, "x0, steer, speed and status are required");
    if (!(dl > 0)) return set_error(ctx, F1P_EINVAL, "dl must be > 0");
    if (ctx->n_wp < 2 || !ctx->has_psi) return set_error(ctx, F1P_ESTATE, "waypoints with a heading column are required");
    if (E == 0) return F1P_OK;
    const bool av_on = ctx->kmpc_qp_av.on, walls_on = ctx->kmpc_qp_walls.on;
    QpWallArgs wl;
    if (walls_on && !av_on && cfg->horizon > KinQp::AVOID_MAX_T) return set_error(ctx, F1P_EINVAL, std::string(KinQp::who) + KinQp::avoid_cap);
    if (walls_on && (rc = qp_wall_args<KinQp>(ctx, &ctx->kmpc_qp_walls, &wl))) return rc;
    if (av_on && (rc = qp_avoid_plan_check<KinQp>(ctx, cfg, E))) return rc;
    const size_t T = cfg->horizon, e = E;
    if ((rc = ensure_qp_warm(ctx, E, cfg->horizon))) return rc;
    Stage s(ctx);
    s.need(8 * 4 * e); s.need(8 * e * 4 * (T + 1));
    s.need(8 * e); s.need(8 * e); s.need(4 * e); s.need(8 * e * T * 2, u); s.need(8 * e, obj);
    if ((rc = s.begin())) return rc;
    const double* d_x0;
    if ((rc = s.in(x0, 4 * e, &d_x0))) return rc;
    double* d_ref = (double*)arena_take(ctx, 8 * e * 4 * (T + 1));
    double* d_steer = s.out(steer, e); double* d_speed = s.out(speed, e); int32_t* d_st = s.out(status, e);
    double* d_u = s.out(u, e * T * 2); double* d_obj = s.out(obj, e);
    if ((rc = launch_kmpc_ref(ctx, d_x0, E, cfg->horizon, cfg->dt, dl, d_ref))) return rc;            // calc_ref_trajectory_kinematic :162-206
    const double* warm = ctx->kmpc_qp_warm_valid ? ctx->kmpc_qp_warm.as<double>() : nullptr;                   // None on the first call (:461-463)
    // (oa, od) interleaved in the warm buffer [E][T][2]: stride 2; each ego's group reads its slice before it writes it
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = warm; io.pd = warm ? warm + 1 : nullptr; io.pstride = 2;
    io.steer = d_steer; io.speed = d_speed; io.status = d_st; io.u = d_u; io.obj = d_obj; io.warm_out = ctx->kmpc_qp_warm.as<double>();
    // (walls without set_avoid: no discs, the context's rho and lin)
    const QpAvoidArgs av(av_on ? ctx->kmpc_obs.cur : nullptr, av_on ? ctx->kmpc_obs.M : 0, ctx->kmpc_qp_av);
    rc = launch_kmpc_qp(ctx, E, cfg, o.max_iter, o.tol, io, av_on || walls_on ? &av : nullptr, walls_on ? &wl : nullptr);
    if (rc) return rc;
    ctx->kmpc_qp_warm_valid = true;
    return s.finish();
}

// ---- moving-disc avoidance rows (k_kmpc_qp.hip AV) -----------------------------------------------------------------------------------
void f1p_kmpc_qp_avoid_default(f1p_kmpc_qp_avoid* avoid) {
    if (!avoid) return;
    memset(avoid, 0, sizeof(*avoid));
    avoid->margin = 0.0; avoid->rho = 1e4; avoid->lin = 10.0;
}

int f1p_kmpc_qp_set_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* avoid) { return qp_set_avoid(ctx, ctx ? &ctx->kmpc_qp_av : nullptr, avoid); }

int f1p_kmpc_qp_avoid_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                          const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                          const f1p_kmpc_qp_avoid* avoid, double* d_steer, double* d_speed, int32_t* d_status, double* d_u, double* d_xk,
                          double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps, double* d_planes, double* d_avoid_duals) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_xk; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    QpAvoidArgs av;
    av.obs = d_obs; av.M = M; av.eps = d_eps; av.planes = d_planes; av.duals = d_avoid_duals;
    return qp_call<KinQp>(ctx, false, E, cfg, opts, io, &av, avoid);
}

int f1p_kmpc_qp_avoid_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                            const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                            const f1p_kmpc_qp_avoid* avoid, double* steer, double* speed, int32_t* status, double* u, double* xk,
                            double* obj, double* duals, int32_t* iters, double* eps, double* planes, double* avoid_duals) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = xk; io.obj = obj; io.duals = duals; io.iters = iters;
    QpAvoidArgs av;
    av.obs = obs; av.M = M; av.eps = eps; av.planes = planes; av.duals = avoid_duals;
    return qp_call<KinQp>(ctx, true, E, cfg, opts, io, &av, avoid);
}

void f1p_kmpc_qp_walls_default(f1p_kmpc_qp_walls* walls) {
    if (!walls) return;
    memset(walls, 0, sizeof(*walls));
    walls->n_samples = 48; walls->margin = 0.0;
}

int f1p_kmpc_qp_set_walls(f1p_ctx* ctx, const f1p_kmpc_qp_walls* walls) { return qp_set_walls<KinQp>(ctx, ctx ? &ctx->kmpc_qp_walls : nullptr, walls); }

int f1p_kmpc_qp_walls_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_prev, int32_t E,
                          const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                          const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* d_steer, double* d_speed,
                          int32_t* d_status, double* d_u, double* d_xk, double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps,
                          double* d_planes, double* d_avoid_duals) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_xk; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    QpAvoidArgs av;
    av.obs = d_obs; av.M = M; av.eps = d_eps; av.planes = d_planes; av.duals = d_avoid_duals;
    return qp_walls_call<KinQp>(ctx, false, E, cfg, opts, io, &av, avoid, walls);
}

int f1p_kmpc_qp_walls_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_prev, int32_t E,
                            const f1p_kmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                            const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* steer, double* speed, int32_t* status,
                            double* u, double* xk, double* obj, double* duals, int32_t* iters, double* eps, double* planes,
                            double* avoid_duals) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = xk; io.obj = obj; io.duals = duals; io.iters = iters;
    QpAvoidArgs av;
    av.obs = obs; av.M = M; av.eps = eps; av.planes = planes; av.duals = avoid_duals;
    return qp_walls_call<KinQp>(ctx, true, E, cfg, opts, io, &av, avoid, walls);
}

int f1p_kmpc_qp_warm_reset(f1p_ctx* ctx) {
    if (!ctx) return F1P_EINVAL;
    ctx->kmpc_qp_warm_valid = false;
    return F1P_OK;
}

int f1p_kmpc_qp_warm_get(f1p_ctx* ctx, double* warm, int32_t E, int32_t T) {
    F1P_ENTER(ctx);
    if (!warm) return set_error(ctx, F1P_EINVAL, "warm is NULL");
    if (!ctx->kmpc_qp_warm_valid || !ctx->kmpc_qp_warm.is(E, T)) return set_error(ctx, F1P_ESTATE, "no qp warm start of this shape is held");
    return warm_download(ctx, &ctx->kmpc_qp_warm, warm, sizeof(double) * 2 * (size_t)E * T);
}

int f1p_kmpc_qp_warm_set(f1p_ctx* ctx, const double* warm, int32_t E, int32_t T) {
    F1P_ENTER(ctx);
    if (!warm || E < 1 || T < 1) return set_error(ctx, F1P_EINVAL, "bad warm / E / T");
    int rc = ensure_qp_warm(ctx, E, T); if (rc) return rc;
    if ((rc = warm_upload(ctx, &ctx->kmpc_qp_warm, warm, sizeof(double) * 2 * (size_t)E * T))) return rc;
    ctx->kmpc_qp_warm_valid = true;
    return F1P_OK;
}

int f1p_kmpc_qp_set_pack(f1p_ctx* ctx, int32_t egos_per_wave) {
    if (!ctx) return F1P_EINVAL;
    if (egos_per_wave != 0 && egos_per_wave != 1 && egos_per_wave != 4) return set_error(ctx, F1P_EINVAL, "egos_per_wave must be 0, 1 or 4");
    ctx->kmpc_qp_pack = egos_per_wave;
    return F1P_OK;
}
