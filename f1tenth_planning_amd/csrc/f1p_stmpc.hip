// f1p_stmpc.hip -- the dynamic (single-track) MPC: shooting on given and on generated controls, the reference's linearised QP, and
// STMPCPlanner.plan with either solver -- the model switch between the dynamic and the kinematic branch is made on the host (BranchSplit)
#include "f1p_host.h"

using namespace f1p;

// The dynamic MPC's model switch, made on the host (dynamic_mpc.py:168): the egos of one plan call in two branches -- 1: dynamic (:181-191),
// 0: kinematic (:168-180), each with its own horizon, time step and reference spacing -- each compacted, uploaded and given its reference, and a
// branch's compact rows put back in the caller's order.  What is solved on the references, the result columns and the warm-start rules are the
// callers' (the QP plan and the shooting plan below).  The uploads read this struct's own vectors, one per branch and none reused, so
// nothing waits in the middle of a call -- and the struct must outlive the stream's work: the callers hold a StreamDrain declared after it.
struct BranchSplit {
    f1p_ctx* ctx;
    const double* x0;                                 // [E][7] the caller's states
    const int32_t* track_id;                          // [E] on the host: ego e's references from track track_id[e]; null: all from the raceline
    int T[2]; double dt[2], dl[2];
    int W;                                            // steps per ego in the caller's rows: max(T[1], T[0])
    std::vector<int32_t> idx[2], bad;                 // the egos of each branch, ascending; those whose track id is outside [0, K): in neither
    std::vector<int32_t> htid[2]; std::vector<double> hx[2], h7;   // what prepare() uploads
    int32_t *d_idx[2] = {}, *d_tid[2] = {};           // a branch's egos (indices into the caller's batch) and their track ids
    double *d_s4[2] = {}, *d_ref7[2] = {};            // its (x, y, v, yaw) rows and its 7-column reference [nb][7][T[b] + 1]
    double *d_x7 = nullptr, *d_ref4 = nullptr;        // the dynamic branch's full states; the kinematic branch's 4-column reference

    BranchSplit(f1p_ctx* c, const double* x0_, const int32_t* track_id_, int E, double v_ks, const f1p_stmpc_cfg* dcfg, double dl_,
                const f1p_kmpc_cfg* kcfg, double dlk)
        : ctx(c), x0(x0_), track_id(track_id_), T{kcfg->horizon, dcfg->horizon}, dt{kcfg->dt, dcfg->dt}, dl{dlk, dl_}, W(std::max(T[0], T[1])) {
        for (int e = 0; e < E; ++e) {
            if (track_id && (track_id[e] < 0 || track_id[e] >= ctx->trk_K)) { bad.push_back(e); continue; }   // k_stmpc_ref_tracks's test
            idx[!(x0[(size_t)e * 7 + 3] <= v_ks)].push_back(e);
        }
    }
    // what prepare() takes from the arena
    size_t arena_bytes() const {
        size_t n = al256(8 * 7 * idx[1].size()) + al256(8 * 4 * (size_t)(T[0] + 1) * idx[0].size());
        for (int b = 0; b < 2; ++b) {
            const size_t nb = idx[b].size();
            n += al256(4 * nb) + al256(8 * 4 * nb) + al256(8 * 7 * (size_t)(T[b] + 1) * nb) + (track_id ? al256(4 * nb) : 0);
        }
        return n;
    }
    // branch b (not empty): index list, states and track ids to the device, then its reference -- calc_ref_trajectory (:195-233) with the branch's
    // (T, dt, dl); for the kinematic branch rows 0, 1, 3, 4 of it (:237-276)
    int prepare(int b, StreamDrain& io) {
        const size_t nb = idx[b].size();
        d_idx[b] = (int32_t*)arena_take(ctx, 4 * nb);
        d_s4[b] = (double*)arena_take(ctx, 8 * 4 * nb);
        d_ref7[b] = (double*)arena_take(ctx, 8 * 7 * (size_t)(T[b] + 1) * nb);
        hx[b].resize(nb * 4);
        for (size_t k = 0; k < nb; ++k) {
            const double* s = x0 + (size_t)idx[b][k] * 7;
            hx[b][4 * k] = s[0]; hx[b][4 * k + 1] = s[1]; hx[b][4 * k + 2] = s[3]; hx[b][4 * k + 3] = s[4];     // (x, y, v, yaw)
        }
        int rc = io.copy(d_idx[b], idx[b].data(), 4 * nb, hipMemcpyHostToDevice); if (rc) return rc;
        if ((rc = io.copy(d_s4[b], hx[b].data(), 8 * 4 * nb, hipMemcpyHostToDevice))) return rc;
        if (track_id) {                                                      // this branch's slice of the ids
            d_tid[b] = (int32_t*)arena_take(ctx, 4 * nb);
            htid[b].resize(nb);
            for (size_t k = 0; k < nb; ++k) htid[b][k] = track_id[idx[b][k]];
            if ((rc = io.copy(d_tid[b], htid[b].data(), 4 * nb, hipMemcpyHostToDevice))) return rc;
        }
        if (b) {
            d_x7 = (double*)arena_take(ctx, 8 * 7 * nb);
            h7.resize(nb * 7);
            for (size_t k = 0; k < nb; ++k) memcpy(&h7[7 * k], x0 + (size_t)idx[b][k] * 7, 7 * sizeof(double));
            if ((rc = io.copy(d_x7, h7.data(), 8 * 7 * nb, hipMemcpyHostToDevice))) return rc;
        } else d_ref4 = (double*)arena_take(ctx, 8 * 4 * (size_t)(T[0] + 1) * nb);
        if ((rc = track_id ? launch_stmpc_ref_tracks(ctx, d_s4[b], d_tid[b], (int)nb, T[b], dt[b], dl[b], d_ref7[b])
                           : launch_stmpc_ref(ctx, d_s4[b], (int)nb, T[b], dt[b], dl[b], d_ref7[b]))) return rc;
        return b ? F1P_OK : launch_stmpc_qp_kref(ctx, d_ref7[0], (int)nb, T[0], d_ref4);
    }
    // row k of branch b's compact rows [nb][2 T[b]] (on the host) -> out [E][W][2] in the caller's order: NaN behind the branch's horizon, and all NaN unless keep
    void scatter_row(int b, size_t k, const double* rows, bool keep, double* out) const {
        const size_t n = 2 * (size_t)T[b];
        double* ue = out + (size_t)idx[b][k] * W * 2;
        for (size_t j = 0; j < (size_t)W * 2; ++j) ue[j] = keep && j < n ? rows[k * n + j] : nan("");
    }
};

// ---------------------------------------------------------------------------------------------------
// dynamic single-track shooting
// ---------------------------------------------------------------------------------------------------
void f1p_stmpc_cfg_default(f1p_stmpc_cfg* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->horizon = 40; cfg->n_rollouts = 512;
    cfg->dt = 0.025; cfg->wheelbase = 0.33; cfg->max_steer = 0.4189; cfg->max_steer_v = 3.2;
    cfg->max_speed = 6.0; cfg->min_speed = 0.0; cfg->max_accel = 3.0;
    const double q[7] = {32.0, 32.0, 0.0, 1.0, 0.5, 0.0, 0.0};
    for (int i = 0; i < 7; ++i) { cfg->q[i] = q[i]; cfg->qf[i] = q[i]; }
    cfg->r[0] = 0.5; cfg->r[1] = 0.01; cfg->rd[0] = 0.3; cfg->rd[1] = 0.01;
    const double p[8] = {3.74, 0.15875, 0.17145, 0.074, 4.718, 5.4562, 0.04712, 1.0489};
    for (int i = 0; i < 8; ++i) cfg->params[i] = p[i];
}

int f1p_stmpc_predict_batch(f1p_ctx* ctx, const double* x0, const double* oa, const double* od_v, int32_t E,
                            const f1p_stmpc_cfg* cfg, double* path) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if (E > 0 && (!x0 || !oa || !od_v || !path)) return set_error(ctx, F1P_EINVAL, "x0, oa, od_v and path are required");
    const size_t T = cfg->horizon, e = E;
    Stage s(ctx);
    s.need(8 * 7 * e); s.need(8 * e * T); s.need(8 * e * T); s.need(8 * e * 7 * (T + 1));
    if ((rc = s.begin())) return rc;
    const double *d_x0, *d_oa, *d_od;
    if ((rc = s.in(x0, 7 * e, &d_x0))) return rc;
    if ((rc = s.in(oa, e * T, &d_oa))) return rc;
    if ((rc = s.in(od_v, e * T, &d_od))) return rc;
    double* d_path = s.out(path, e * 7 * (T + 1));
    if ((rc = launch_stmpc_predict(ctx, d_x0, d_oa, d_od, E, cfg, d_path))) return rc;
    return s.finish();
}

int f1p_stmpc_ref_batch(f1p_ctx* ctx, const double* states, int32_t E, int32_t horizon, double dt, double dl, double* ref) {
    return ref_batch_impl(ctx, 7, states, nullptr, false, E, horizon, dt, dl, ref);
}

int f1p_stmpc_ref_tracks_batch(f1p_ctx* ctx, const double* states, const int32_t* track_id, int32_t E, int32_t horizon, double dt, double dl,
                               double* ref) {
    return ref_batch_impl(ctx, 7, states, track_id, true, E, horizon, dt, dl, ref);
}

int f1p_stmpc_ref_tracks_dev(f1p_ctx* ctx, const double* d_states, const int32_t* d_track_id, int32_t E, int32_t horizon, double dt, double dl,
                             double* d_ref) {
    F1P_ENTER(ctx);
    const int rc = validate_ref(ctx, d_states, d_track_id, true, E, horizon, dt, dl, d_ref); if (rc) return rc;
    return launch_stmpc_ref_tracks(ctx, d_states, d_track_id, E, horizon, dt, dl, d_ref);
}

int f1p_stmpc_set_mode(f1p_ctx* ctx, int32_t mixed, float* d_cost32, int32_t* d_n_refined) {
    if (!ctx) return F1P_EINVAL;
    ctx->stmpc_mixed = mixed != 0;
    ctx->d_dbg_st_cost32 = d_cost32; ctx->d_dbg_st_nref = d_n_refined;
    return F1P_OK;
}

// f1p_stmpc_set_collision's preconditions, checked by every entry point that would launch the tested kernels -- before anything is launched
// or any warm-start tag is touched.  kinematic: the call may run f1p_stmpc_plan_batch's kinematic branch (one workgroup per ego with the test)
// E: the caller's ego count (f1p_stmpc_set_obstacles' rows are in the caller's order: for plan_batch the batch's E, not a branch's)
// (collision_check and set_obstacles, which both planners share, are defined in f1p_kmpc.hip and declared in f1p_host.h)
static int stmpc_collision_check(f1p_ctx* ctx, bool kinematic, int E) {
    return collision_check(ctx, ctx->stmpc_obs, ctx->stmpc_collision, ctx->stmpc_col_nsub, ctx->stmpc_col_nsub_k, "stmpc", kinematic, E);
}

int f1p_stmpc_set_collision(f1p_ctx* ctx, int32_t on, int32_t n_sub, int32_t n_sub_k) {
    F1P_ENTER(ctx);
    if (n_sub < 1 || n_sub > 16 || n_sub_k < 1 || n_sub_k > 16)
        return set_error(ctx, F1P_EINVAL, "stmpc collision test: n_sub and n_sub_k must be in [1, 16]");
    ctx->stmpc_collision = on != 0;
    ctx->stmpc_col_nsub = n_sub; ctx->stmpc_col_nsub_k = n_sub_k;
    return F1P_OK;
}

// (a state of its own beside f1p_kmpc_set_obstacles'; f1p_kmpc_set_groups does not bear on the dynamic filter)
int f1p_stmpc_set_obstacles(f1p_ctx* ctx, const double* obs, int32_t E, int32_t M) { return set_obstacles(ctx, ctx->stmpc_obs, "stmpc", false, obs, E, M, false); }
int f1p_stmpc_set_obstacles_dev(f1p_ctx* ctx, const double* d_obs, int32_t E, int32_t M) { return set_obstacles(ctx, ctx->stmpc_obs, "stmpc", false, d_obs, E, M, true); }

int f1p_stmpc_shoot_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const float* d_controls, int32_t E,
                        const f1p_stmpc_cfg* cfg, double* d_steer, double* d_speed, int32_t* d_best_idx,
                        double* d_best_cost, double* d_best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = stmpc_collision_check(ctx, false, E))) return rc;
    if (E > 0 && (!d_x0 || !d_ref || !d_controls || !d_steer || !d_speed || !d_best_idx))
        return set_error(ctx, F1P_EINVAL, "x0, ref, controls, steer, speed and best_idx are required");
    return launch_stmpc_shoot(ctx, d_x0, d_ref, d_controls, E, cfg, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
}

int f1p_stmpc_shoot_batch(f1p_ctx* ctx, const double* x0, const double* ref, const float* controls, int32_t E,
                          const f1p_stmpc_cfg* cfg, double* steer, double* speed, int32_t* best_idx, double* best_cost,
                          double* best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = stmpc_collision_check(ctx, false, E))) return rc;
    if (E > 0 && (!x0 || !ref || !controls || !steer || !speed || !best_idx))
        return set_error(ctx, F1P_EINVAL, "x0, ref, controls, steer, speed and best_idx are required");
    const size_t T = cfg->horizon, R = cfg->n_rollouts, e = E;
    Stage s(ctx);
    s.need(8 * 7 * e); s.need(8 * e * 7 * (T + 1)); s.need(4 * e * T * 2 * R);
    s.need(8 * e); s.need(8 * e); s.need(4 * e); s.need(8 * e, best_cost); s.need(8 * e * T * 2, best_seq);
    if ((rc = s.begin())) return rc;
    const double *d_x0, *d_ref; const float* d_c;
    if ((rc = s.in(x0, 7 * e, &d_x0))) return rc;
    if ((rc = s.in(ref, e * 7 * (T + 1), &d_ref))) return rc;
    if ((rc = s.in(controls, e * T * 2 * R, &d_c))) return rc;
    double* d_steer = s.out(steer, e); double* d_speed = s.out(speed, e); int32_t* d_bi = s.out(best_idx, e);
    double* d_bc = s.out(best_cost, e); double* d_bs = s.out(best_seq, e * T * 2);
    if ((rc = launch_stmpc_shoot(ctx, d_x0, d_ref, d_c, E, cfg, d_steer, d_speed, d_bi, d_bc, d_bs))) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------------
// the reference's linearised dynamic-MPC QP (k_stmpc_qp.hip) and STMPCPlanner.plan with it
// ---------------------------------------------------------------------------------------------------
// the cfg checks of the shooting path, diagonal weights and bounds sane, 2 <= horizon <= F1P_STMPC_QP_MAX_T; opts
static int validate_stmpc_qp(f1p_ctx* ctx, const f1p_stmpc_cfg* cfg, int E, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o) {
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if (cfg->horizon > F1P_STMPC_QP_MAX_T) return set_error(ctx, F1P_EINVAL, "stmpc qp: horizon must be <= F1P_STMPC_QP_MAX_T (44)");
    if (cfg->horizon < 2) return set_error(ctx, F1P_EINVAL, "stmpc qp: horizon must be >= 2");
    for (int k = 0; k < 7; ++k)
        if (!(cfg->q[k] >= 0) || !(cfg->qf[k] >= 0) || !isfinite(cfg->q[k]) || !isfinite(cfg->qf[k]))
            return set_error(ctx, F1P_EINVAL, "stmpc qp: state weights must be finite and >= 0");
    for (int k = 0; k < 2; ++k)
        if (!(cfg->r[k] > 0) || !(cfg->rd[k] >= 0) || !isfinite(cfg->r[k]) || !isfinite(cfg->rd[k]))
            return set_error(ctx, F1P_EINVAL, "stmpc qp: input weights must be finite, r > 0 (strict convexity), rd >= 0");
    if (!(cfg->max_accel > 0) || !(cfg->max_steer > 0) || !(cfg->max_steer_v > 0) || !(cfg->max_speed >= cfg->min_speed))
        return set_error(ctx, F1P_EINVAL, "stmpc qp: bounds must be > 0 and max_speed >= min_speed");
    for (int k = 0; k < 8; ++k)
        if (!isfinite(cfg->params[k])) return set_error(ctx, F1P_EINVAL, "stmpc qp: vehicle parameters must be finite");
    return qp_opts(ctx, opts, o, "stmpc qp");
}

// the dynamic QP as qp_call's model (f1p_host.h)
struct DynQp {
    using Cfg = f1p_stmpc_cfg;
    static constexpr int NX = 7, DUALS = 10, AVOID_MAX_T = F1P_STMPC_QP_AVOID_MAX_T;
    static constexpr const char *who = "stmpc", *avoid_cap = " qp avoid: horizon must be <= F1P_STMPC_QP_AVOID_MAX_T (40: the packed avoidance rows beside H and the Newton matrix in LDS)";
    static constexpr bool EMPTY_RETURNS = true;
    static int validate(f1p_ctx* ctx, const Cfg* cfg, int E, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o) { return validate_stmpc_qp(ctx, cfg, E, opts, o); }
    static int launch(f1p_ctx* ctx, int E, const Cfg* cfg, int max_iter, double tol, const QpIo& io, const QpAvoidArgs* avoid, const QpWallArgs* walls) {
        return launch_stmpc_qp(ctx, E, cfg, max_iter, tol, io, avoid, walls);
    }
    static const ObsState& obs(const f1p_ctx* ctx) { return ctx->stmpc_obs; }
    static const f1p_kmpc_qp_avoid& av(const f1p_ctx* ctx) { return ctx->stmpc_qp_av; }
};

int64_t f1p_stmpc_qp_avoid_lds_bytes(int32_t horizon) { return horizon < 2 ? -1 : (int64_t)stmpc_qp_avoid_lds_bytes(horizon); }

int f1p_stmpc_qp_set_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* avoid) { return qp_set_avoid(ctx, ctx ? &ctx->stmpc_qp_av : nullptr, avoid); }

int f1p_stmpc_qp_avoid_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev,
                           int32_t E, const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                           const f1p_kmpc_qp_avoid* avoid, double* d_steer, double* d_speed, int32_t* d_status, double* d_u, double* d_x,
                           double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps, double* d_planes, double* d_avoid_duals) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_v_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_x; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    QpAvoidArgs av;
    av.obs = d_obs; av.M = M; av.eps = d_eps; av.planes = d_planes; av.duals = d_avoid_duals;
    return qp_call<DynQp>(ctx, false, E, cfg, opts, io, &av, avoid);
}

int f1p_stmpc_qp_avoid_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                             const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                             const f1p_kmpc_qp_avoid* avoid, double* steer, double* speed, int32_t* status, double* u, double* x,
                             double* obj, double* duals, int32_t* iters, double* eps, double* planes, double* avoid_duals) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_v_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = x; io.obj = obj; io.duals = duals; io.iters = iters;
    QpAvoidArgs av;
    av.obs = obs; av.M = M; av.eps = eps; av.planes = planes; av.duals = avoid_duals;
    return qp_call<DynQp>(ctx, true, E, cfg, opts, io, &av, avoid);
}

int f1p_stmpc_qp_set_walls(f1p_ctx* ctx, const f1p_kmpc_qp_walls* walls) { return qp_set_walls<DynQp>(ctx, ctx ? &ctx->stmpc_qp_walls : nullptr, walls); }

int f1p_stmpc_qp_walls_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev,
                           int32_t E, const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* d_obs, int32_t M,
                           const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* d_steer, double* d_speed,
                           int32_t* d_status, double* d_u, double* d_x, double* d_obj, double* d_duals, int32_t* d_iters, double* d_eps,
                           double* d_planes, double* d_avoid_duals) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_v_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_x; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    QpAvoidArgs av;
    av.obs = d_obs; av.M = M; av.eps = d_eps; av.planes = d_planes; av.duals = d_avoid_duals;
    return qp_walls_call<DynQp>(ctx, false, E, cfg, opts, io, &av, avoid, walls);
}

int f1p_stmpc_qp_walls_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                             const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, const double* obs, int32_t M,
                             const f1p_kmpc_qp_avoid* avoid, const f1p_kmpc_qp_walls* walls, double* steer, double* speed, int32_t* status,
                             double* u, double* x, double* obj, double* duals, int32_t* iters, double* eps, double* planes,
                             double* avoid_duals) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_v_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = x; io.obj = obj; io.duals = duals; io.iters = iters;
    QpAvoidArgs av;
    av.obs = obs; av.M = M; av.eps = eps; av.planes = planes; av.duals = avoid_duals;
    return qp_walls_call<DynQp>(ctx, true, E, cfg, opts, io, &av, avoid, walls);
}

int f1p_stmpc_qp_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, const double* d_oa_prev, const double* d_od_v_prev, int32_t E,
                     const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* d_steer, double* d_speed, int32_t* d_status,
                     double* d_u, double* d_x, double* d_obj, double* d_duals, int32_t* d_iters) {
    QpIo io;
    io.x0 = d_x0; io.ref = d_ref; io.pa = d_oa_prev; io.pd = d_od_v_prev;
    io.steer = d_steer; io.speed = d_speed; io.status = d_status; io.u = d_u; io.x = d_x; io.obj = d_obj; io.duals = d_duals; io.iters = d_iters;
    if (ctx && ctx->stmpc_qp_walls.on) return qp_walls_call<DynQp>(ctx, false, E, cfg, opts, io, nullptr, nullptr, &ctx->stmpc_qp_walls);
    return qp_call<DynQp>(ctx, false, E, cfg, opts, io, nullptr, nullptr);
}

int f1p_stmpc_qp_batch(f1p_ctx* ctx, const double* x0, const double* ref, const double* oa_prev, const double* od_v_prev, int32_t E,
                       const f1p_stmpc_cfg* cfg, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status, double* u,
                       double* x, double* obj, double* duals, int32_t* iters) {
    QpIo io;
    io.x0 = x0; io.ref = ref; io.pa = oa_prev; io.pd = od_v_prev;
    io.steer = steer; io.speed = speed; io.status = status; io.u = u; io.x = x; io.obj = obj; io.duals = duals; io.iters = iters;
    return qp_call<DynQp>(ctx, true, E, cfg, opts, io, nullptr, nullptr);
}

// the ctx's plan warm start for (E, W); a change of shape drops the old contents (every length back to 0 = None)
static int ensure_stqp_warm(f1p_ctx* ctx, int E, int W) {
    bool fresh = false;
    const int rc = warm_ensure(ctx, &ctx->stmpc_qp_warm, sizeof(double) * 2 * (size_t)E * W, E, W, 0, false, &fresh);
    if (fresh) ctx->stmpc_qp_len.assign((size_t)E, 0);
    return rc;
}

// f1p_stmpc_qp_plan_batch (track_id == nullptr: every reference from the raceline) and f1p_stmpc_qp_plan_tracks_batch (track_id [E] host:
// ego e's references from track track_id[e]; an id outside [0, K) joins neither branch, its warm start is neither read nor written)
static int stmpc_qp_plan_impl(f1p_ctx* ctx, const double* x0, const int32_t* track_id, bool tracks, int32_t E, const f1p_stmpc_cfg* dcfg,
                              const f1p_kmpc_cfg* kcfg, double v_ks, double dl, double dlk, const f1p_kmpc_qp_opts* opts, double* steer,
                              double* speed, int32_t* status, int32_t* branch, double* u, double* obj) {
    F1P_ENTER(ctx);
    f1p_kmpc_qp_opts o, ok_;
    int rc = validate_stmpc_qp(ctx, dcfg, E, opts, &o); if (rc) return rc;
    if ((rc = validate_kmpc_qp(ctx, kcfg, E, opts, &ok_))) return rc;
    if (kcfg->horizon > dcfg->horizon) return set_error(ctx, F1P_EINVAL, "stmpc qp plan: TK must be <= T");
    if (E > 0 && (!x0 || !steer || !speed || !status)) return set_error(ctx, F1P_EINVAL, "x0, steer, speed and status are required");
    if (!(dl > 0) || !(dlk > 0)) return set_error(ctx, F1P_EINVAL, "dl and dlk must be > 0");
    if (tracks) {
        if (E > 0 && !track_id) return set_error(ctx, F1P_EINVAL, "track_id is NULL");
        if ((rc = need_tracks(ctx, true, false))) return rc;
    } else if (ctx->n_wp < 2 || !ctx->has_psi) {
        return set_error(ctx, F1P_ESTATE, "waypoints with a heading column are required");
    }
    if (E == 0) return F1P_OK;
    const bool av = ctx->stmpc_qp_av.on != 0, walls = ctx->stmpc_qp_walls.on != 0;
    QpWallArgs wl;
    if (walls && !av) {                                                       // the caps on T and TK hold with walls alone
        if (dcfg->horizon > DynQp::AVOID_MAX_T) return set_error(ctx, F1P_EINVAL, std::string(DynQp::who) + DynQp::avoid_cap);
        if (kcfg->horizon > 31) return set_error(ctx, F1P_EINVAL, "stmpc qp avoid: the kinematic branch's horizon must be <= 31 (2TK + 1 inputs, one lane each)");
    }
    if (walls && (rc = qp_wall_args<DynQp>(ctx, &ctx->stmpc_qp_walls, &wl))) return rc;
    if (av && (rc = qp_avoid_plan_check<DynQp>(ctx, dcfg, E, kcfg))) return rc;
    const double* d_obs_all = av ? ctx->stmpc_obs.cur : nullptr;              // [E][M][5] in the caller's order, or none held
    const int Mo = d_obs_all ? ctx->stmpc_obs.M : 0;
    const int T = dcfg->horizon, TK = kcfg->horizon, W = T;                   // W = max(T, TK)
    if ((rc = ensure_stqp_warm(ctx, E, W))) return rc;
    double* d_warm = ctx->stmpc_qp_warm.as<double>();
    // the branch split (:168) and the reset rules (:1005, :1052), on the host
    BranchSplit sp(ctx, x0, tracks ? track_id : nullptr, E, v_ks, dcfg, dl, kcfg, dlk);
    std::vector<int32_t> use[2];
    for (int b = 0; b < 2; ++b)
        for (const int e : sp.idx[b]) { const int len = ctx->stmpc_qp_len[e]; use[b].push_back(b ? (len >= T) : (len > 0 && len <= TK)); }
    const size_t nd = sp.idx[1].size(), nk = sp.idx[0].size();
    const size_t need = sp.arena_bytes() + 2 * al256(8 * 2 * T * nd) + 2 * al256(8 * 2 * TK * nk) + al256(4 * nd) + al256(4 * nk) +
                        3 * al256(8 * (size_t)E) + al256(4 * (size_t)E) + al256(8 * 5 * (size_t)Mo * nd) + al256(8 * 5 * (size_t)Mo * nk);
    if ((rc = arena_reset(ctx, need))) return rc;
    std::vector<double> hs(E), hv(E), ho(E), hw[2];
    std::vector<int32_t> hst(E);
    StreamDrain io{ctx};                                                      // behind every vector the stream reads or writes: sp's, use, the results
    double* d_steer = (double*)arena_take(ctx, 8 * (size_t)E);
    double* d_speed = (double*)arena_take(ctx, 8 * (size_t)E);
    double* d_obj = (double*)arena_take(ctx, 8 * (size_t)E);
    int32_t* d_st = (int32_t*)arena_take(ctx, 4 * (size_t)E);
    double* d_wout[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; ++b) {
        const int nb = (int)sp.idx[b].size(), Tb = b ? T : TK;
        if (nb == 0) continue;
        int32_t* d_use = (int32_t*)arena_take(ctx, 4 * (size_t)nb);
        double* d_win = (double*)arena_take(ctx, 8 * 2 * (size_t)Tb * nb);
        d_wout[b] = (double*)arena_take(ctx, 8 * 2 * (size_t)Tb * nb);
        if ((rc = sp.prepare(b, io))) return rc;
        if ((rc = io.copy(d_use, use[b].data(), 4 * (size_t)nb, hipMemcpyHostToDevice))) return rc;
        if ((rc = launch_stmpc_qp_warm_in(ctx, d_warm, sp.d_idx[b], d_use, nb, Tb, W, d_win))) return rc;
        // this branch's egos are written contiguously from offset 0 of its own slice: kinematic egos after the dynamic ones
        const size_t off = b ? 0 : nd;
        QpIo q;
        q.pa = d_win; q.pd = d_win + 1; q.pstride = 2;
        q.steer = d_steer + off; q.speed = d_speed + off; q.status = d_st + off; q.obj = d_obj + off; q.warm_out = d_wout[b];
        QpAvoidArgs qa(nullptr, Mo, ctx->stmpc_qp_av);
        if (av && Mo) {                                                       // this branch's discs, gathered on the device; each branch its own variant
            double* d_obs = (double*)arena_take(ctx, 8 * 5 * (size_t)Mo * nb);
            if ((rc = launch_stmpc_qp_obs_in(ctx, d_obs_all, sp.d_idx[b], nb, Mo, d_obs))) return rc;
            qa.obs = d_obs;
        }
        if (b) {
            q.x0 = sp.d_x7; q.ref = sp.d_ref7[1];
            rc = launch_stmpc_qp(ctx, nb, dcfg, o.max_iter, o.tol, q, av || walls ? &qa : nullptr, walls ? &wl : nullptr);
        } else {
            q.x0 = sp.d_s4[0]; q.ref = sp.d_ref4;
            rc = launch_kmpc_qp(ctx, nb, kcfg, ok_.max_iter, ok_.tol, q, av || walls ? &qa : nullptr, walls ? &wl : nullptr);
        }
        if (rc) return rc;
        if ((rc = launch_stmpc_qp_warm_out(ctx, d_wout[b], sp.d_idx[b], nb, Tb, W, d_warm))) return rc;
    }
    // results: [dynamic egos | kinematic egos] -> the caller's order
    if ((rc = io.copy(hs.data(), d_steer, 8 * (size_t)E, hipMemcpyDeviceToHost))) return rc;
    if ((rc = io.copy(hv.data(), d_speed, 8 * (size_t)E, hipMemcpyDeviceToHost))) return rc;
    if ((rc = io.copy(ho.data(), d_obj, 8 * (size_t)E, hipMemcpyDeviceToHost))) return rc;
    if ((rc = io.copy(hst.data(), d_st, 4 * (size_t)E, hipMemcpyDeviceToHost))) return rc;
    for (int b = 0; b < 2; ++b) {
        if (!u || sp.idx[b].empty()) continue;
        hw[b].resize(sp.idx[b].size() * 2 * (size_t)(b ? T : TK));
        if ((rc = io.copy(hw[b].data(), d_wout[b], 8 * hw[b].size(), hipMemcpyDeviceToHost))) return rc;
    }
    if ((rc = io.finish())) return rc;
    const double NaN = nan("");
    for (int b = 0; b < 2; ++b) {
        const size_t off = b ? 0 : nd;
        for (size_t k = 0; k < sp.idx[b].size(); ++k) {
            const int e = sp.idx[b][k];
            const int st = hst[off + k];
            steer[e] = hs[off + k]; speed[e] = hv[off + k]; status[e] = st;
            if (branch) branch[e] = b;
            if (obj) obj[e] = ho[off + k];
            const bool ok = st == 0 || st == 2;
            ctx->stmpc_qp_len[e] = ok ? (int32_t)(b ? T : TK) : 0;            // statuses 1, 3: the reference's None
            if (u) sp.scatter_row(b, k, hw[b].data(), ok, u);
        }
    }
    for (const int e : sp.bad) {                                              // a bad track id: its warm start and length stay as they were
        steer[e] = NaN; speed[e] = NaN; status[e] = F1P_ST_BAD_TRACK;
        if (branch) branch[e] = -1;
        if (obj) obj[e] = NaN;
        if (u) std::fill(u + (size_t)e * W * 2, u + (size_t)(e + 1) * W * 2, NaN);
    }
    return F1P_OK;
}

int f1p_stmpc_qp_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_stmpc_cfg* dcfg, const f1p_kmpc_cfg* kcfg, double v_ks,
                            double dl, double dlk, const f1p_kmpc_qp_opts* opts, double* steer, double* speed, int32_t* status,
                            int32_t* branch, double* u, double* obj) {
    return stmpc_qp_plan_impl(ctx, x0, nullptr, false, E, dcfg, kcfg, v_ks, dl, dlk, opts, steer, speed, status, branch, u, obj);
}

int f1p_stmpc_qp_plan_tracks_batch(f1p_ctx* ctx, const double* x0, const int32_t* track_id, int32_t E, const f1p_stmpc_cfg* dcfg,
                                   const f1p_kmpc_cfg* kcfg, double v_ks, double dl, double dlk, const f1p_kmpc_qp_opts* opts,
                                   double* steer, double* speed, int32_t* status, int32_t* branch, double* u, double* obj) {
    return stmpc_qp_plan_impl(ctx, x0, track_id, true, E, dcfg, kcfg, v_ks, dl, dlk, opts, steer, speed, status, branch, u, obj);
}

int f1p_stmpc_qp_warm_reset(f1p_ctx* ctx) {
    if (!ctx) return F1P_EINVAL;
    std::fill(ctx->stmpc_qp_len.begin(), ctx->stmpc_qp_len.end(), 0);
    return F1P_OK;
}

int f1p_stmpc_qp_warm_get(f1p_ctx* ctx, double* warm, int32_t* len, int32_t E, int32_t W) {
    F1P_ENTER(ctx);
    if (!warm || !len) return set_error(ctx, F1P_EINVAL, "warm / len is NULL");
    if (!ctx->stmpc_qp_warm.is(E, W)) return set_error(ctx, F1P_ESTATE, "no stmpc qp warm start of this shape is held");
    const int rc = warm_download(ctx, &ctx->stmpc_qp_warm, warm, sizeof(double) * 2 * (size_t)E * W); if (rc) return rc;
    memcpy(len, ctx->stmpc_qp_len.data(), sizeof(int32_t) * (size_t)E);
    return F1P_OK;
}

int f1p_stmpc_qp_warm_set(f1p_ctx* ctx, const double* warm, const int32_t* len, int32_t E, int32_t W) {
    F1P_ENTER(ctx);
    if (!warm || !len || E < 1 || W < 1) return set_error(ctx, F1P_EINVAL, "bad warm / len / E / W");
    for (int e = 0; e < E; ++e)
        if (len[e] < 0 || len[e] > W) return set_error(ctx, F1P_EINVAL, "len must be in [0, W]");
    int rc = ensure_stqp_warm(ctx, E, W); if (rc) return rc;
    if ((rc = warm_upload(ctx, &ctx->stmpc_qp_warm, warm, sizeof(double) * 2 * (size_t)E * W))) return rc;
    memcpy(ctx->stmpc_qp_len.data(), len, sizeof(int32_t) * (size_t)E);
    return F1P_OK;
}

// ---------------------------------------------------------------------------------------------------
// the dynamic MPC's shooting solver with in-kernel control generation and a per-ego warm start on the device
// ---------------------------------------------------------------------------------------------------
static int validate_st_sampler(f1p_ctx* ctx, const f1p_stmpc_sampler* smp) {
    if (!smp) return set_error(ctx, F1P_EINVAL, "sampler is NULL");
    const double sg[3] = {smp->sigma_steer_v, smp->sigma_accel, smp->sigma_steer};
    for (const double v : sg)
        if (!(v >= 0.0) || !isfinite(v)) return set_error(ctx, F1P_EINVAL, "sampler sigmas must be finite and >= 0");
    if (smp->ego_offset < 0) return set_error(ctx, F1P_EINVAL, "sampler ego_offset must be >= 0");
    return F1P_OK;
}

// the ctx's warm start for (E, T, TK): E + 1 rows of max(T, TK) x 2 floats -- the last row stays zero (the row every ego reads when a
// call generates without a warm start and must not write one).  A change of shape drops the old contents.
static int ensure_st_warm(f1p_ctx* ctx, int E, int T, int TK) {
    bool fresh = false;
    const int rc = warm_ensure(ctx, &ctx->stmpc_warm, sizeof(float) * 2 * (size_t)(T > TK ? T : TK) * ((size_t)E + 1), E, T, TK, true, &fresh);
    if (fresh) ctx->stmpc_warm_tag.assign((size_t)E, 0);
    return rc;
}

// the buffer of a dynamic-only call: whatever TK the ctx's plans use, as long as E and T are the call's
static int ensure_st_warm_dyn(f1p_ctx* ctx, int E, int T) {
    const WarmBuf& w = ctx->stmpc_warm;
    if (w.d && w.key[0] == E && w.key[1] == T && w.key[2] <= T) return F1P_OK;
    return ensure_st_warm(ctx, E, T, 0);
}

// floats per row of the buffer held: 2 max(T, TK)
static int st_warm_stride(const f1p_ctx* ctx) { return 2 * std::max(ctx->stmpc_warm.key[1], ctx->stmpc_warm.key[2]); }

int f1p_stmpc_gen_controls_dev(f1p_ctx* ctx, float* d_controls, int32_t E, const f1p_stmpc_cfg* cfg, const f1p_stmpc_sampler* smp) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = validate_st_sampler(ctx, smp))) return rc;
    if (E == 0) return F1P_OK;
    if (!d_controls) return set_error(ctx, F1P_EINVAL, "controls is NULL");
    const int T = cfg->horizon;
    if ((rc = ensure_st_warm_dyn(ctx, E, T))) return rc;
    const int ws = st_warm_stride(ctx);
    float* d_warm = ctx->stmpc_warm.as<float>();
    bool all = smp->use_warm != 0, none = !smp->use_warm;
    for (int e = 0; e < E && smp->use_warm; ++e) { if (ctx->stmpc_warm_tag[e] != 2) all = false; else none = false; }
    float* zero_row = d_warm + (size_t)E * ws;
    if (all) return launch_stmpc_gen_controls(ctx, d_controls, E, cfg, smp, d_warm, ws);
    if (none) return launch_stmpc_gen_controls(ctx, d_controls, E, cfg, smp, zero_row, 0);
    // some egos hold a dynamic warm start, the others start from zeros: ego by ego (a mixed state only a plan_batch leaves behind)
    f1p_stmpc_sampler s1 = *smp;
    for (int e = 0; e < E; ++e) {
        s1.ego_offset = smp->ego_offset + e;
        float* row = ctx->stmpc_warm_tag[e] == 2 ? d_warm + (size_t)e * ws : zero_row;
        if ((rc = launch_stmpc_gen_controls(ctx, d_controls + (size_t)e * T * 2 * cfg->n_rollouts, 1, cfg, &s1, row, 0))) return rc;
    }
    return F1P_OK;
}

int f1p_stmpc_plan_dev(f1p_ctx* ctx, const double* d_x0, const double* d_ref, int32_t E, const f1p_stmpc_cfg* cfg,
                       const f1p_stmpc_sampler* smp, double* d_steer, double* d_speed, int32_t* d_best_idx, double* d_best_cost,
                       double* d_best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, cfg, E); if (rc) return rc;
    if ((rc = validate_st_sampler(ctx, smp))) return rc;
    if ((rc = stmpc_collision_check(ctx, false, E))) return rc;
    if (E == 0) return F1P_OK;
    if (!d_x0 || !d_ref || !d_steer || !d_speed || !d_best_idx) return set_error(ctx, F1P_EINVAL, "x0, ref, steer, speed and best_idx are required");
    if ((rc = ensure_st_warm_dyn(ctx, E, cfg->horizon))) return rc;
    const size_t ws = (size_t)st_warm_stride(ctx);
    float* d_warm = ctx->stmpc_warm.as<float>();
    // the egos that start over: all of them (one memset), or the few a plan_batch left in the other branch
    size_t n_restart = 0;
    for (int e = 0; e < E; ++e) n_restart += !smp->use_warm || ctx->stmpc_warm_tag[e] != 2;
    if (n_restart == (size_t)E) {
        F1P_HIP(ctx, hipMemsetAsync(d_warm, 0, sizeof(float) * ws * (size_t)E, ctx->stream));
    } else if (n_restart) {
        for (int e = 0; e < E; ++e)
            if (ctx->stmpc_warm_tag[e] != 2) F1P_HIP(ctx, hipMemsetAsync(d_warm + (size_t)e * ws, 0, sizeof(float) * ws, ctx->stream));
    }
    std::fill(ctx->stmpc_warm_tag.begin(), ctx->stmpc_warm_tag.end(), 0);    // (a failed launch leaves no half-written warm start behind as valid)
    rc = launch_stmpc_plan_gen(ctx, d_x0, d_ref, E, cfg, smp, d_warm, (int)ws, nullptr, d_steer, d_speed, d_best_idx, d_best_cost, d_best_seq);
    if (rc == F1P_OK) std::fill(ctx->stmpc_warm_tag.begin(), ctx->stmpc_warm_tag.end(), 2);
    else (void)hipMemsetAsync(d_warm, 0, sizeof(float) * ws * (size_t)E, ctx->stream);
    return rc;
}

int f1p_stmpc_plan_batch(f1p_ctx* ctx, const double* x0, int32_t E, const f1p_stmpc_cfg* dcfg, const f1p_kmpc_cfg* kcfg, double v_ks,
                         double dl, double dlk, const f1p_stmpc_sampler* smp, double* steer, double* speed, int32_t* best_idx,
                         double* best_cost, int32_t* branch, double* best_seq) {
    F1P_ENTER(ctx);
    int rc = validate_stmpc(ctx, dcfg, E); if (rc) return rc;
    if ((rc = validate_kmpc(ctx, kcfg, E))) return rc;
    if ((rc = validate_st_sampler(ctx, smp))) return rc;
    if ((rc = stmpc_collision_check(ctx, true, E))) return rc;
    if (kcfg->n_rollouts > 8192) return set_error(ctx, F1P_EINVAL, "at most 8192 rollouts per kinematic plan");
    if (E > 0 && (!x0 || !steer || !speed || !best_idx)) return set_error(ctx, F1P_EINVAL, "x0, steer, speed and best_idx are required");
    if (!(dl > 0) || !(dlk > 0)) return set_error(ctx, F1P_EINVAL, "dl and dlk must be > 0");
    if (ctx->n_wp < 2 || !ctx->has_psi) return set_error(ctx, F1P_ESTATE, "waypoints with a heading column are required");
    if (E == 0) return F1P_OK;
    const int T = dcfg->horizon, TK = kcfg->horizon, W = T > TK ? T : TK;
    if ((rc = ensure_st_warm(ctx, E, T, TK))) return rc;
    float* d_warm = ctx->stmpc_warm.as<float>();
    // the model switch (:168) and the restart rule, on the host
    BranchSplit sp(ctx, x0, nullptr, E, v_ks, dcfg, dl, kcfg, dlk);
    std::vector<int32_t> restart;
    for (int b = 0; b < 2; ++b)
        for (const int e : sp.idx[b])
            if (!smp->use_warm || ctx->stmpc_warm_tag[e] != (b ? 2 : 1)) restart.push_back(e);   // (k_stmpc_warm_zero takes the rows in any order)
    std::fill(ctx->stmpc_warm_tag.begin(), ctx->stmpc_warm_tag.end(), 0);    // until the plan is known to have been issued
    const size_t nr = restart.size();
    size_t need = sp.arena_bytes() + al256(4 * nr);
    for (int b = 0; b < 2; ++b) {
        const size_t nb = sp.idx[b].size(), Tb = b ? T : TK;
        need += 3 * al256(8 * nb) + al256(4 * nb) + al256(8 * 2 * Tb * nb);
    }
    if ((rc = arena_reset(ctx, need))) return rc;
    std::vector<double> hs[2], hv[2], hc[2], hq[2];
    std::vector<int32_t> hi[2];
    StreamDrain io{ctx};                                                      // behind every vector the stream reads or writes: sp's, restart, the results
    if (nr) {
        int32_t* d_rows = (int32_t*)arena_take(ctx, 4 * nr);
        if ((rc = io.copy(d_rows, restart.data(), 4 * nr, hipMemcpyHostToDevice))) return rc;
        if ((rc = launch_stmpc_warm_zero(ctx, d_warm, d_rows, (int)nr, 2 * W))) return rc;
    }
    double *d_steer[2], *d_speed[2], *d_bc[2], *d_bs[2];
    int32_t* d_bi[2];
    f1p_kmpc_sampler ks;
    ks.seed = smp->seed; ks.call = smp->call; ks.use_warm = 1; ks.sigma_accel = smp->sigma_accel; ks.sigma_steer = smp->sigma_steer;
    for (int b = 0; b < 2; ++b) {
        const size_t nb = sp.idx[b].size(), Tb = b ? T : TK;
        if (nb == 0) continue;
        d_steer[b] = (double*)arena_take(ctx, 8 * nb); d_speed[b] = (double*)arena_take(ctx, 8 * nb); d_bc[b] = (double*)arena_take(ctx, 8 * nb);
        d_bi[b] = (int32_t*)arena_take(ctx, 4 * nb);
        d_bs[b] = (double*)arena_take(ctx, 8 * 2 * Tb * nb);
        if ((rc = sp.prepare(b, io))) return rc;
        if (b) rc = launch_stmpc_plan_gen(ctx, sp.d_x7, sp.d_ref7[1], (int)nb, dcfg, smp, d_warm, 2 * W, sp.d_idx[1], d_steer[b], d_speed[b], d_bi[b],
                                          d_bc[b], d_bs[b]);
        else rc = launch_kmpc_plan_gen(ctx, sp.d_s4[0], sp.d_ref4, (int)nb, kcfg, &ks, d_warm, d_warm, d_steer[b], d_speed[b], d_bi[b],
                                       d_bc[b], d_bs[b], sp.d_idx[0], 2 * W, (uint32_t)smp->ego_offset);
        if (rc) return rc;
    }
    // results: each branch's compact arrays -> the caller's order
    for (int b = 0; b < 2; ++b) {
        const size_t nb = sp.idx[b].size(), Tb = b ? T : TK;
        if (nb == 0) continue;
        hs[b].resize(nb); hv[b].resize(nb); hc[b].resize(nb); hi[b].resize(nb);
        if ((rc = io.copy(hs[b].data(), d_steer[b], 8 * nb, hipMemcpyDeviceToHost))) return rc;
        if ((rc = io.copy(hv[b].data(), d_speed[b], 8 * nb, hipMemcpyDeviceToHost))) return rc;
        if ((rc = io.copy(hi[b].data(), d_bi[b], 4 * nb, hipMemcpyDeviceToHost))) return rc;
        if (best_cost && (rc = io.copy(hc[b].data(), d_bc[b], 8 * nb, hipMemcpyDeviceToHost))) return rc;
        if (best_seq) { hq[b].resize(nb * 2 * Tb); if ((rc = io.copy(hq[b].data(), d_bs[b], 8 * 2 * Tb * nb, hipMemcpyDeviceToHost))) return rc; }
    }
    if ((rc = io.finish())) return rc;
    for (int b = 0; b < 2; ++b)
        for (size_t k = 0; k < sp.idx[b].size(); ++k) {
            const int e = sp.idx[b][k];
            steer[e] = hs[b][k]; speed[e] = hv[b][k]; best_idx[e] = hi[b][k];
            if (best_cost) best_cost[e] = hc[b][k];
            if (branch) branch[e] = b;
            ctx->stmpc_warm_tag[e] = b ? 2 : 1;
            if (best_seq) sp.scatter_row(b, k, hq[b].data(), true, best_seq);
        }
    return F1P_OK;
}

int f1p_stmpc_warm_reset(f1p_ctx* ctx) {
    if (!ctx) return F1P_EINVAL;
    std::fill(ctx->stmpc_warm_tag.begin(), ctx->stmpc_warm_tag.end(), 0);    // (a row whose tag is not its branch's is zeroed by the plan that reads it)
    ctx->stmpc_warm_nonfinite = false;
    return F1P_OK;
}

int f1p_stmpc_warm_get(f1p_ctx* ctx, float* warm, int32_t* tag, int32_t E, int32_t T, int32_t TK) {
    F1P_ENTER(ctx);
    if (!warm || !tag) return set_error(ctx, F1P_EINVAL, "warm / tag is NULL");
    if (!ctx->stmpc_warm.is(E, T, TK)) return set_error(ctx, F1P_ESTATE, "no stmpc warm start of this shape is held");
    const int rc = warm_download(ctx, &ctx->stmpc_warm, warm, sizeof(float) * 2 * (size_t)E * (T > TK ? T : TK)); if (rc) return rc;
    memcpy(tag, ctx->stmpc_warm_tag.data(), sizeof(int32_t) * (size_t)E);
    return F1P_OK;
}

int f1p_stmpc_warm_set(f1p_ctx* ctx, const float* warm, const int32_t* tag, int32_t E, int32_t T, int32_t TK) {
    F1P_ENTER(ctx);
    if (!warm || !tag || E < 1 || T < 1 || TK < 0) return set_error(ctx, F1P_EINVAL, "bad warm / tag / E / T / TK");
    for (int e = 0; e < E; ++e)
        if (tag[e] < 0 || tag[e] > 2) return set_error(ctx, F1P_EINVAL, "tag must be 0, 1 or 2");
    int rc = ensure_st_warm(ctx, E, T, TK); if (rc) return rc;
    if ((rc = warm_upload(ctx, &ctx->stmpc_warm, warm, sizeof(float) * 2 * (size_t)E * (T > TK ? T : TK)))) return rc;
    memcpy(ctx->stmpc_warm_tag.data(), tag, sizeof(int32_t) * (size_t)E);
    // the only way a non-finite value enters a warm start (the kernels write clamped controls, or a NaN they were handed here)
    ctx->stmpc_warm_nonfinite = false;
    for (size_t q = 0; q < 2 * (size_t)E * (T > TK ? T : TK); ++q) if (!isfinite(warm[q])) { ctx->stmpc_warm_nonfinite = true; break; }
    return F1P_OK;
}
