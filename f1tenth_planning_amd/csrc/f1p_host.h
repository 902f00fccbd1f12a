// f1p_host.h -- what the host-side translation units of libf1p.so (f1p_core / scene / trackers / lattice / kmpc / stmpc / comm .hip) share
// beyond f1p_internal.h: the entry macro, the staging plan of the *_batch wrappers (Stage), the look-up of page-locked caller arrays, the guard of
// frames that copy asynchronously from their own vectors (StreamDrain), and the checks used by more than one unit.  Host only: no k_*.hip
// includes it.  What it declares lives in namespace f1p and stays hidden (-fvisibility=hidden).
#pragma once

#include <math.h>
#include <string.h>

#include <algorithm>

#include <new>
#include <string>
#include <vector>

// The exported surface is what include/f1p.h declares: its declarations (extern "C") are made with default visibility HERE, before anything else
// includes it, and the definitions in the units inherit both.  Whatever else a unit defines stays hidden (-fvisibility=hidden).
#pragma GCC visibility push(default)
#include "../../include/f1p.h"
#pragma GCC visibility pop
#include "f1p_internal.h"

#define F1P_ENTER(ctx)                                              \
    if (!(ctx)) return F1P_EINVAL;                                  \
    F1P_HIP((ctx), hipSetDevice((ctx)->device))

namespace f1p {

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

#define F1P_SMALL_D2H_BYTES ((size_t)64 * 1024)      // calls up to this size: outputs written by the kernels straight into the page-locked block
#define F1P_BOUNCE_BYTES ((size_t)1024 * 1024)       // the block; results up to this size come back in ONE copy + a host-side scatter
int ensure_bounce(f1p_ctx* ctx);                     // f1p_core.hip

// staged host<->device transfer plan for the *_batch wrappers
struct Stage {
    f1p_ctx* ctx;
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<Out> outs;
    size_t total = 0, out_total = 0;
    // Small calls (a single vehicle, a few hundred egos): the outputs -- and inputs of a few hundred bytes, i.e. a pose or two --
    // live in the context's page-locked, device-visible block: the kernels write their results straight into host memory and no
    // hipMemcpy is issued at all (each one is ~10-15 us of latency; a single-vehicle plan() is otherwise mostly copies).
    // Larger inputs still go through a copy: a kernel that re-reads them (previous headings, controls) must find them in HBM.
    bool zc = false;
    size_t zc_used = 0;
    explicit Stage(f1p_ctx* c) : ctx(c) {}
    void need(size_t bytes, bool used = true) { if (used) total += al256(bytes); }
    int begin() {
        zc = total <= F1P_SMALL_D2H_BYTES && ensure_bounce(ctx) == F1P_OK;
        zc_used = 0;
        return arena_reset(ctx, total);
    }
    void* zc_take(size_t bytes) { void* p = ctx->h_bounce + zc_used; zc_used += al256(bytes); return p; }
    template <typename T> int in(const T* host, size_t count, const T** dev) {
        *dev = nullptr;
        if (!host || count == 0) return F1P_OK;
        if (zc && count * sizeof(T) <= 512) {
            T* d = (T*)zc_take(count * sizeof(T));
            memcpy(d, host, count * sizeof(T));
            *dev = d;
            return F1P_OK;
        }
        T* d = (T*)arena_take(ctx, count * sizeof(T));
        F1P_HIP(ctx, hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        *dev = d;
        return F1P_OK;
    }
    template <typename T> T* out(T* host, size_t count) {
        if (!host || count == 0) return nullptr;
        T* d = zc ? (T*)zc_take(count * sizeof(T)) : (T*)arena_take(ctx, count * sizeof(T));
        outs.push_back({(void*)host, (void*)d, count * sizeof(T)});
        return d;
    }
    int finish() {
        if (zc) {
            auto in_block = [&](const void* p) { return (const char*)p >= ctx->h_bounce && (const char*)p < ctx->h_bounce + F1P_BOUNCE_BYTES; };
            for (auto& o : outs)                                  // an in/out buffer that went through the device arena (larger than a pose)
                if (!in_block(o.dev)) F1P_HIP(ctx, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
            F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (auto& o : outs) if (in_block(o.dev)) memcpy(o.host, o.dev, o.bytes);
            return F1P_OK;
        }
        return gather(nullptr);
    }
    // Results to the host: arrays that sit back to back in the arena and together fit the page-locked block come back in ONE copy
    // and are scattered on the host (a hipMemcpyAsync per array is ~10 us of submission each -- six of them were a third of a
    // 4096-ego plan()'s latency); anything else (the trajectories) is copied on its own.  `skip`: an output the caller copies itself.
    int gather(const void* skip) {
        std::vector<Out*> small;
        const char *lo = nullptr, *hi = nullptr;
        for (auto& o : outs) {
            if (o.host == skip) continue;
            const char* b = (const char*)o.dev;
            const char* nlo = lo && lo < b ? lo : b;
            const char* nhi = hi && hi > b + o.bytes ? hi : b + o.bytes;
            if ((size_t)(nhi - nlo) <= F1P_BOUNCE_BYTES && o.bytes <= F1P_BOUNCE_BYTES / 4) { small.push_back(&o); lo = nlo; hi = nhi; }
            else F1P_HIP(ctx, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (small.size() > 1 && ensure_bounce(ctx) == F1P_OK) {
            F1P_HIP(ctx, hipMemcpyAsync(ctx->h_bounce, lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, ctx->stream));
            F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (Out* o : small) memcpy(o->host, ctx->h_bounce + ((const char*)o->dev - lo), o->bytes);
            return F1P_OK;
        }
        for (Out* o : small) F1P_HIP(ctx, hipMemcpyAsync(o->host, o->dev, o->bytes, hipMemcpyDeviceToHost, ctx->stream));
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return F1P_OK;
    }
};

// The device-side address of [p, p + bytes) when the WHOLE range lies in page-locked host memory this device can address (hipHostMalloc /
// hipHostRegister), else null.  A kernel that stores through it writes straight into the caller's array; a range that is only partly
// registered would fault, so both ends must be known to HIP as host memory with ONE linear device mapping between them (the
// first byte alone had been checked, and the host address used instead of attr.devicePointer).
void* pinned_device_ptr(const void* p, size_t bytes);
// ... with the context's own page-locked blocks answered from its table (no runtime call)
void* pinned_device_ptr(const f1p_ctx* ctx, const void* p, size_t bytes);

// A frame whose own host vectors are the source or the destination of asynchronous copies: every way out of it drains the stream first.
// Declared before the first such copy; the copies go through copy(), the success path ends in finish() (the frame's ONE synchronisation).
struct StreamDrain {
    f1p_ctx* ctx;
    bool armed = true;
    ~StreamDrain() { if (armed) (void)hipStreamSynchronize(ctx->stream); }
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (bytes) F1P_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
        return F1P_OK;
    }
    int finish() { armed = false; F1P_HIP(ctx, hipStreamSynchronize(ctx->stream)); return F1P_OK; }
};

// checks shared by several units
int need_tracks(f1p_ctx* ctx, bool psi, bool kappa);                                        // f1p_scene.hip: a track set (with these columns) is loaded
// the checks both shooting configurations share (f1p_kmpc_cfg, f1p_stmpc_cfg)
template <typename CFG> int validate_shoot_cfg(f1p_ctx* ctx, const CFG* cfg, int E) {
    if (!cfg) return set_error(ctx, F1P_EINVAL, "cfg is NULL");
    if (E < 0) return set_error(ctx, F1P_EINVAL, "E must be >= 0");
    if (cfg->horizon < 1 || cfg->horizon > 4096) return set_error(ctx, F1P_EINVAL, "horizon must be in [1, 4096]");
    if (cfg->n_rollouts < 1) return set_error(ctx, F1P_EINVAL, "n_rollouts must be >= 1");
    if (!(cfg->dt > 0) || !(cfg->wheelbase > 0)) return set_error(ctx, F1P_EINVAL, "dt and wheelbase must be > 0");
    return F1P_OK;
}
inline int validate_kmpc(f1p_ctx* ctx, const f1p_kmpc_cfg* cfg, int E) { return validate_shoot_cfg(ctx, cfg, E); }
inline int validate_stmpc(f1p_ctx* ctx, const f1p_stmpc_cfg* cfg, int E) { return validate_shoot_cfg(ctx, cfg, E); }
// f1p_kmpc.hip: the QP's cfg checks, and opts (nullable: the defaults) into *o, range-checked
int validate_kmpc_qp(f1p_ctx* ctx, const f1p_kmpc_cfg* cfg, int E, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o);
int qp_opts(f1p_ctx* ctx, const f1p_kmpc_qp_opts* opts, f1p_kmpc_qp_opts* o, const char* what);
int validate_qp_avoid(f1p_ctx* ctx, const f1p_kmpc_qp_avoid* a);
// f1p_kmpc.hip: f1p_{kmpc,stmpc}_qp_set_avoid on the planner's own switch `state`
int qp_set_avoid(f1p_ctx* ctx, f1p_kmpc_qp_avoid* state, const f1p_kmpc_qp_avoid* avoid);

// The stateless QP entry points f1p_{kmpc,stmpc}_qp[_avoid]_{batch,dev} are one body (qp_call) over a model Q: KinQp (f1p_kmpc.hip) or DynQp
// (f1p_stmpc.hip), each with
//   Cfg; NX (the state width), DUALS (rows per step: duals [E][DUALS T - 2]), AVOID_MAX_T (the avoidance variant's longest horizon)
//   who ("kmpc" / "stmpc": the prefix of the messages), avoid_cap (the message past AVOID_MAX_T)
//   EMPTY_RETURNS (the *_batch entries return F1P_OK at E == 0 before they stage)
//   validate(ctx, cfg, E, opts, o), launch(ctx, E, cfg, max_iter, tol, io, avoid, walls)
//   obs(ctx), av(ctx): the planner's discs and its set_avoid switch
// set_avoid is on: what the entry points check before they launch the avoidance variant on the context's discs, held in the order of the
// caller's E egos (kcfg: a plan's kinematic branch, which runs k_kmpc_qp's variant)
template <class Q>
int qp_avoid_plan_check(f1p_ctx* ctx, const typename Q::Cfg* cfg, int E, const f1p_kmpc_cfg* kcfg = nullptr) {
    const std::string w = Q::who;
    if (cfg->horizon > Q::AVOID_MAX_T) return set_error(ctx, F1P_EINVAL, w + Q::avoid_cap);
    if (kcfg && kcfg->horizon > 31) return set_error(ctx, F1P_EINVAL, w + " qp avoid: the kinematic branch's horizon must be <= 31 (2TK + 1 inputs, one lane each)");
    const ObsState& st = Q::obs(ctx);
    if (st.cur && E != st.E)
        return set_error(ctx, F1P_ESTATE, w + " obstacles were set for " + std::to_string(st.E) + " egos, this plan has " + std::to_string(E) + " (f1p_" + w + "_set_obstacles)");
    return F1P_OK;
}

// io: the caller's arrays, on the host (staged: *_batch) or on the device (*_dev).  avoid null: the plain QP -- which a *_dev call runs as
// the avoidance variant on the context's discs while set_avoid is on.  Else avoid holds the call's obs, M and outputs, and `numbers`
// (nullable: the defaults) its margin, rho and lin.  walls (with avoid): the wall variant (f1p_{kmpc,stmpc}_qp_walls_*), whose obs may
// be null with M = 0.
template <class Q>
int qp_call(f1p_ctx* ctx, bool staged, int E, const typename Q::Cfg* cfg, const f1p_kmpc_qp_opts* opts, const QpIo& io, const QpAvoidArgs* avoid,
            const f1p_kmpc_qp_avoid* numbers, const QpWallArgs* walls = nullptr) {
    F1P_ENTER(ctx);
    const std::string w = Q::who;
    f1p_kmpc_qp_opts o;
    QpAvoidArgs av;
    int rc = Q::validate(ctx, cfg, E, opts, &o); if (rc) return rc;
    if (avoid) {
        if (cfg->horizon > Q::AVOID_MAX_T) return set_error(ctx, F1P_EINVAL, w + Q::avoid_cap);
        if (walls) {
            if (avoid->M < 0 || avoid->M > F1P_KMPC_MAX_OBS) return set_error(ctx, F1P_EINVAL, w + " qp walls: M must be in [0, 16]");
            if (E > 0 && avoid->M > 0 && !avoid->obs) return set_error(ctx, F1P_EINVAL, w + " qp walls: obs is NULL with M > 0");
        } else {
            if (avoid->M < 1 || avoid->M > F1P_KMPC_MAX_OBS) return set_error(ctx, F1P_EINVAL, w + " qp avoid: M must be in [1, 16]");
            if (E > 0 && !avoid->obs) return set_error(ctx, F1P_EINVAL, w + " qp avoid: obs is NULL");
        }
        f1p_kmpc_qp_avoid a;
        f1p_kmpc_qp_avoid_default(&a);
        if (numbers) a = *numbers;
        if ((rc = validate_qp_avoid(ctx, &a))) return rc;
        av = *avoid;
        av.margin = a.margin; av.rho = a.rho; av.lin = a.lin;
    }
    if (E > 0 && (!io.x0 || !io.ref || !io.steer || !io.speed || !io.status)) return set_error(ctx, F1P_EINVAL, "x0, ref, steer, speed and status are required");
    if (!staged) {
        if (!avoid && Q::av(ctx).on) {
            if ((rc = qp_avoid_plan_check<Q>(ctx, cfg, E))) return rc;
            av = QpAvoidArgs(Q::obs(ctx).cur, Q::obs(ctx).M, Q::av(ctx));
            avoid = &av;
        }
        return Q::launch(ctx, E, cfg, o.max_iter, o.tol, io, avoid ? &av : nullptr, walls);
    }
    if (Q::EMPTY_RETURNS && E == 0) return F1P_OK;
    const size_t T = cfg->horizon, e = E, m = av.M, NX = Q::NX, ND = Q::DUALS * T - 2;
    Stage s(ctx);
    s.need(8 * NX * e); s.need(8 * e * NX * (T + 1)); s.need(8 * e * T, io.pa); s.need(8 * e * T, io.pd); s.need(8 * e * m * 5, avoid);
    s.need(8 * e); s.need(8 * e); s.need(4 * e); s.need(8 * e * T * 2, io.u); s.need(8 * e * NX * (T + 1), io.x); s.need(8 * e, io.obj);
    s.need(8 * e * ND, io.duals); s.need(4 * e, io.iters);
    s.need(8 * e, av.eps); s.need(8 * e * T * 8, av.planes); s.need(8 * e * (2 * T + 1), av.duals);
    if ((rc = s.begin())) return rc;
    QpIo d;
    if ((rc = s.in(io.x0, NX * e, &d.x0))) return rc;
    if ((rc = s.in(io.ref, e * NX * (T + 1), &d.ref))) return rc;
    if ((rc = s.in(io.pa, e * T, &d.pa))) return rc;
    if ((rc = s.in(io.pd, e * T, &d.pd))) return rc;
    if ((rc = s.in(av.obs, e * m * 5, &av.obs))) return rc;
    d.steer = s.out(io.steer, e); d.speed = s.out(io.speed, e); d.status = s.out(io.status, e);
    d.u = s.out(io.u, e * T * 2); d.x = s.out(io.x, e * NX * (T + 1)); d.obj = s.out(io.obj, e);
    d.duals = s.out(io.duals, e * ND); d.iters = s.out(io.iters, e);
    av.eps = s.out(av.eps, e); av.planes = s.out(av.planes, e * T * 8); av.duals = s.out(av.duals, e * (2 * T + 1));
    if ((rc = Q::launch(ctx, E, cfg, o.max_iter, o.tol, d, avoid ? &av : nullptr, walls))) return rc;
    return s.finish();
}

// ---- wall rows (k_kmpc_qp.hip / k_stmpc_qp.hip WALL): one body over KinQp / DynQp ------------------------------------
template <class Q>
int validate_qp_walls(f1p_ctx* ctx, const f1p_kmpc_qp_walls* w) {
    if (w->n_samples < 1 || w->n_samples > F1P_KMPC_QP_WALL_MAX_SAMPLES || !isfinite(w->margin))
        return set_error(ctx, F1P_EINVAL, std::string(Q::who) + " qp walls: n_samples must be in [1, 256] and margin finite");
    return F1P_OK;
}

// w (nullable: the defaults), checked, and the context's grid as it is now -> the kernel's arguments
template <class Q>
int qp_wall_args(f1p_ctx* ctx, const f1p_kmpc_qp_walls* w, QpWallArgs* out) {
    const std::string who = Q::who;
    f1p_kmpc_qp_walls d;
    f1p_kmpc_qp_walls_default(&d);
    if (w) d = *w;
    const int rc = validate_qp_walls<Q>(ctx, &d); if (rc) return rc;
    if (!ctx->has_grid) return set_error(ctx, F1P_ESTATE, who + " qp walls are on but no occupancy grid is loaded (f1p_set_grid)");
    if (ctx->n_disc > 0)
        return set_error(ctx, F1P_ESTATE, who + " qp walls are a point / disc test: remove the oriented footprint (f1p_set_footprint) and use f1p_inflate_grid");
    out->g = grid_dev(ctx);
    out->h = 0.5 * ctx->res;
    out->n_samples = d.n_samples;
    out->margin = d.margin;
    return F1P_OK;
}

// f1p_{kmpc,stmpc}_qp_set_walls on the planner's own switch `state`
template <class Q>
int qp_set_walls(f1p_ctx* ctx, f1p_kmpc_qp_walls* state, const f1p_kmpc_qp_walls* walls) {
    F1P_ENTER(ctx);
    if (!walls || !walls->on) { state->on = 0; return F1P_OK; }
    const int rc = validate_qp_walls<Q>(ctx, walls); if (rc) return rc;
    *state = *walls;
    state->on = 1;
    return F1P_OK;
}

// the wall problem of E egos.  av null: the discs the context holds (while the planner's set_avoid is on, else none) with its numbers.
// cfg, opts and the horizon's cap are qp_call's to check.
template <class Q>
int qp_walls_call(f1p_ctx* ctx, bool staged, int E, const typename Q::Cfg* cfg, const f1p_kmpc_qp_opts* opts, const QpIo& io, const QpAvoidArgs* av,
                  const f1p_kmpc_qp_avoid* numbers, const f1p_kmpc_qp_walls* walls) {
    F1P_ENTER(ctx);
    QpWallArgs wl;
    int rc = qp_wall_args<Q>(ctx, walls, &wl); if (rc) return rc;
    QpAvoidArgs held;
    if (!av) {
        const bool on = Q::av(ctx).on;
        if (on && cfg && (rc = qp_avoid_plan_check<Q>(ctx, cfg, E))) return rc;
        held = QpAvoidArgs(on ? Q::obs(ctx).cur : nullptr, on ? Q::obs(ctx).M : 0, Q::av(ctx));
        av = &held; numbers = &Q::av(ctx);
    }
    return qp_call<Q>(ctx, staged, E, cfg, opts, io, av, numbers, &wl);
}

// f1p_kmpc.hip: the argument checks of the four reference extractions (f1p_{kmpc,stmpc}_ref[_tracks]_{batch,dev}), and the *_batch body behind them:
// ncol = 4 (kinematic rows) or 7 (dynamic rows); track_id (host) is read when tracks, else every ego follows the raceline
int validate_ref(f1p_ctx* ctx, const void* states, const int32_t* track_id, bool tracks, int E, int horizon, double dt, double dl, const void* ref);
int ref_batch_impl(f1p_ctx* ctx, int ncol, const double* states, const int32_t* track_id, bool tracks, int32_t E, int32_t horizon, double dt, double dl,
                   double* ref);
// f1p_kmpc.hip: what the two shooting planners' rollout tests share on the host.  who: "kmpc" / "stmpc", the prefix of every message.
// set_obstacles: obs (host or device, by `dev`) -> the discs in force of `st`; null or M == 0 clears.  groups_matter: the planner's tested
// kernels run one workgroup per ego, so f1p_kmpc_set_groups(> 0) refuses the set.
int set_obstacles(f1p_ctx* ctx, ObsState& st, const char* who, bool groups_matter, const double* obs, int32_t E, int32_t M, bool dev);
// the preconditions of the tests of a plan over E egos, checked before anything is launched: the discs of `st` (set for E egos), and -- while
// `on` -- the occupancy test with its n_sub points per step (n_sub_k: the second count of f1p_stmpc_set_collision, F1P_NO_NSUB_K: there is none).
// kinematic: the call may run the kinematic filter (one workgroup per ego with a test)
#define F1P_NO_NSUB_K (-1)
int collision_check(f1p_ctx* ctx, const ObsState& st, bool on, int n_sub, int n_sub_k, const char* who, bool kinematic, int E);

}  // namespace f1p
