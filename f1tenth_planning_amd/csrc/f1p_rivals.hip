// f1p_rivals.hip -- the rivals entry points of include/f1p.h: the races' member lists on the context, the asynchronous device call and its
// host-array wrapper (kernel: k_rivals.hip)
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
