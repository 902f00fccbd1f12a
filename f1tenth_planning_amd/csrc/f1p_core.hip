// f1p_core.hip -- the core of libf1p.so's extern "C" surface (include/f1p.h): errors, the device arena, the warm-start buffers, context
// create / destroy, device and page-locked memory, the timer
#include <dlfcn.h>

#include "f1p_host.h"

using namespace f1p;

static thread_local std::string g_create_error;

namespace f1p {

int set_error(f1p_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

int check_hip(f1p_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return F1P_OK;
    const int code = (e == hipErrorOutOfMemory) ? F1P_ENOMEM : F1P_EHIP;
    return set_error(ctx, code, std::string(what) + ": " + hipGetErrorString(e));
}

int arena_reset(f1p_ctx* ctx, size_t need_bytes) {
    ctx->arena_used = 0;
    if (need_bytes <= ctx->arena_bytes) return F1P_OK;
    if (ctx->d_arena) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->d_arena); ctx->d_arena = nullptr; ctx->arena_bytes = 0; }
    size_t want = need_bytes + (need_bytes >> 2) + 4096;
    F1P_HIP(ctx, hipMalloc((void**)&ctx->d_arena, want));
    ctx->arena_bytes = want;
    return F1P_OK;
}

void* arena_take(f1p_ctx* ctx, size_t bytes) {
    void* p = ctx->d_arena + ctx->arena_used;
    ctx->arena_used += al256(bytes);
    return p;
}

GridDev grid_dev(const f1p_ctx* ctx) {
    GridDev g;
    g.bits = ctx->d_bits; g.w = ctx->gw; g.h = ctx->gh; g.wwords = ctx->gwwords;
    g.inv_res = ctx->inv_res; g.ox = ctx->ox; g.oy = ctx->oy;
    return g;
}

int ensure_bounce(f1p_ctx* ctx) {
    if (ctx->h_bounce) return F1P_OK;
    F1P_HIP(ctx, hipHostMalloc((void**)&ctx->h_bounce, F1P_BOUNCE_BYTES, hipHostMallocDefault));
    return F1P_OK;
}

void* pinned_device_ptr(const f1p_ctx* ctx, const void* p, size_t bytes) {
    if (!p || bytes == 0) return nullptr;
    const char* c = (const char*)p;
    if (ctx->h_step && ctx->h_step_dev && c >= ctx->h_step && c + bytes <= ctx->h_step + ctx->step_host_bytes) return ctx->h_step_dev + (c - ctx->h_step);
    for (const auto& b : ctx->host_blocks)
        if (c >= b.base && c + bytes <= b.base + b.bytes) return b.dev + (c - b.base);
    return pinned_device_ptr(p, bytes);
}
void* pinned_device_ptr(const void* p, size_t bytes) {
    if (!p || bytes == 0) return nullptr;
    hipPointerAttribute_t a, b;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // pageable: not known to HIP
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    if (bytes > 1) {
        if (hipPointerGetAttributes(&b, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (b.type != hipMemoryTypeHost || !b.devicePointer) return nullptr;
        if ((const char*)b.devicePointer - (const char*)a.devicePointer != (ptrdiff_t)(bytes - 1)) return nullptr;
        void* base = nullptr; size_t size = 0;                       // one allocation (where the runtime can tell)
        if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)a.devicePointer) == hipSuccess) {
            if ((const char*)a.devicePointer + bytes > (const char*)base + size) return nullptr;
        } else (void)hipGetLastError();
    }
    return a.devicePointer;
}

int warm_ensure(f1p_ctx* ctx, WarmBuf* w, size_t bytes, int a, int b, int c, bool zero, bool* fresh) {
    if (w->is(a, b, c)) return F1P_OK;
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (w->d) (void)hipFree(w->d);
    *w = WarmBuf();
    *fresh = true;
    F1P_HIP(ctx, hipMalloc(&w->d, bytes));
    if (zero) F1P_HIP(ctx, hipMemsetAsync(w->d, 0, bytes, ctx->stream));
    w->bytes = bytes; w->key[0] = a; w->key[1] = b; w->key[2] = c;
    return F1P_OK;
}

int warm_upload(f1p_ctx* ctx, WarmBuf* w, const void* host, size_t bytes) {
    F1P_HIP(ctx, hipMemcpyAsync(w->d, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F1P_OK;
}

int warm_download(f1p_ctx* ctx, const WarmBuf* w, void* host, size_t bytes) {
    F1P_HIP(ctx, hipMemcpyAsync(host, w->d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F1P_OK;
}

}  // namespace f1p

const char* f1p_version(void) { return F1P_VERSION_STRING; }

int f1p_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return F1P_ENODEV; }
    return n;
}

int f1p_create(f1p_ctx** out, int device) {
    if (!out) return set_error(nullptr, F1P_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return set_error(nullptr, F1P_ENODEV, std::string("no HIP device visible (") + hipGetErrorString(e) + "): libf1p.so has no CPU fallback");
    if (device < 0 || device >= n) return set_error(nullptr, F1P_ENODEV, "device index out of range");
    f1p_ctx* ctx = new (std::nothrow) f1p_ctx();
    if (!ctx) return set_error(nullptr, F1P_ENOMEM, "out of host memory");
    ctx->device = device;
    int rc = F1P_OK;
    do {
        if ((e = hipSetDevice(device)) != hipSuccess) { rc = check_hip(nullptr, e, "hipSetDevice"); break; }
        if ((e = hipGetDeviceProperties(&ctx->prop, device)) != hipSuccess) { rc = check_hip(nullptr, e, "hipGetDeviceProperties"); break; }
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) { rc = check_hip(nullptr, e, "hipStreamCreate"); break; }
        if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess) { rc = check_hip(nullptr, e, "hipEventCreate"); break; }
        if ((e = hipEventCreate(&ctx->ev1)) != hipSuccess) { rc = check_hip(nullptr, e, "hipEventCreate"); break; }
    } while (0);
    if (rc != F1P_OK) { f1p_destroy(ctx); return rc; }
    *out = ctx;
    return F1P_OK;
}

void f1p_destroy(f1p_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    f1p_comm_destroy(ctx);
    void* ptrs[] = {ctx->lat_obs.d, ctx->d_lat_pace, ctx->d_lat_obs_xf, ctx->d_wx, ctx->d_wy, ctx->d_wv, ctx->d_wpsi, ctx->d_wkappa, ctx->d_wbox, ctx->d_tx, ctx->d_ty, ctx->d_tv, ctx->d_tpsi, ctx->d_tkappa, ctx->d_tbox, ctx->d_ttab, ctx->d_bits, ctx->d_bits0, ctx->d_bits_clear, ctx->d_bb_scratch, ctx->d_arena, ctx->d_comm_key, ctx->d_comm_idx, ctx->kmpc_warm.d, ctx->kmpc_qp_warm.d, ctx->stmpc_qp_warm.d, ctx->stmpc_warm.d, ctx->d_kmpc_scratch, ctx->d_mix_scratch, ctx->d_split_scratch, ctx->d_rec_scratch, ctx->d_st_scratch, ctx->d_audit, ctx->d_audit_buf, ctx->d_cl_theta[0], ctx->d_cl_theta[1], ctx->d_step, ctx->d_comm_rec, ctx->d_order, ctx->d_kmpc_cfg, ctx->kmpc_obs.d, ctx->stmpc_obs.d, ctx->d_riv_mem, ctx->d_riv_rng, ctx->arc_wp.cum, ctx->arc_wp.ok, ctx->arc_trk.cum, ctx->arc_trk.ok, ctx->arc_wp.tim, ctx->arc_wp.pok, ctx->arc_trk.tim, ctx->arc_trk.pok, ctx->d_riv_tid, ctx->d_riv_rec, ctx->d_riv_idx};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->h_bounce) (void)hipHostFree(ctx->h_bounce);
    if (ctx->h_step) (void)hipHostFree(ctx->h_step);
    if (ctx->h_kmpc_cfg) (void)hipHostFree(ctx->h_kmpc_cfg);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (auto& ev : ctx->ev_chunk) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->ev_prof) if (ev) (void)hipEventDestroy(ev);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (auto& st : ctx->pipe_stream) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (auto& ev : ctx->ev_pipe) if (ev) (void)hipEventDestroy(ev);
    if (ctx->rccl_lib) dlclose(ctx->rccl_lib);
    delete ctx;
}

const char* f1p_last_error(const f1p_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int f1p_device_info(const f1p_ctx* ctx, char* name, size_t name_len, int32_t* compute_units, char* arch, size_t arch_len) {
    if (!ctx) return F1P_EINVAL;
    if (name && name_len) { strncpy(name, ctx->prop.name, name_len - 1); name[name_len - 1] = 0; }
    if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
    if (arch && arch_len) { strncpy(arch, ctx->prop.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    return F1P_OK;
}

int f1p_dev_alloc(f1p_ctx* ctx, void** dptr, size_t bytes) {
    F1P_ENTER(ctx);
    if (!dptr) return set_error(ctx, F1P_EINVAL, "dptr is NULL");
    *dptr = nullptr;
    F1P_HIP(ctx, hipMalloc(dptr, bytes ? bytes : 1));
    return F1P_OK;
}
int f1p_dev_free(f1p_ctx* ctx, void* dptr) {
    F1P_ENTER(ctx);
    if (dptr) F1P_HIP(ctx, hipFree(dptr));
    return F1P_OK;
}
int f1p_host_alloc(f1p_ctx* ctx, void** hptr, size_t bytes) {
    F1P_ENTER(ctx);
    if (!hptr) return set_error(ctx, F1P_EINVAL, "hptr is NULL");
    *hptr = nullptr;
    F1P_HIP(ctx, hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, *hptr, 0) == hipSuccess && dev) ctx->host_blocks.push_back({(char*)*hptr, bytes ? bytes : 1, (char*)dev});
    else (void)hipGetLastError();                                // (not in the table: the per-call checks decide)
    return F1P_OK;
}
int f1p_host_free(f1p_ctx* ctx, void* hptr) {
    F1P_ENTER(ctx);
    if (hptr) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));             // a kernel may still be writing into it (zero-copy outputs).  FIRST: a failed sync returns with the block still tracked
        for (size_t i = 0; i < ctx->host_blocks.size(); ++i)
            if (ctx->host_blocks[i].base == (char*)hptr) { ctx->host_blocks.erase(ctx->host_blocks.begin() + (long)i); break; }
        F1P_HIP(ctx, hipHostFree(hptr));
    }
    return F1P_OK;
}
int f1p_h2d(f1p_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    F1P_ENTER(ctx);
    if (bytes && (!dst_dev || !src_host)) return set_error(ctx, F1P_EINVAL, "NULL pointer");
    if (bytes) F1P_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return F1P_OK;
}
int f1p_d2h(f1p_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
    F1P_ENTER(ctx);
    if (bytes && (!dst_host || !src_dev)) return set_error(ctx, F1P_EINVAL, "NULL pointer");
    if (bytes) F1P_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return F1P_OK;
}
int f1p_memset(f1p_ctx* ctx, void* dst_dev, int value, size_t bytes) {
    F1P_ENTER(ctx);
    if (bytes) F1P_HIP(ctx, hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    return F1P_OK;
}
int f1p_sync(f1p_ctx* ctx) {
    F1P_ENTER(ctx);
    F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F1P_OK;
}
int f1p_timer_begin(f1p_ctx* ctx) {
    F1P_ENTER(ctx);
    F1P_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return F1P_OK;
}
int f1p_timer_end(f1p_ctx* ctx, float* elapsed_ms) {
    F1P_ENTER(ctx);
    F1P_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    F1P_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    F1P_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (elapsed_ms) *elapsed_ms = ms;
    return F1P_OK;
}
