// f1p_comm.hip -- the RCCL exchange step of the candidate-sharded lattice plan (cross-rank argmin) and its local kernels on host arrays
#include <dlfcn.h>

#include <rccl/rccl.h>

#include "f1p_host.h"

using namespace f1p;

// ---------------------------------------------------------------------------------------------------
// RCCL, loaded with dlopen so libf1p.so itself has no link-time dependency on it.  Types and enum values come
// from <rccl/rccl.h> (ncclUint64, ncclInt32, ncclMin ...); only the entry points are resolved at run time.
// ---------------------------------------------------------------------------------------------------
static_assert(NCCL_UNIQUE_ID_BYTES == F1P_COMM_ID_BYTES, "f1p.h must carry RCCL's unique-id size");
typedef ncclResult_t (*pfn_ncclGetUniqueId)(ncclUniqueId*);
typedef ncclResult_t (*pfn_ncclCommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
typedef ncclResult_t (*pfn_ncclCommDestroy)(ncclComm_t);
typedef ncclResult_t (*pfn_ncclCommCount)(const ncclComm_t, int*);
typedef ncclResult_t (*pfn_ncclCommUserRank)(const ncclComm_t, int*);
typedef ncclResult_t (*pfn_ncclAllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
typedef ncclResult_t (*pfn_ncclAllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
typedef const char* (*pfn_ncclGetErrorString)(ncclResult_t);

static int rccl_open(f1p_ctx* ctx) {
    if (ctx->rccl_lib) return F1P_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        ctx->rccl_lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
        if (ctx->rccl_lib) return F1P_OK;
    }
    return set_error(ctx, F1P_ECOMM, std::string("cannot load librccl.so: ") + dlerror());
}

template <typename F> static F rccl_sym(f1p_ctx* ctx, const char* name) { return (F)dlsym(ctx->rccl_lib, name); }

static std::string rccl_err(f1p_ctx* ctx, const char* what, ncclResult_t r) {
    auto es = rccl_sym<pfn_ncclGetErrorString>(ctx, "ncclGetErrorString");
    return std::string(what) + " failed: " + (es ? es(r) : "?") + " (code " + std::to_string((int)r) + ")";
}

int f1p_comm_unique_id(f1p_ctx* ctx, uint8_t id[F1P_COMM_ID_BYTES]) {
    F1P_ENTER(ctx);
    int rc = rccl_open(ctx); if (rc) return rc;
    auto fn = rccl_sym<pfn_ncclGetUniqueId>(ctx, "ncclGetUniqueId");
    if (!fn) return set_error(ctx, F1P_ECOMM, "ncclGetUniqueId not found");
    ncclUniqueId uid;
    const ncclResult_t r = fn(&uid);
    if (r != ncclSuccess) return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclGetUniqueId", r));
    memcpy(id, uid.internal, F1P_COMM_ID_BYTES);
    return F1P_OK;
}

int f1p_comm_init(f1p_ctx* ctx, const uint8_t id[F1P_COMM_ID_BYTES], int32_t nranks, int32_t rank) {
    F1P_ENTER(ctx);
    if (nranks < 1 || rank < 0 || rank >= nranks) return set_error(ctx, F1P_EINVAL, "bad nranks / rank");
    int rc = rccl_open(ctx); if (rc) return rc;
    if (ctx->comm) f1p_comm_destroy(ctx);
    auto fn = rccl_sym<pfn_ncclCommInitRank>(ctx, "ncclCommInitRank");
    if (!fn) return set_error(ctx, F1P_ECOMM, "ncclCommInitRank not found");
    ncclUniqueId uid;
    memcpy(uid.internal, id, F1P_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = fn(&comm, nranks, uid, rank);
    if (r != ncclSuccess) { ctx->comm = nullptr; return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclCommInitRank", r)); }
    ctx->comm = comm;
    ctx->comm_rank = rank; ctx->comm_nranks = nranks;
    return F1P_OK;
}

int f1p_comm_info(f1p_ctx* ctx, int32_t* nranks, int32_t* rank) {
    F1P_ENTER(ctx);
    if (!ctx->comm) return set_error(ctx, F1P_ESTATE, "communicator not initialised: call f1p_comm_init");
    auto cnt = rccl_sym<pfn_ncclCommCount>(ctx, "ncclCommCount");
    auto ur = rccl_sym<pfn_ncclCommUserRank>(ctx, "ncclCommUserRank");
    if (!cnt || !ur) return set_error(ctx, F1P_ECOMM, "ncclCommCount / ncclCommUserRank not found");
    int n = 0, r = 0;
    ncclResult_t e = cnt((ncclComm_t)ctx->comm, &n);
    if (e == ncclSuccess) e = ur((ncclComm_t)ctx->comm, &r);
    if (e != ncclSuccess) return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclCommCount", e));
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    return F1P_OK;
}

int f1p_comm_destroy(f1p_ctx* ctx) {
    if (!ctx) return F1P_EINVAL;
    if (ctx->comm && ctx->rccl_lib) {
        auto fn = rccl_sym<pfn_ncclCommDestroy>(ctx, "ncclCommDestroy");
        if (fn) (void)fn((ncclComm_t)ctx->comm);
    }
    ctx->comm = nullptr;
    return F1P_OK;
}

// Cross-rank argmin with np.argmin's rules (first minimum; a NaN cost is "smaller" than any number, lattice_planner.py:159-172,
// f1p::argmin_better).  ncclMin on floating point leaves NaN handling unspecified, so the cost travels as a monotone
// unsigned 64-bit key (k_argmin_key: NaN -> 0, otherwise the IEEE bits made order-preserving) and both reductions are
// integer minima: all-reduce(min, u64) on the key, then all-reduce(min, i32) on the index among the ranks holding that key.
// The key map is a bijection on non-NaN doubles (-0.0 is folded into +0.0, which np.argmin also treats as equal), so the
// cost that comes back is bit-identical to the single-GPU result.
int f1p_comm_argmin_dev(f1p_ctx* ctx, double* d_cost, int32_t* d_idx, int32_t E) {
    F1P_ENTER(ctx);
    if (!ctx->comm) return set_error(ctx, F1P_ESTATE, "communicator not initialised: call f1p_comm_init");
    if (E < 0 || (E > 0 && (!d_cost || !d_idx))) return set_error(ctx, F1P_EINVAL, "bad cost / idx / E");
    if (E == 0) return F1P_OK;
    if (E > ctx->comm_cap) {
        F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_comm_key) (void)hipFree(ctx->d_comm_key);
        if (ctx->d_comm_idx) (void)hipFree(ctx->d_comm_idx);
        ctx->d_comm_key = nullptr; ctx->d_comm_idx = nullptr; ctx->comm_cap = 0;
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_comm_key, sizeof(uint64_t) * 2 * (size_t)E));   // [own keys | reduced keys]
        F1P_HIP(ctx, hipMalloc((void**)&ctx->d_comm_idx, sizeof(int32_t) * (size_t)E));
        ctx->comm_cap = E;
    }
    if (ctx->comm_exchange == 1) {
        // ONE collective: all-gather of the (key, index) records (16 B per ego and rank), then every rank takes the minimum itself.  Half
        // the xGMI latency of the two dependent all-reduces below at the price of N x 16 B instead of 12 B per ego on the wire.
        const int N = ctx->comm_nranks;
        if (E > ctx->comm_rec_cap || N != ctx->comm_rec_ranks) {
            F1P_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (ctx->d_comm_rec) (void)hipFree(ctx->d_comm_rec);
            ctx->d_comm_rec = nullptr; ctx->comm_rec_cap = 0;
            F1P_HIP(ctx, hipMalloc((void**)&ctx->d_comm_rec, sizeof(uint64_t) * 2 * (size_t)E * (size_t)(N + 1)));
            ctx->comm_rec_cap = E; ctx->comm_rec_ranks = N;
        }
        auto ag = rccl_sym<pfn_ncclAllGather>(ctx, "ncclAllGather");
        if (!ag) return set_error(ctx, F1P_ECOMM, "ncclAllGather not found");
        uint64_t* mine = ctx->d_comm_rec;
        uint64_t* all = ctx->d_comm_rec + 2 * (size_t)ctx->comm_rec_cap;
        int rc1 = launch_argmin_pack(ctx, d_cost, d_idx, mine, E); if (rc1) return rc1;
        ncclResult_t r1 = ag(mine, all, 2 * (size_t)E, ncclUint64, (ncclComm_t)ctx->comm, ctx->stream);
        if (r1 != ncclSuccess) return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclAllGather(u64)", r1));
        return launch_argmin_reduce(ctx, all, N, E, d_idx, d_cost);
    }
    auto ar = rccl_sym<pfn_ncclAllReduce>(ctx, "ncclAllReduce");
    if (!ar) return set_error(ctx, F1P_ECOMM, "ncclAllReduce not found");
    uint64_t* own = ctx->d_comm_key;
    uint64_t* red = ctx->d_comm_key + E;
    int rc = launch_argmin_key(ctx, d_cost, own, E); if (rc) return rc;
    // 1. global minimum key per ego
    ncclResult_t r = ar(own, red, (size_t)E, ncclUint64, ncclMin, (ncclComm_t)ctx->comm, ctx->stream);
    if (r != ncclSuccess) return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclAllReduce(min, u64)", r));
    // 2. ranks that hold that key keep their index, the others contribute INT32_MAX; the winning cost is decoded in place
    rc = launch_argmin_mask(ctx, own, red, d_idx, ctx->d_comm_idx, d_cost, E); if (rc) return rc;
    // 3. lowest index among the holders (np.argmin first-minimum rule)
    r = ar(ctx->d_comm_idx, d_idx, (size_t)E, ncclInt32, ncclMin, (ncclComm_t)ctx->comm, ctx->stream);
    if (r != ncclSuccess) return set_error(ctx, F1P_ECOMM, rccl_err(ctx, "ncclAllReduce(min, i32)", r));
    return F1P_OK;
}

int f1p_comm_set_exchange(f1p_ctx* ctx, int32_t mode) {
    if (!ctx) return F1P_EINVAL;
    if (mode != 0 && mode != 1) return set_error(ctx, F1P_EINVAL, "mode must be 0 (two all-reduces) or 1 (one all-gather + local minimum)");
    ctx->comm_exchange = mode;
    return F1P_OK;
}

// the local kernels of the single-collective exchange on host arrays (the all-gather replaced by the caller): cost / idx [N][E] of N
// emulated ranks -> idx_out [E], cost_out [E]
int f1p_argmin_gather_reduce_batch(f1p_ctx* ctx, const double* cost, const int32_t* idx, int32_t N, int32_t E, int32_t* idx_out, double* cost_out) {
    F1P_ENTER(ctx);
    if (N < 1 || E < 0 || (E > 0 && (!cost || !idx || !idx_out || !cost_out))) return set_error(ctx, F1P_EINVAL, "bad argument");
    const size_t n = (size_t)N * E;
    Stage s(ctx);
    s.need(8 * n); s.need(4 * n); s.need(16 * n); s.need(4 * (size_t)E); s.need(8 * (size_t)E);
    int rc = s.begin(); if (rc) return rc;
    const double* d_c; const int32_t* d_i;
    if ((rc = s.in(cost, n, &d_c))) return rc;
    if ((rc = s.in(idx, n, &d_i))) return rc;
    uint64_t* d_rec = (uint64_t*)arena_take(ctx, 16 * n);
    int32_t* d_io = s.out(idx_out, (size_t)E); double* d_co = s.out(cost_out, (size_t)E);
    for (int r = 0; r < N; ++r)
        if ((rc = launch_argmin_pack(ctx, d_c + (size_t)r * E, d_i + (size_t)r * E, d_rec + 2 * (size_t)r * E, E))) return rc;
    if ((rc = launch_argmin_reduce(ctx, d_rec, N, E, d_io, d_co))) return rc;
    return s.finish();
}

// the two local kernels of the exchange on host arrays (the collective replaced by the caller): lets a single-GPU box check
// the key map against np.argmin for NaN / inf / signed-zero costs.  keys_out [E] <- key(cost[e]);
int f1p_argmin_key_batch(f1p_ctx* ctx, const double* cost, int32_t E, uint64_t* keys_out) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!cost || !keys_out))) return set_error(ctx, F1P_EINVAL, "bad cost / keys / E");
    Stage s(ctx);
    s.need(8 * (size_t)E); s.need(8 * (size_t)E);
    int rc = s.begin(); if (rc) return rc;
    const double* d_c;
    if ((rc = s.in(cost, (size_t)E, &d_c))) return rc;
    uint64_t* d_k = s.out(keys_out, (size_t)E);
    if ((rc = launch_argmin_key(ctx, d_c, d_k, E))) return rc;
    return s.finish();
}
// own_keys / min_keys / idx [E] -> masked_idx [E] (idx where own == min, else INT32_MAX), cost_out [E] = decoded min key
int f1p_argmin_mask_batch(f1p_ctx* ctx, const uint64_t* own_keys, const uint64_t* min_keys, const int32_t* idx, int32_t E,
                          int32_t* masked_idx, double* cost_out) {
    F1P_ENTER(ctx);
    if (E < 0 || (E > 0 && (!own_keys || !min_keys || !idx || !masked_idx || !cost_out))) return set_error(ctx, F1P_EINVAL, "NULL argument");
    Stage s(ctx);
    s.need(8 * (size_t)E); s.need(8 * (size_t)E); s.need(4 * (size_t)E); s.need(4 * (size_t)E); s.need(8 * (size_t)E);
    int rc = s.begin(); if (rc) return rc;
    const uint64_t *d_o, *d_m; const int32_t* d_i;
    if ((rc = s.in(own_keys, (size_t)E, &d_o))) return rc;
    if ((rc = s.in(min_keys, (size_t)E, &d_m))) return rc;
    if ((rc = s.in(idx, (size_t)E, &d_i))) return rc;
    int32_t* d_mi = s.out(masked_idx, (size_t)E); double* d_c = s.out(cost_out, (size_t)E);
    if ((rc = launch_argmin_mask(ctx, d_o, d_m, d_i, d_mi, d_c, E))) return rc;
    return s.finish();
}
