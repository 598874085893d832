// api_comm.hip — shards and gathers: a shard's rows, the RCCL gather (vpt_comm_*) and the peer-copy gather of one process's contexts.  The only
// file of the host layer that includes rccl.h: vpt_ctx::comm is an opaque pointer everywhere else.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "api_ctx.hpp"

using namespace vpt::api;

// ---- helpers of this file alone
namespace {

int ensure_gather_buf(vpt_ctx* c) {
    if (c->gather_buf) return VPT_OK;
    HIPCHK(c, hipMalloc((void**)&c->gather_buf, vpt_shard_floats(c) * 4 * (size_t)c->P.shard_count));
    return VPT_OK;
}
int nccl_fail(vpt_ctx* c, const char* what, ncclResult_t r) {
    c->err = std::string(what) + " failed: " + ncclGetErrorString(r);
    return VPT_ERR_DEVICE;
}
// root: gather_buf -> full image (rows re-interleaved); shard_count == 1: the image already is the whole image
int assemble_from_gather_buf(vpt_ctx* c) {
    if (c->P.shard_count == 1) return VPT_OK;
    launch_scatter_rows(c->main.stream, c->gather_buf, c->full_image, c->P.width, c->P.height, c->P.shard_count, (uint32_t)(vpt_shard_floats(c) / 4));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    HIPCHK(c, hipGetLastError());
    c->full_valid = true;
    return VPT_OK;
}

}  // namespace

extern "C" {

size_t vpt_shard_floats(const vpt_ctx* c) {
    if (!c) return 0;
    uint32_t max_rows = shard_rows_of(c->P.height, 0, c->P.shard_count);
    return (size_t)max_rows * c->P.width * 4;
}
int vpt_get_shard_device(vpt_ctx* c, void* dst) {
    if (!c || !dst) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    { int rd = quiesce(c); if (rd) return rd; }
    size_t bytes = (size_t)c->P.shard_pixels * 16, padded = vpt_shard_floats(c) * 4;
    HIPCHK(c, hipMemcpyAsync(dst, c->image, bytes, hipMemcpyDeviceToDevice, c->main.stream));
    if (padded > bytes) HIPCHK(c, hipMemsetAsync((char*)dst + bytes, 0, padded - bytes, c->main.stream));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return VPT_OK;
}
int vpt_assemble_shards(vpt_ctx* c, const void* gathered, uint32_t shard_count) {
    if (!c || !gathered) return VPT_ERR_INVALID_ARGUMENT;
    if (shard_count != c->P.shard_count) return fail(c, VPT_ERR_INVALID_ARGUMENT, "shard_count mismatch");
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    { int rd = quiesce(c); if (rd) return rd; }
    float* dst = c->P.shard_count > 1 ? c->full_image : c->image;
    launch_scatter_rows(c->main.stream, (const float*)gathered, dst, c->P.width, c->P.height, shard_count, (uint32_t)(vpt_shard_floats(c) / 4));
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    HIPCHK(c, hipGetLastError());
    c->full_valid = true;
    return VPT_OK;
}

// ---- the one collective of the path (include/vpt.h) ----
int vpt_comm_unique_id(void* id_out) {
    if (!id_out) return VPT_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(ncclUniqueId) == VPT_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return VPT_ERR_DEVICE;
    memcpy(id_out, &id, sizeof(id));
    return VPT_OK;
}
int vpt_comm_init(vpt_ctx* c, const void* id, int rank, int world) {
    if (!c || !id) return VPT_ERR_INVALID_ARGUMENT;
    if (world < 1 || rank < 0 || rank >= world || (uint32_t)rank != c->P.shard_rank || (uint32_t)world != c->P.shard_count)
        return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_comm_init: rank / world must equal the context's shard_rank / shard_count");
    if (c->comm) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_comm_init: the context already has a communicator");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    {   // the RCCL behind these calls is whichever librccl the process mapped first, not necessarily the one linked against
        int v = 0;
        if (ncclGetVersion(&v) != ncclSuccess) return fail(c, VPT_ERR_DEVICE, "ncclGetVersion failed");
        if (v / 10000 != NCCL_VERSION_CODE / 10000) {
            char msg[160]; snprintf(msg, sizeof(msg), "vpt_comm_init: the mapped RCCL is version %d, this library was built against %d (different major version)", v, (int)NCCL_VERSION_CODE);
            return fail(c, VPT_ERR_DEVICE, msg);
        }
    }
    ncclUniqueId uid; memcpy(&uid, id, sizeof(uid));
    ncclResult_t r = ncclCommInitRank(&c->comm, world, uid, rank);
    if (r != ncclSuccess) { c->comm = nullptr; return nccl_fail(c, "ncclCommInitRank", r); }
    c->comm_rank = rank; c->comm_world = world;
    return VPT_OK;
}
int vpt_comm_gather_shards(vpt_ctx* c, int root) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (!c->comm) return fail(c, VPT_ERR_INVALID_ARGUMENT, "vpt_comm_gather_shards before vpt_comm_init");
    if (root < 0 || root >= c->comm_world) return fail(c, VPT_ERR_INVALID_ARGUMENT, "root out of range");
    if (!c->buffers_ok) return fail(c, VPT_ERR_DEVICE, "no render buffers: the last vpt_resize failed");
    { int rd = quiesce(c); if (rd) return rd; }
    const bool is_root = c->comm_rank == root;
    if (is_root) { int rc = ensure_gather_buf(c); if (rc) return rc; }
    // every rank contributes its rows padded to the largest shard (the image buffer is allocated at that size);
    // the launch is ordered behind the renders already on the context's stream
    ncclResult_t r = ncclGather(c->image, is_root ? c->gather_buf : nullptr, vpt_shard_floats(c), ncclFloat32, root, c->comm, c->main.stream);
    if (r != ncclSuccess) return nccl_fail(c, "ncclGather", r);
    HIPCHK(c, hipStreamSynchronize(c->main.stream));
    return is_root ? assemble_from_gather_buf(c) : VPT_OK;
}
int vpt_comm_get_info(vpt_ctx* c, vpt_comm_info* out) {
    if (!c || !out) return VPT_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    int v = 0;
    if (ncclGetVersion(&v) == ncclSuccess) out->rccl_version_runtime = v;
    out->rccl_version_compiled = (int32_t)NCCL_VERSION_CODE;
    Dl_info di{};
    if (dladdr((const void*)&ncclGather, &di) && di.dli_fname) snprintf(out->library_path, sizeof(out->library_path), "%s", di.dli_fname);
    out->rank = -1; out->device = -1;
    if (c->comm) {
        int n = 0, r = -1, d = -1;
        if (ncclCommCount(c->comm, &n) != ncclSuccess || ncclCommUserRank(c->comm, &r) != ncclSuccess || ncclCommCuDevice(c->comm, &d) != ncclSuccess)
            return fail(c, VPT_ERR_DEVICE, "ncclCommCount / ncclCommUserRank / ncclCommCuDevice failed");
        out->nranks = n; out->rank = r; out->device = d;
    }
    return VPT_OK;
}
int vpt_comm_destroy(vpt_ctx* c) {
    if (!c) return VPT_ERR_INVALID_ARGUMENT;
    if (c->comm) {
        (void)hipSetDevice(c->cfg.device);
        ncclResult_t r = ncclCommDestroy(c->comm);
        c->comm = nullptr; c->comm_rank = -1; c->comm_world = 0;
        if (r != ncclSuccess) return nccl_fail(c, "ncclCommDestroy", r);
    }
    return VPT_OK;
}
int vpt_multi_gather_shards(vpt_ctx* const* ctxs, uint32_t count, uint32_t root) {
    if (!ctxs || count == 0 || root >= count || !ctxs[root]) return VPT_ERR_INVALID_ARGUMENT;
    vpt_ctx* R = ctxs[root];
    if (R->P.shard_count != count) return fail(R, VPT_ERR_INVALID_ARGUMENT, "vpt_multi_gather_shards: count must equal shard_count");
    for (uint32_t k = 0; k < count; k++) {
        vpt_ctx* c = ctxs[k];
        if (!c || c->P.shard_rank != k || c->P.shard_count != count || c->P.width != R->P.width || c->P.height != R->P.height || !c->buffers_ok)
            return fail(R, VPT_ERR_INVALID_ARGUMENT, "vpt_multi_gather_shards: context k must be shard k of the same image");
    }
    for (uint32_t k = 0; k < count; k++) { HIPCHK(R, hipSetDevice(ctxs[k]->cfg.device)); int rd = drain(ctxs[k]); if (rd) return rd; }
    HIPCHK(R, hipSetDevice(R->cfg.device));
    int rc = ensure_gather_buf(R);
    if (rc) return rc;
    const size_t stride = vpt_shard_floats(R) * 4;
    for (uint32_t k = 0; k < count; k++) {   // direct peer copies: xGMI is point to point, every shard takes its own link into root
        vpt_ctx* c = ctxs[k];
        HIPCHK(R, hipSetDevice(c->cfg.device));
        if (c->cfg.device != R->cfg.device) {
            hipError_t e = hipDeviceEnablePeerAccess(R->cfg.device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); }  // the copy below then stages through the host
            else (void)hipGetLastError();
        }
        HIPCHK(R, hipMemcpyPeerAsync((char*)R->gather_buf + (size_t)k * stride, R->cfg.device, c->image, c->cfg.device, stride, c->main.stream));
    }
    for (uint32_t k = 0; k < count; k++) {
        HIPCHK(R, hipSetDevice(ctxs[k]->cfg.device));
        HIPCHK(R, hipStreamSynchronize(ctxs[k]->main.stream));
    }
    HIPCHK(R, hipSetDevice(R->cfg.device));
    return assemble_from_gather_buf(R);
}

}  // extern "C"
