// C ABI, host side: the multi-GPU gather of the packed primitive lists (see cape_gather.hip) -- packing, the RCCL communicator,
// the gathers and the primitive count.
#include <cstring>

#include "cape_handle.h"

using namespace cape::abi;

namespace {

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

void fill_layout(const cape_handle_s* h, const cape_gather_config& c, cape_gather_layout& L)
{
    L = cape_gather_layout{};
    L.frames_capacity = c.frames_capacity;
    L.planes_capacity = c.frames_capacity * c.planes_per_frame;
    L.cylinders_capacity = c.frames_capacity * c.cylinders_per_frame;
    L.cells = h->cells;
    size_t off = align16(sizeof(cape_packed_header));
    L.frames_offset = off;
    off = align16(off + (size_t)L.frames_capacity * sizeof(cape_packed_frame));
    L.planes_offset = off;
    off = align16(off + (size_t)L.planes_capacity * sizeof(cape_packed_plane));
    L.cylinders_offset = off;
    off = align16(off + (size_t)L.cylinders_capacity * sizeof(cape_packed_cylinder));
    if (c.flags & CAPE_GATHER_LABELS)
    {
        L.plane_labels_offset = off;
        off = align16(off + (size_t)L.frames_capacity * h->cells);
        L.cyl_labels_offset = off;
        off = align16(off + (size_t)L.frames_capacity * h->cells);
    }
    L.bytes_per_rank = off;
}

// default capacities the first time a pack / gather is asked for without cape_gather_configure
int ensure_gather_configured(cape_handle_s* h)
{
    if (h->gather.packed[0])
        return CAPE_OK;
    cape_gather_config c{};
    c.frames_capacity = h->cfg.max_batch;
    return cape_gather_configure(h, &c, nullptr);
}

int pack_into_next_slot(cape_handle_s* h, int n_frames, int first_frame, hipStream_t stream)
{
    auto& G = h->gather;
    const int slot = G.packSlot ^ 1;
    // the slot may still be read by the all-gather of two batches ago
    if (G.packedBusy[slot])
    {
        CAPE_HIP_TRY(hipStreamWaitEvent(stream, G.packedFree[slot], 0));
        G.packedBusy[slot] = false;
    }
    const cape_gather_layout& L = G.layout;
    unsigned char* base = G.packed[slot];
    cape::PackParams p{};
    p.records = h->res.records;
    p.recordsBase = h->res.records;
    p.poolBase = h->cfg.max_batch;
    p.planeLabelsIn = h->res.planeLabels;
    p.cylLabelsIn = h->res.cylLabels;
    p.header = reinterpret_cast<cape_packed_header*>(base);
    p.frames = reinterpret_cast<cape_packed_frame*>(base + L.frames_offset);
    p.planes = reinterpret_cast<cape_packed_plane*>(base + L.planes_offset);
    p.cylinders = reinterpret_cast<cape_packed_cylinder*>(base + L.cylinders_offset);
    p.planeLabels8 = L.plane_labels_offset ? base + L.plane_labels_offset : nullptr;
    p.cylLabels8 = L.cyl_labels_offset ? base + L.cyl_labels_offset : nullptr;
    p.nFrames = n_frames;
    p.firstFrame = first_frame;
    p.framesCapacity = L.frames_capacity;
    p.planesCapacity = L.planes_capacity;
    p.cylindersCapacity = L.cylinders_capacity;
    p.cells = h->cells;
    p.flags = G.cfg.flags;
    CAPE_HIP_TRY(cape::launch_pack(p, stream));
    G.packSlot = slot;
    return CAPE_OK;
}

// root < 0: ncclAllGather (every rank receives); root >= 0: ncclGather to that rank (recv_dev is read on the root only)
int gather_impl(cape_handle h, int32_t n_frames, int32_t first_frame, int32_t root, void* recv_dev, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& G = h->gather;
    if (!G.comm)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no communicator: call cape_comm_init first");
    if (root >= G.commWorld)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "root outside [0, world)");
    if (!recv_dev && (root < 0 || root == G.commRank))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "recv_dev is null on a receiving rank");
    if (root >= 0 && !cape::rccl_has_gather())
        return fail(CAPE_ERR_UNSUPPORTED, "this librccl.so has no ncclGather: use cape_gather_primitives");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    if (const int rc = ensure_gather_configured(h); rc != CAPE_OK)
        return rc;
    if (n_frames > G.layout.frames_capacity)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds cape_gather_config.frames_capacity");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (const int rc = pack_into_next_slot(h, n_frames, first_frame, stream); rc != CAPE_OK)
        return rc;
    const int slot = G.packSlot;
    // the collective runs on the handle's own stream, behind the pack kernels: the caller's stream is free for the
    // kernels of the next batch
    CAPE_HIP_TRY(hipEventRecord(G.packReady, stream));
    CAPE_HIP_TRY(hipStreamWaitEvent(G.commStream, G.packReady, 0));
    if (root < 0)
    {
        if (const int rc = cape::rccl_all_gather_bytes(G.packed[slot], recv_dev, G.layout.bytes_per_rank, G.comm, G.commStream); rc != 0)
            return fail(CAPE_ERR_HIP, std::string("ncclAllGather: ") + cape::rccl_error_string(rc));
    }
    else if (const int rc = cape::rccl_gather_bytes(G.packed[slot], recv_dev, G.layout.bytes_per_rank, root, G.comm, G.commStream);
             rc != 0)
        return fail(CAPE_ERR_HIP, std::string("ncclGather: ") + cape::rccl_error_string(rc));
    CAPE_HIP_TRY(hipEventRecord(G.packedFree[slot], G.commStream));
    G.packedBusy[slot] = true;
    CAPE_HIP_TRY(hipEventRecord(G.done, G.commStream));
    G.pending = true;
    return CAPE_OK;
}

} // namespace

extern "C" {

int cape_gather_configure(cape_handle h, const cape_gather_config* cfg, cape_gather_layout* layout_out)
{
    if (!h || !cfg)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    cape_gather_config c = *cfg;
    if (c.planes_per_frame == 0)
        c.planes_per_frame = 16;
    if (c.cylinders_per_frame == 0)
        c.cylinders_per_frame = 8;
    if (c.frames_capacity <= 0 || c.frames_capacity > h->cfg.max_batch || c.planes_per_frame < 0 ||
        c.planes_per_frame > 4096 || c.cylinders_per_frame < 0 || c.cylinders_per_frame > 4096 ||
        (c.flags & ~(uint32_t)CAPE_GATHER_LABELS))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "frames_capacity in [1, max_batch], planes/cylinders per frame in [1, 4096], known flags");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize()); // nothing may still read the old slots
    auto& G = h->gather;
    cape_gather_layout L;
    fill_layout(h, c, L);
    for (int k = 0; k < 2; ++k)
    {
        G.packed[k].reset();
        G.packedBusy[k] = false;
    }
    G.pending = false;
    for (int k = 0; k < 2; ++k)
    {
        CAPE_HIP_TRY(G.packed[k].alloc(L.bytes_per_rank));
        CAPE_HIP_TRY(hipMemset(G.packed[k], 0, L.bytes_per_rank));
        CAPE_HIP_TRY(G.packedFree[k].ensure());
    }
    CAPE_HIP_TRY(G.packReady.ensure());
    CAPE_HIP_TRY(G.done.ensure());
    G.cfg = c;
    G.layout = L;
    if (layout_out)
        *layout_out = L;
    return CAPE_OK;
}

int cape_pack_primitives(cape_handle h, int32_t n_frames, int32_t first_frame, void** packed_dev, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    if (const int rc = ensure_gather_configured(h); rc != CAPE_OK)
        return rc;
    if (n_frames > h->gather.layout.frames_capacity)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds cape_gather_config.frames_capacity");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (const int rc = pack_into_next_slot(h, n_frames, first_frame, stream); rc != CAPE_OK)
        return rc;
    if (packed_dev)
        *packed_dev = h->gather.packed[h->gather.packSlot];
    return CAPE_OK;
}

int cape_copy_packed(cape_handle h, void* packed_host)
{
    if (!h || !packed_host)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->gather.packed[0])
        return fail(CAPE_ERR_INVALID_ARGUMENT, "nothing has been packed yet");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(hipMemcpy(packed_host, h->gather.packed[h->gather.packSlot], h->gather.layout.bytes_per_rank, hipMemcpyDeviceToHost));
    return CAPE_OK;
}

int cape_comm_unique_id(void* id_out)
{
    if (!id_out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    if (const char* why = cape::rccl_load())
        return fail(CAPE_ERR_UNSUPPORTED, why);
    cape::RcclUniqueId id;
    if (const int rc = cape::rccl_unique_id(&id); rc != 0)
        return fail(CAPE_ERR_HIP, std::string("ncclGetUniqueId: ") + cape::rccl_error_string(rc));
    std::memcpy(id_out, id.internal, CAPE_COMM_ID_BYTES);
    return CAPE_OK;
}

int cape_comm_init(cape_handle h, const void* id_, int32_t rank, int32_t world)
{
    if (!h || !id_ || world <= 0 || rank < 0 || rank >= world)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or rank outside [0, world)");
    auto& G = h->gather;
    if (G.comm)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the handle already has a communicator (cape_comm_destroy first)");
    if (const char* why = cape::rccl_load())
        return fail(CAPE_ERR_UNSUPPORTED, why);
    CAPE_ON_DEVICE(h);
    cape::RcclUniqueId id;
    std::memcpy(id.internal, id_, CAPE_COMM_ID_BYTES);
    CAPE_HIP_TRY(G.commStream.ensure());
    if (const int rc = cape::rccl_comm_init(&G.comm, world, id, rank); rc != 0)
    {
        G.comm = nullptr;
        return fail(CAPE_ERR_HIP, std::string("ncclCommInitRank: ") + cape::rccl_error_string(rc));
    }
    G.commRank = rank;
    G.commWorld = world;
    return CAPE_OK;
}

int cape_comm_info(cape_handle h, cape_comm_info_t* out)
{
    if (!h || !out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->nranks = out->rank = out->device = -1;
    out->handle_device = h->cfg.device;
    if (!h->gather.comm)
        return CAPE_OK; // no communicator: has_comm = 0
    out->has_comm = 1;
    out->has_gather = cape::rccl_has_gather() ? 1 : 0;
    CAPE_ON_DEVICE(h);
    int count = -1, rank = -1, device = -1;
    cape::rccl_comm_query(h->gather.comm, &count, &rank, &device);
    out->nranks = count;
    out->rank = rank;
    out->device = device;
    out->init_nranks = h->gather.commWorld;
    out->init_rank = h->gather.commRank;
    return CAPE_OK;
}

int cape_comm_destroy(cape_handle h)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    auto& G = h->gather;
    if (!G.comm)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    if (G.commStream)
        CAPE_HIP_TRY(hipStreamSynchronize(G.commStream));
    const int rc = cape::rccl_comm_destroy(G.comm);
    G.comm = nullptr;
    G.pending = false;
    if (rc != 0)
        return fail(CAPE_ERR_HIP, std::string("ncclCommDestroy: ") + cape::rccl_error_string(rc));
    return CAPE_OK;
}

int cape_gather_primitives(cape_handle h, int32_t n_frames, int32_t first_frame, void* recv_dev, void* stream_)
{
    return gather_impl(h, n_frames, first_frame, -1, recv_dev, stream_);
}

int cape_gather_primitives_root(cape_handle h, int32_t n_frames, int32_t first_frame, int32_t root, void* recv_dev, void* stream_)
{
    if (root < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "root outside [0, world)");
    return gather_impl(h, n_frames, first_frame, root, recv_dev, stream_);
}

int cape_count_primitives(cape_handle h, int32_t n_frames, int32_t* n_planes, int32_t* n_cylinders, int32_t* max_planes_per_frame)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    int32_t tot[4] = {0, 0, 0, 0};
    if (n_frames > 0)
    {
        CAPE_HIP_TRY(h->gather.countScratch.ensure(4));
        // behind the batch, wherever it was enqueued (the caller's stream AND the handle's side stream of an asynchronous
        // second pass), without touching those streams
        CAPE_HIP_TRY(sync_handle(h));
        hipStream_t st = nullptr;
        CAPE_HIP_TRY(cape::launch_count_primitives(h->res.records, n_frames, h->gather.countScratch, st));
        CAPE_HIP_TRY(hipMemcpyAsync(tot, h->gather.countScratch, sizeof(tot), hipMemcpyDeviceToHost, st));
        CAPE_HIP_TRY(hipStreamSynchronize(st));
    }
    if (n_planes)
        *n_planes = tot[0];
    if (n_cylinders)
        *n_cylinders = tot[1];
    if (max_planes_per_frame)
        *max_planes_per_frame = tot[2];
    return CAPE_OK;
}

int cape_gather_wait(cape_handle h, void* stream_, int32_t host_sync)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->gather.pending)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    if (host_sync)
    {
        CAPE_HIP_TRY(hipEventSynchronize(h->gather.done));
        h->gather.pending = false;
    }
    else
    {
        CAPE_HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream_), h->gather.done, 0));
    }
    return CAPE_OK;
}

} // extern "C"
