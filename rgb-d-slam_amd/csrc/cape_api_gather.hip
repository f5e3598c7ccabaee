// C ABI, host side: the multi-GPU gather of the packed primitive lists (see cape_gather.hip) -- packing, the RCCL communicator,
// the gathers and the primitive count.
#include <cstring>
#include <limits>

#include "cape_handle.h"

using namespace cape::abi;

namespace {

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

void fill_layout(const cape_handle_s* h, const cape_gather_config& c, int vertices_per_frame, cape_gather_layout& L,
                 cape_gather_polygon_layout& PL)
{
    L = cape_gather_layout{};
    PL = cape_gather_polygon_layout{};
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
    if (c.flags & CAPE_GATHER_POLYGONS)
    {
        // appended behind everything the buffer holds without the flag: those sections keep their offsets
        PL.polygons_capacity = L.planes_capacity;
        PL.vertices_capacity = c.frames_capacity * vertices_per_frame;
        PL.polygon_header_offset = off;
        off = align16(off + sizeof(cape_packed_polygon_header));
        PL.polygons_offset = off;
        off = align16(off + (size_t)PL.polygons_capacity * sizeof(cape_polygon));
        PL.vertices_offset = off;
        off = align16(off + (size_t)PL.vertices_capacity * 2 * sizeof(double));
    }
    L.bytes_per_rank = off;
}

// scratch of the pack kernels with CAPE_GATHER_POLYGONS: per frame an int2 (ring vertices, kept polygons) and a 64-bit vertex offset,
// then one 64-bit word (vertices of the shipped rings)
size_t ring_scratch_bytes(int frames) { return (size_t)frames * (sizeof(int2) + sizeof(long long)) + sizeof(unsigned long long); }

// the polygons of cape_build_polygons cover frames [0, n_frames) of the current batch (the rule of cape_copy_polygons)
int require_polygons(const cape_handle_s* h, int n_frames, const char* who)
{
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, std::string(who) + ": n_frames exceeds the frames of the last cape_build_polygons of the current batch "
                                                          "(call cape_build_polygons after cape_extract first)");
    return CAPE_OK;
}

// what the pack and count kernels read of the batch: its records and, with polygons, their rows and vertex slabs
void bind_batch(const cape_handle_s* h, int n_frames, bool polygons, cape::PackParams& p)
{
    p.records = h->res.records;
    p.recordsBase = h->res.records;
    p.poolBase = h->cfg.max_batch;
    p.nFrames = n_frames;
    if (polygons)
    {
        p.polygonsIn = h->poly.polygons;
        p.verticesIn = reinterpret_cast<const double2*>(h->poly.vertices.get());
        p.boundaryCapacity = h->boundaryCap;
    }
}

int configure_impl(cape_handle h, const cape_gather_config* cfg, int32_t vertices_per_frame, bool polygons, cape_gather_layout* layout_out,
                   cape_gather_polygon_layout* polygon_layout_out)
{
    if (!h || !cfg)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    cape_gather_config c = *cfg;
    if (polygons)
        c.flags |= CAPE_GATHER_POLYGONS;
    if (c.planes_per_frame == 0)
        c.planes_per_frame = 16;
    if (c.cylinders_per_frame == 0)
        c.cylinders_per_frame = 8;
    if (vertices_per_frame == 0)
        vertices_per_frame = CAPE_GATHER_DEFAULT_VERTICES_PER_FRAME;
    if (c.frames_capacity <= 0 || c.frames_capacity > h->cfg.max_batch || c.planes_per_frame < 0 ||
        c.planes_per_frame > 4096 || c.cylinders_per_frame < 0 || c.cylinders_per_frame > 4096 ||
        (c.flags & ~(uint32_t)(CAPE_GATHER_LABELS | CAPE_GATHER_POLYGONS)))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "frames_capacity in [1, max_batch], planes/cylinders per frame in [1, 4096], known flags");
    if (vertices_per_frame < 0 || (int64_t)c.frames_capacity * vertices_per_frame > std::numeric_limits<int32_t>::max())
        return fail(CAPE_ERR_INVALID_ARGUMENT, "vertices_per_frame >= 0 and frames_capacity x vertices_per_frame within an int32");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize()); // nothing may still read the old slots
    auto& G = h->gather;
    cape_gather_layout L;
    cape_gather_polygon_layout PL;
    fill_layout(h, c, vertices_per_frame, L, PL);
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
    if (c.flags & CAPE_GATHER_POLYGONS)
        CAPE_HIP_TRY(G.ringScratch.alloc(ring_scratch_bytes(c.frames_capacity)));
    CAPE_HIP_TRY(G.packReady.ensure());
    CAPE_HIP_TRY(G.done.ensure());
    G.cfg = c;
    G.layout = L;
    G.polygonLayout = PL;
    if (layout_out)
        *layout_out = L;
    if (polygon_layout_out)
        *polygon_layout_out = PL;
    return CAPE_OK;
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
    const bool polygons = (G.cfg.flags & CAPE_GATHER_POLYGONS) != 0;
    if (polygons)
        if (const int rc = require_polygons(h, n_frames, "packing with CAPE_GATHER_POLYGONS"); rc != CAPE_OK)
            return rc; // (before anything is written: nothing is packed)
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
    bind_batch(h, n_frames, polygons, p);
    p.planeLabelsIn = h->res.planeLabels;
    p.cylLabelsIn = h->res.cylLabels;
    p.header = reinterpret_cast<cape_packed_header*>(base);
    p.frames = reinterpret_cast<cape_packed_frame*>(base + L.frames_offset);
    p.planes = reinterpret_cast<cape_packed_plane*>(base + L.planes_offset);
    p.cylinders = reinterpret_cast<cape_packed_cylinder*>(base + L.cylinders_offset);
    p.planeLabels8 = L.plane_labels_offset ? base + L.plane_labels_offset : nullptr;
    p.cylLabels8 = L.cyl_labels_offset ? base + L.cyl_labels_offset : nullptr;
    p.firstFrame = first_frame;
    p.framesCapacity = L.frames_capacity;
    p.planesCapacity = L.planes_capacity;
    p.cylindersCapacity = L.cylinders_capacity;
    p.cells = h->cells;
    p.flags = G.cfg.flags;
    if (polygons)
    {
        const cape_gather_polygon_layout& PL = G.polygonLayout;
        p.polygonHeader = reinterpret_cast<cape_packed_polygon_header*>(base + PL.polygon_header_offset);
        p.polygons = reinterpret_cast<cape_polygon*>(base + PL.polygons_offset);
        p.vertices = reinterpret_cast<double2*>(base + PL.vertices_offset);
        p.verticesCapacity = PL.vertices_capacity;
        unsigned char* scratch = G.ringScratch;
        p.frameRings = reinterpret_cast<int2*>(scratch);
        p.frameVertexOffset = reinterpret_cast<long long*>(scratch + (size_t)L.frames_capacity * sizeof(int2));
        p.verticesUsed = reinterpret_cast<unsigned long long*>(scratch + (size_t)L.frames_capacity * (sizeof(int2) + sizeof(long long)));
    }
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
    return configure_impl(h, cfg, 0, false, layout_out, nullptr);
}

int cape_gather_configure_polygons(cape_handle h, const cape_gather_config* cfg, int32_t vertices_per_frame, cape_gather_layout* layout_out,
                                   cape_gather_polygon_layout* polygon_layout_out)
{
    if (vertices_per_frame < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "negative vertices_per_frame");
    return configure_impl(h, cfg, vertices_per_frame, true, layout_out, polygon_layout_out);
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

int cape_count_polygon_vertices(cape_handle h, int32_t n_frames, int64_t* n_vertices, int32_t* max_vertices_per_frame)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    if (const int rc = require_polygons(h, n_frames, "cape_count_polygon_vertices"); rc != CAPE_OK)
        return rc;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    unsigned long long tot[2] = {0ull, 0ull};
    if (n_frames > 0)
    {
        CAPE_HIP_TRY(h->gather.vertexCountScratch.ensure(2));
        CAPE_HIP_TRY(sync_handle(h)); // behind the batch and its polygons, wherever they were enqueued (as cape_count_primitives)
        hipStream_t st = nullptr;
        cape::PackParams p{};
        bind_batch(h, n_frames, true, p);
        CAPE_HIP_TRY(cape::launch_count_polygon_vertices(p, h->gather.vertexCountScratch, st));
        CAPE_HIP_TRY(hipMemcpyAsync(tot, h->gather.vertexCountScratch, sizeof(tot), hipMemcpyDeviceToHost, st));
        CAPE_HIP_TRY(hipStreamSynchronize(st));
    }
    if (n_vertices)
        *n_vertices = (int64_t)tot[0];
    if (max_vertices_per_frame)
        *max_vertices_per_frame = (int32_t)tot[1];
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
