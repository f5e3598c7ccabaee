// C ABI, host side: debug and test entry points -- per-cell statistics, the seed sequence, one polygon on its own, profile
// slots and the internal counters of the rectify, polygon and matching kernels.
#include <memory>
#include <new>
#include <vector>

#include "cape_handle.h"

using namespace cape::abi;

extern "C" {

int cape_copy_cell_stats(cape_handle h, int32_t frame, cape_cell_stats* out)
{
    if (!h || !out || frame < 0 || frame >= h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    const size_t C = (size_t)h->cells, off = (size_t)frame * C;
    std::vector<double> sums(C * cape::kSumStride), plane(C * cape::kPlaneStride), score(C);
    std::vector<float> tol(C);
    std::vector<uint32_t> flags(C);
    std::vector<int32_t> bins(C);
    CAPE_HIP_TRY(copy_out(sums.data(), h->cellSums, off * cape::kSumStride, sums.size()));
    CAPE_HIP_TRY(copy_out(plane.data(), h->cellPlane, off * cape::kPlaneStride, plane.size()));
    CAPE_HIP_TRY(copy_out(score.data(), h->cellScore, off, C));
    CAPE_HIP_TRY(copy_out(tol.data(), h->cellTol, off, C));
    CAPE_HIP_TRY(copy_out(flags.data(), h->cellFlags, off, C));
    CAPE_HIP_TRY(copy_out(bins.data(), h->cellBins, off, C));
    for (size_t i = 0; i < C; ++i)
    {
        cape_cell_stats& o = out[i];
        for (int k = 0; k < 9; ++k)
            o.sums[k] = sums[i * cape::kSumStride + k];
        const double* p = &plane[i * cape::kPlaneStride];
        o.normal[0] = p[0]; o.normal[1] = p[1]; o.normal[2] = p[2];
        o.d = p[3];
        o.centroid[0] = p[4]; o.centroid[1] = p[5]; o.centroid[2] = p[6];
        o.mse = p[7];
        o.score = score[i];
        o.tol = tol[i];
        o.point_count = flags[i] & cape::kCountMask;
        o.bin = bins[i];
        o.planar = (flags[i] & cape::kFlagPlanar) ? 1u : 0u;
        o.inorder = (flags[i] & cape::kFlagInorder) ? 1u : 0u;
        o.pad = 0;
    }
    return CAPE_OK;
}

int cape_copy_seed_sequence(cape_handle h, int32_t frame, int32_t* seeds_out, int32_t capacity, int32_t* n_out)
{
    if (!h || !n_out || frame < 0 || frame >= h->cfg.max_batch || capacity < 0 || (capacity > 0 && !seeds_out))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame / buffer");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    cape_frame_header hdr;
    CAPE_HIP_TRY(hipMemcpy(&hdr, &h->res.records[frame].header, sizeof(hdr), hipMemcpyDeviceToHost));
    *n_out = hdr.n_seeds;
    int n = hdr.n_seeds < h->cells ? hdr.n_seeds : h->cells; // the buffer keeps one entry per cell
    n = n < capacity ? n : capacity;
    std::vector<uint16_t> tmp((size_t)(n > 0 ? n : 0));
    CAPE_HIP_TRY(copy_out(tmp.data(), h->seedSeq, (size_t)frame * h->cells, tmp.size()));
    for (int i = 0; i < n; ++i)
        seeds_out[i] = (int32_t)tmp[(size_t)i];
    return CAPE_OK;
}

int cape_debug_polygon(cape_handle h, const double* points3, int32_t n, const double* normal, const double* center,
                       cape_polygon* polygon_out, double* vertices_out)
{
    if (!h || !points3 || !normal || !center || !polygon_out || n < 0 || n > h->boundaryCap)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or more points than boundary_capacity");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    // a one-plane frame of its own: record, boundary points, polygon and vertex arrays (freed on the way out)
    std::unique_ptr<cape_frame_record> hostRec(new (std::nothrow) cape_frame_record());
    if (!hostRec)
        return fail(CAPE_ERR_HIP, "out of host memory");
    std::memset(hostRec.get(), 0, sizeof(cape_frame_record));
    hostRec->header.n_plane_segments = 1;
    hostRec->header.n_planes = 1;
    cape_plane_segment& s = hostRec->segments[0];
    for (int k = 0; k < 3; ++k)
    {
        s.normal[k] = normal[k];
        s.centroid[k] = center[k];
    }
    s.is_output = 1;
    s.planar = 1;
    s.boundary_offset = 0;
    s.boundary_count = (uint32_t)n;
    const size_t cap = (size_t)h->boundaryCap;
    Buffer<cape_frame_record> rec;
    Buffer<double> bnd, verts;
    Buffer<cape_polygon> poly;
    Buffer<unsigned char> ladder;
    CAPE_HIP_TRY(rec.alloc(1));
    CAPE_HIP_TRY(bnd.alloc(cap * 3));
    CAPE_HIP_TRY(poly.alloc(CAPE_MAX_PLANES));
    CAPE_HIP_TRY(verts.alloc(cap * 2));
    CAPE_HIP_TRY(ladder.alloc(cape::polygon_scratch_bytes(1, h->boundaryCap)));
    CAPE_HIP_TRY(hipMemcpy(rec, hostRec.get(), sizeof(cape_frame_record), hipMemcpyHostToDevice));
    if (n)
        CAPE_HIP_TRY(hipMemcpy(bnd, points3, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
    cape::PolygonParams p;
    p.records = rec;
    p.boundary = bnd;
    p.polygons = poly;
    p.vertices = reinterpret_cast<double2*>(verts.get());
    p.boundaryCapacity = h->boundaryCap;
    p.prof = nullptr;
    cape::polygon_bind_scratch(p, ladder, 1, h->boundaryCap);
    p.computeUnits = 4;
    p.originInCentroid = 1; // an arbitrary origin, as the caller asked
    CAPE_HIP_TRY(cape::launch_polygons(p, 1, nullptr));
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(copy_out(polygon_out, poly, 0, 1));
    CAPE_HIP_TRY(copy_out(vertices_out, verts, 0, (size_t)polygon_out->vertex_count * 2));
    return CAPE_OK;
}

int cape_debug_cycles(cape_handle h, int32_t n_frames, unsigned long long* out)
{
    if (!h || !out || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(copy_out(out, h->debugCycles, 0, (size_t)n_frames * cape::kProfileSlots));
    return CAPE_OK;
}

int cape_debug_rectify_flagged(cape_handle h, int32_t* count)
{
    if (!h || !count)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    *count = 0;
    if (!h->rectFlags)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    unsigned n = 0;
    CAPE_HIP_TRY(copy_out(&n, h->rectFlags, h->rectFlags.size() / 2, 1)); // (behind the per-frame flags: see cape_handle_s::rectFlags)
    *count = (int32_t)n;
    return CAPE_OK;
}

int cape_debug_polygon_queue(cape_handle h, uint32_t* reserved, uint32_t* tickets, uint32_t* slots)
{
    if (!h || !reserved || !tickets || !slots)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    *reserved = *tickets = *slots = 0;
    if (!h->poly.ladder || h->poly.frames <= 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    cape::PolygonParams p;
    cape::polygon_bind_scratch(p, h->poly.ladder, (size_t)h->cfg.max_batch + (size_t)h->chain.spillRecords, h->boundaryCap);
    uint32_t hd[2] = {0, 0};
    CAPE_HIP_TRY(hipMemcpy(hd, p.queue, sizeof hd, hipMemcpyDeviceToHost));
    *reserved = hd[0];
    *tickets = hd[1];
    const size_t wanted = cape::polygon_queue_slots((size_t)h->poly.frames + (size_t)h->chain.spillRecords); // (the batch + the spill pool)
    *slots = (uint32_t)(wanted < (size_t)p.queueCapacity ? wanted : (size_t)p.queueCapacity);
    return CAPE_OK;
}

int cape_debug_match_lists(cape_handle h, uint32_t* words32)
{
    if (!h || !words32)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    std::memset(words32, 0, 32 * sizeof(uint32_t));
    if (!h->poly.lists)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(copy_out(words32, h->poly.lists, 0, 32));
    return CAPE_OK;
}

int cape_debug_map_match_lists(cape_handle h, uint32_t* words8)
{
    if (!h || !words8)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    std::memset(words8, 0, 8 * sizeof(uint32_t));
    const unsigned char* work = h->lastMapMatcher == cape_handle_s::kMapMatchRecords ? h->map.work.get()
                                : h->lastMapMatcher == cape_handle_s::kMapMatchWide  ? h->mapWide.work.get()
                                : h->lastMapMatcher == cape_handle_s::kMapMatchShards ? h->shardMatch.work.get()
                                                                                      : nullptr;
    if (!work)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(hipMemcpy(words8, work, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost)); // (the counters start the buffer: map_work_layout)
    return CAPE_OK;
}

int cape_debug_ring_union(cape_handle h, const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, const double* frames27,
                          cape_plane_union* row_out, double* vertices_out)
{
    static const double kCanonical[27] = {1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0};
    if (!h || !ring_a || !ring_b || !row_out || !vertices_out || n_a < 3 || n_b < 3 || n_a > 4096 || n_b > 4096)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or a ring of fewer than 3 / more than 4096 vertices");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    // a one-pair launch over buffers of its own (freed on the way out): the results of the last cape_map_union are not touched
    Buffer<double> a, b, frames, verts;
    Buffer<cape_plane_union> row;
    CAPE_HIP_TRY(a.alloc((size_t)n_a * 2));
    CAPE_HIP_TRY(b.alloc((size_t)n_b * 2));
    CAPE_HIP_TRY(frames.alloc(27));
    CAPE_HIP_TRY(verts.alloc((size_t)CAPE_MAP_MAX_RING * 2));
    CAPE_HIP_TRY(row.alloc(1));
    CAPE_HIP_TRY(hipMemcpy(a, ring_a, (size_t)n_a * 2 * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(b, ring_b, (size_t)n_b * 2 * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(frames, frames27 ? frames27 : kCanonical, 27 * sizeof(double), hipMemcpyHostToDevice));
    cape::RingUnionParams p{};
    p.ringA = reinterpret_cast<const double2*>(a.get());
    p.ringB = reinterpret_cast<const double2*>(b.get());
    p.nA = n_a;
    p.nB = n_b;
    p.frames27 = frames;
    p.row = row;
    p.vertices = reinterpret_cast<double2*>(verts.get());
    CAPE_HIP_TRY(cape::launch_ring_union(p, nullptr));
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(copy_out(row_out, row, 0, 1));
    const size_t n = row_out->vertex_count <= CAPE_MAP_MAX_RING ? row_out->vertex_count : 0;
    CAPE_HIP_TRY(copy_out(vertices_out, verts, 0, n * 2));
    return CAPE_OK;
}

// cape_debug_polygon_union and cape_debug_polygon_union_cut: the same arguments and buffers, the kernel of the mode
static int debug_polygon_union(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                               const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out, bool cut)
{
    static const double kCanonical[27] = {1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0};
    if (!h || !rings_a || !counts_a || !ring_b || !row_out || !rings_out || !vertices_out || n_rings_a < 1 || n_rings_a > 1 + CAPE_MAP_MAX_HOLES ||
        n_b < 3 || n_b > 4096)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument, n_rings_a outside [1, 1 + CAPE_MAP_MAX_HOLES] or a ring of fewer than 3 / more than 4096 vertices");
    size_t n_a = 0;
    for (int32_t k = 0; k < n_rings_a; ++k)
    {
        if (counts_a[k] < 3 || counts_a[k] > 4096)
            return fail(CAPE_ERR_INVALID_ARGUMENT, "a ring of fewer than 3 / more than 4096 vertices");
        n_a += (size_t)counts_a[k];
    }
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    // a one-pair launch over buffers of its own (freed on the way out): the results of the last union call are not touched
    Buffer<double> a, b, frames, verts;
    Buffer<int32_t> counts;
    Buffer<cape_plane_union> row;
    Buffer<cape_plane_union_rings> ringRow;
    CAPE_HIP_TRY(a.alloc(n_a * 2));
    CAPE_HIP_TRY(counts.alloc((size_t)n_rings_a));
    CAPE_HIP_TRY(b.alloc((size_t)n_b * 2));
    CAPE_HIP_TRY(frames.alloc(27));
    CAPE_HIP_TRY(verts.alloc((size_t)CAPE_MAP_UNION_FRAME_VERTICES * 2));
    CAPE_HIP_TRY(row.alloc(1));
    CAPE_HIP_TRY(ringRow.alloc(1));
    CAPE_HIP_TRY(hipMemcpy(a, rings_a, n_a * 2 * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(counts, counts_a, (size_t)n_rings_a * sizeof(int32_t), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(b, ring_b, (size_t)n_b * 2 * sizeof(double), hipMemcpyHostToDevice));
    CAPE_HIP_TRY(hipMemcpy(frames, frames27 ? frames27 : kCanonical, 27 * sizeof(double), hipMemcpyHostToDevice));
    cape::PolygonUnionParams p{};
    p.ringsA = reinterpret_cast<const double2*>(a.get());
    p.countsA = counts;
    p.nRingsA = n_rings_a;
    p.ringB = reinterpret_cast<const double2*>(b.get());
    p.nB = n_b;
    p.frames27 = frames;
    p.row = row;
    p.ringRow = ringRow;
    p.vertices = reinterpret_cast<double2*>(verts.get());
    CAPE_HIP_TRY(cut ? cape::launch_polygon_union_cut(p, nullptr) : cape::launch_polygon_union(p, nullptr));
    CAPE_HIP_TRY(hipDeviceSynchronize());
    CAPE_HIP_TRY(copy_out(row_out, row, 0, 1));
    CAPE_HIP_TRY(copy_out(rings_out, ringRow, 0, 1));
    size_t n = 0;
    for (uint32_t k = 0; k < rings_out->ring_count && k < 1 + CAPE_MAP_MAX_HOLES; ++k)
        n += rings_out->vertex_count[k];
    CAPE_HIP_TRY(copy_out(vertices_out, verts, 0, (n <= CAPE_MAP_UNION_FRAME_VERTICES ? n : 0) * 2));
    return CAPE_OK;
}

int cape_debug_polygon_union(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b,
                             const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out)
{
    return debug_polygon_union(h, rings_a, counts_a, n_rings_a, ring_b, n_b, frames27, row_out, rings_out, vertices_out, false);
}

int cape_debug_polygon_union_cut(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b,
                                 int32_t n_b, const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out,
                                 double* vertices_out)
{
    return debug_polygon_union(h, rings_a, counts_a, n_rings_a, ring_b, n_b, frames27, row_out, rings_out, vertices_out, true);
}

} // extern "C"
