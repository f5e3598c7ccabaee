// C ABI, host side: depth rectification (N3), plane matching between consecutive frames (N2), the boundary polygons of the planes
// (N1) and the matches between them, carried frame included.  The map's calls: cape_api_map_match.hip, cape_api_map_update.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cape_api_map.h"

using namespace cape::abi;

namespace {

// the optional prev_to_cur of the two polygon matchers, n_frames x 16 doubles in the caller's memory order (entry 0 is read by a
// carried call only): the header promises that they are read before the call returns -- through the pinned twin.  *dev is their
// device copy, left alone where none are given
int upload_prev_to_cur(cape_handle_s::Buffer<double>& poses, PinnedTwin& twin, size_t maxBatch, int32_t n_frames, const double* prev_to_cur,
                       hipStream_t stream, const double** dev)
{
    if (!prev_to_cur)
        return CAPE_OK;
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
    CAPE_HIP_TRY(poses.ensure(maxBatch * 16));
    CAPE_HIP_TRY(twin.upload(poses, poseBytes, maxBatch * 16 * sizeof(double), stream, [&](void* stage) { std::memcpy(stage, prev_to_cur, poseBytes); }));
    *dev = poses;
    return CAPE_OK;
}

int match_polygons_impl(cape_handle h, int32_t n_frames, const double* prev_to_cur, uint32_t flags, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& P = h->poly;
    if (n_frames > P.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (flags & ~(uint32_t)(CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    const size_t B = (size_t)h->cfg.max_batch;
    const size_t pairCapacity = B * CAPE_MATCH_MAX_PLANES * CAPE_MATCH_MAX_PLANES;
    CAPE_HIP_TRY(P.matches.ensure(B));
    CAPE_HIP_TRY(P.lists.ensure(64 + 4 * pairCapacity));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::MatchPolygonParams p;
    if (const int rc = upload_prev_to_cur(P.poses, P.posesTwin, B, n_frames, prev_to_cur, stream, &p.poses); rc != CAPE_OK)
        return rc;
    p.records = h->res.records;
    p.polygons = P.polygons;
    p.vertices = reinterpret_cast<const double2*>(P.vertices.get());
    p.matches = P.matches;
    p.listCounts = P.lists;
    p.pairLists = P.lists + 64;
    p.pairCapacity = pairCapacity;
    p.computeUnits = h->computeUnits;
    p.ldsLimitBytes = h->ldsLimit;
    p.boundaryCapacity = h->boundaryCap;
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match_polygons(p, n_frames, stream));
    P.matchFrames = n_frames;
    return CAPE_OK;
}

// entries of its work list at most (112 MB of buffers): the GATED pairs of a call, a few per kept plane -- 1 024 per frame of a
// 4 096-frame batch, where a frame of 128 planes on a checkerboard of facets gates some hundreds; a frame beyond it is flagged
constexpr size_t kWideWorkMax = (size_t)1 << 22;
// the carried frame's buffers as the kernels take them.  A served ring has at most min(kPolyMaxPoints, boundary capacity) vertices
// (boundary points of its record's slab; a plane of more is CAPE_POLY_OVERFLOW and has no ring) and at most 128 planes are carried:
// the vertex store holds every frame the matcher would serve
int carry_ring_capacity(const cape_handle_s* h) { return std::min(cape::kPolyMaxPoints, h->boundaryCap); }
cape::MatchCarry bind_carry(const cape_handle_s* h)
{
    const auto& K = h->carry;
    cape::MatchCarry c;
    c.info = K.info;
    c.planes = K.planes;
    c.segs = K.segs;
    c.polygons = K.polygons;
    c.vertices = reinterpret_cast<double2*>(K.vertices.get());
    c.ringCapacity = carry_ring_capacity(h);
    return c;
}

} // namespace

extern "C" {

int cape_rectify_depth(cape_handle h, const float* depth_dev, float* rectified_dev, int32_t n_frames,
                       const double* cam2_to_cam1, void* stream_)
{
    if (!h || !depth_dev || !rectified_dev || !cam2_to_cam1 || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or negative frame count");
    if (n_frames == 0)
        return CAPE_OK;
    if (depth_dev == rectified_dev)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "rectify_depth is not in-place");
    CAPE_ON_DEVICE(h);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    // (a device-wide synchronisation before the smaller buffer is freed)
    CAPE_HIP_TRY(h->rectFlags.grow(2 * (size_t)n_frames + 1, [] { return hipDeviceSynchronize(); }));
    cape::RectifyParams p;
    p.in = depth_dev;
    p.out = rectified_dev;
    p.ldsLimitBytes = h->ldsLimit;
    p.frameFlag = h->rectFlags;
    p.flagged = h->rectFlags + h->rectFlags.size() / 2;
    {
        const char* eb = std::getenv("CAPE_RECTIFY_BAND");
        p.bandRows = eb ? std::atoi(eb) : 0;
    }
    p.W = h->cfg.width;
    p.H = h->cfg.height;
    p.xpre = h->xpre;
    p.ypre = h->ypre;
    for (int i = 0; i < 12; ++i)
        p.T[i] = cam2_to_cam1[i];
    p.fx = h->cfg.fx;
    p.fy = h->cfg.fy;
    p.cx = h->cfg.cx;
    p.cy = h->cfg.cy;
    {
        // Which source rows can land in a band of target rows?  The row displacement of this rig, sampled over the image and over
        // depths from 0.3 m to 10 m (plain doubles: a prediction, the kernel checks every pixel and flags what escapes it).
        double lo = 0.0, hi = 0.0;
        bool any = false;
        const double zs[] = {300.0, 600.0, 1200.0, 2500.0, 5000.0, 10000.0};
        for (int ry = 0; ry <= 4; ++ry)
            for (int rx = 0; rx <= 4; ++rx)
                for (double z : zs)
                {
                    const double row = (h->cfg.height - 1) * ry / 4.0, col = (h->cfg.width - 1) * rx / 4.0;
                    const double x = (col - h->cfg.cx) / h->cfg.fx * z, y = (row - h->cfg.cy) / h->cfg.fy * z;
                    const double q1 = p.T[4] * x + p.T[5] * y + p.T[6] * z + p.T[7], q2 = p.T[8] * x + p.T[9] * y + p.T[10] * z + p.T[11];
                    if (!(q2 > 0))
                        continue;
                    const double d = (h->cfg.fy * q1 / q2 + h->cfg.cy) - row;
                    lo = any ? std::min(lo, d) : d;
                    hi = any ? std::max(hi, d) : d;
                    any = true;
                }
        const char* em = std::getenv("CAPE_RECTIFY_MARGIN");
        const int margin = em ? std::atoi(em) : 2;
        const double cap = 4.0 * h->cfg.height; // (a degenerate rig: everything escapes, the general kernels take over)
        p.shiftLo = (int)std::floor(std::max(-cap, std::min(cap, lo))) - margin;
        p.shiftHi = (int)std::ceil(std::max(-cap, std::min(cap, hi))) + margin;
    }
    CAPE_HIP_TRY(cape::launch_rectify(p, n_frames, h->computeUnits, stream));
    return CAPE_OK;
}

int cape_rectify_depth_host(cape_handle h, const float* depth_host, float* rectified_host, int32_t n_frames,
                            const double* cam2_to_cam1)
{
    if (!h || !depth_host || !rectified_host || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument or negative frame count");
    CAPE_ON_DEVICE(h);
    const size_t n = (size_t)n_frames * h->cfg.width * h->cfg.height;
    Buffer<float> din, dout;
    CAPE_HIP_TRY(din.alloc(n));
    if (dout.alloc(n) != hipSuccess)
        return fail(CAPE_ERR_HIP, "hipMalloc failed");
    if (hipMemcpy(din, depth_host, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(CAPE_ERR_HIP, "H2D copy failed");
    if (const int rc = cape_rectify_depth(h, din, dout, n_frames, cam2_to_cam1, nullptr); rc != CAPE_OK)
        return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess)
        return fail(CAPE_ERR_HIP, "rectify kernels failed");
    if (copy_out(rectified_host, dout, 0, n) != hipSuccess)
        return fail(CAPE_ERR_HIP, "D2H copy failed");
    return CAPE_OK;
}

int cape_match_consecutive(cape_handle h, int32_t n_frames, uint32_t flags, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    if (flags & ~(uint32_t)(CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    StreamScope streamScope(h, static_cast<hipStream_t>(stream_));
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    CAPE_HIP_TRY(h->matches.ensure((size_t)h->cfg.max_batch));
    cape::MatchParams p;
    p.records = h->res.records;
    p.plane_labels = h->res.planeLabels;
    p.matches = h->matches;
    p.cells = h->cells;
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match(p, n_frames, static_cast<hipStream_t>(stream_)));
    return CAPE_OK;
}

int cape_device_matches(cape_handle h, void** matches)
{
    if (!h || !matches)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->matches)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "cape_match_consecutive has not run");
    *matches = h->matches;
    return CAPE_OK;
}

int cape_copy_matches(cape_handle h, int32_t n_frames, cape_frame_match* out)
{
    if (!h || !out || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    if (!h->matches)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "cape_match_consecutive has not run");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(sync_handle(h));
    CAPE_HIP_TRY(copy_out(out, h->matches, 0, (size_t)n_frames));
    return CAPE_OK;
}

int cape_build_polygons(cape_handle h, int32_t n_frames, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->res.lastFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the last cape_extract batch");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    auto& P = h->poly;
    const size_t B = (size_t)h->cfg.max_batch + (size_t)h->chain.spillRecords; // a polygon row / vertex slab per record, spill pool included
    // the records and boundary points of a few-frame handle live in pinned host memory (the kernel reads them over PCIe); the
    // polygons follow them there
    if (!P.polygons)
        CAPE_HIP_TRY(alloc_result(P.polygons, B * CAPE_MAX_PLANES, h->resultsOnHost));
    if (!P.vertices)
        CAPE_HIP_TRY(alloc_result(P.vertices, B * (size_t)h->boundaryCap * 2, h->resultsOnHost));
    CAPE_HIP_TRY(P.ladder.ensure(cape::polygon_scratch_bytes(B, h->boundaryCap)));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::PolygonParams p;
    cape::polygon_bind_scratch(p, P.ladder, B, h->boundaryCap);
    p.computeUnits = h->computeUnits;
    p.originInCentroid = 0;
    p.records = h->res.records;
    p.boundary = h->res.boundary;
    p.polygons = P.polygons;
    p.vertices = reinterpret_cast<double2*>(P.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.prof = h->debugCycles;
    p.poolBase = h->cfg.max_batch;
    p.poolCapacity = h->chain.spillRecords;
    p.poolUsed = h->chain.spillCounters;
#ifdef CAPE_POLY_PROFILE
    CAPE_HIP_TRY(hipMemsetAsync(h->debugCycles, 0, (size_t)n_frames * cape::kProfileSlots * 8, stream));
    CAPE_HIP_TRY(hipMemsetAsync(h->debugCycles + 6, 0xFF, 2 * 8, stream)); // the two minima of the task kernel's timeline
#endif
    h->res.doneArmed = false; // the chain's completion word was written before this kernel: results are waited for the slow way
    h->measure.frames = 0; // (the measurements index the polygons this call replaces)
    invalidate_frame_results(h);
    CAPE_HIP_TRY(cape::launch_polygons(p, n_frames, stream));
    P.frames = n_frames;
    return CAPE_OK;
}

int cape_match_polygons(cape_handle h, int32_t n_frames, uint32_t flags, void* stream_)
{
    return match_polygons_impl(h, n_frames, nullptr, flags, stream_);
}

int cape_match_polygons_pose(cape_handle h, int32_t n_frames, const double* prev_to_cur, uint32_t flags, void* stream_)
{
    return match_polygons_impl(h, n_frames, prev_to_cur, flags, stream_);
}

int cape_copy_polygon_matches(cape_handle h, int32_t n_frames, cape_frame_match_exact* out)
{
    if (!h || !out || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    if (!h->poly.matches)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "cape_match_polygons has not run");
    if (n_frames > h->poly.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_match_polygons of the current batch");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(out, h->poly.matches, 0, (size_t)n_frames));
    return CAPE_OK;
}

int cape_match_polygons_wide(cape_handle h, int32_t n_frames, const double* prev_to_cur, uint32_t flags, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (flags & ~(uint32_t)(CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0 | CAPE_MATCH_MAP_AREAS | CAPE_MATCH_CARRY))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    const bool keepAreas = (flags & CAPE_MATCH_MAP_AREAS) != 0, carried = (flags & CAPE_MATCH_CARRY) != 0;
    if (carried && !h->carry.saved)
        return fail(CAPE_ERR_CAPACITY, "CAPE_MATCH_CARRY: no frame is carried (cape_match_carry_save first)");
    const size_t areaDoubles = (size_t)n_frames * WP * WP;
    if (keepAreas && areaDoubles * sizeof(double) > kMapAreasBudget)
        return fail(CAPE_ERR_CAPACITY, "the inter-area table of this call would exceed 1 GiB (fewer frames per call, or no CAPE_MATCH_MAP_AREAS)");
    auto& W = h->wide;
    W.matchFrames = 0;
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const size_t B = (size_t)h->cfg.max_batch;
    const size_t cap = std::min(B * WP * WP, kWideWorkMax);
    const MapWorkLayout lay = map_work_layout(h->cfg.max_batch, cap, 0); // (no map: no gate masks)
    CAPE_HIP_TRY(W.frames.ensure(B));
    CAPE_HIP_TRY(W.match.ensure(3 * B * WP));
    CAPE_HIP_TRY(W.kept.ensure(B * WP));
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    CAPE_HIP_TRY(W.work.grow(lay.total, drain));
    if (keepAreas)
        CAPE_HIP_TRY(W.areas.grow(areaDoubles, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::MatchWideParams p{};
    if (const int rc = upload_prev_to_cur(W.poses, W.posesTwin, B, n_frames, prev_to_cur, stream, &p.poses); rc != CAPE_OK)
        return rc;
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.maxBatch = h->cfg.max_batch;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords;
    p.frames = W.frames;
    p.match = W.match;
    p.segPrev = W.match + B * WP;
    p.segCur = W.match + 2 * B * WP;
    p.areas = keepAreas ? W.areas.get() : nullptr;
    p.kept = W.kept;
    p.list = bind_pair_list(W.work, lay, cap);
    p.computeUnits = h->computeUnits;
    p.ldsLimitBytes = h->ldsLimit;
    if (carried)
        p.carry = bind_carry(h);
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match_wide(p, n_frames, stream));
    W.matchFrames = n_frames;
    W.matchAreas = keepAreas;
    return CAPE_OK;
}

int cape_copy_polygon_matches_wide(cape_handle h, int32_t n_frames, cape_frame_match_wide* frames, int32_t* match, int32_t* seg_prev,
                                   int32_t* seg_cur, double* inter_area)
{
    constexpr size_t WP = CAPE_MATCH_WIDE_MAX_PLANES;
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& W = h->wide;
    if (n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_match_polygons_wide of the current batch");
    if (inter_area && n_frames > 0 && !W.matchAreas)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_match_polygons_wide did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t B = (size_t)h->cfg.max_batch, n = (size_t)n_frames * WP;
    CAPE_HIP_TRY(copy_out(frames, W.frames, 0, (size_t)n_frames));
    CAPE_HIP_TRY(copy_out(match, W.match, 0, n));
    CAPE_HIP_TRY(copy_out(seg_prev, W.match, B * WP, n));
    CAPE_HIP_TRY(copy_out(seg_cur, W.match, 2 * B * WP, n));
    CAPE_HIP_TRY(copy_out(inter_area, W.areas, 0, n * WP));
    return CAPE_OK;
}

int cape_match_carry_save(cape_handle h, int32_t frame, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_WIDE_MAX_PLANES;
    if (!h || frame < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame");
    if (frame >= h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "the frame is not covered by the last cape_build_polygons of the current batch");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    auto& K = h->carry;
    CAPE_HIP_TRY(K.info.ensure(1));
    CAPE_HIP_TRY(K.planes.ensure(WP * 4));
    CAPE_HIP_TRY(K.segs.ensure(WP));
    CAPE_HIP_TRY(K.polygons.ensure(WP));
    CAPE_HIP_TRY(K.vertices.ensure(WP * (size_t)carry_ring_capacity(h) * 2));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::CarrySaveParams p{};
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.maxBatch = h->cfg.max_batch;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords;
    p.frame = frame;
    p.carry = bind_carry(h);
    K.saved = false; // (a launch that fails leaves no carry behind rather than half of one)
    CAPE_HIP_TRY(cape::launch_carry_save(p, stream));
    K.saved = true;
    return CAPE_OK;
}

int cape_match_carry_clear(cape_handle h)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    h->carry.saved = false;
    return CAPE_OK;
}

int cape_match_carry_info(cape_handle h, cape_match_carry_info_t* out)
{
    if (!h || !out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null argument");
    *out = cape_match_carry_info_t{};
    if (!h->carry.saved)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(out, h->carry.info, 0, 1));
    out->valid = 1;
    return CAPE_OK;
}

int cape_device_polygons(cape_handle h, cape_polygon** polygons, double** vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (h->poly.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no polygons of the current batch: cape_build_polygons has not run since the last cape_extract");
    if (polygons)
        *polygons = h->poly.polygons;
    if (vertices)
        *vertices = h->poly.vertices;
    return CAPE_OK;
}

int cape_copy_polygons(cape_handle h, int32_t n_frames, cape_polygon* polygons, double* vertices)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& P = h->poly;
    if (!P.polygons)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no polygons have been built yet");
    if (n_frames > P.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons of the current batch");
    CAPE_ON_DEVICE(h);
    if (const int rc = settle_results(h); rc != CAPE_OK)
        return rc;
    const size_t n = (size_t)n_frames;
    CAPE_HIP_TRY(copy_out(polygons, P.polygons, 0, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(vertices, P.vertices, 0, n * (size_t)h->boundaryCap * 2));
    return CAPE_OK;
}

int cape_copy_spill_polygons(cape_handle h, int32_t first, int32_t count, cape_polygon* polygons, double* vertices)
{
    if (!h || first < 0 || count < 0 || first > h->chain.spillRecords || count > h->chain.spillRecords - first)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / spill record range");
    const auto& P = h->poly;
    if (!P.polygons || P.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no cape_build_polygons has run on the current batch");
    CAPE_ON_DEVICE(h);
    if (const int rc = settle_results(h); rc != CAPE_OK)
        return rc;
    const size_t at = (size_t)h->cfg.max_batch + (size_t)first, n = (size_t)count, cap = (size_t)h->boundaryCap;
    CAPE_HIP_TRY(copy_out(polygons, P.polygons, at * CAPE_MAX_PLANES, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(vertices, P.vertices, at * cap * 2, n * cap * 2));
    return CAPE_OK;
}

} // extern "C"
