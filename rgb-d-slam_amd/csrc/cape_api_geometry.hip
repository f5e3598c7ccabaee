// C ABI, host side: depth rectification (N3), plane matching between consecutive frames and against a persistent map (N2), the
// boundary polygons of the planes (N1) and the matches between them.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "cape_handle.h"

using namespace cape::abi;

namespace {

// parameters::matching (src/parameters.hpp:89-95), evaluated on the host like the reference's function-local statics
template <typename Params> void set_match_thresholds(Params& p, uint32_t flags)
{
    p.flags = flags;
    p.minCosAngle = std::abs(std::cos(20.0 * M_PI / 180.0));
    p.maxDistance = 100.0;
    const double planeMinimalOverlap = static_cast<double>(0.4f);
    p.minOverlap = (flags & CAPE_MATCH_ADVANCED) ? planeMinimalOverlap / 2 : planeMinimalOverlap;
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
    if (prev_to_cur)
    {
        // the poses travel to the device in the caller's memory order: n_frames x 16 doubles (entry 0 is never read).  The
        // header promises that prev_to_cur is read before the call returns: through the pinned twin
        const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
        CAPE_HIP_TRY(P.poses.ensure(B * 16));
        CAPE_HIP_TRY(P.posesTwin.upload(P.poses, poseBytes, B * 16 * sizeof(double), stream,
                                        [&](void* stage) { std::memcpy(stage, prev_to_cur, poseBytes); }));
        p.poses = P.poses;
    }
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

// the work buffers of cape_match_map, one allocation: counters, per-frame ranges, the gate masks (maskWords 64-bit words per map
// plane: one for frames of up to 64 kept planes, two for cape_match_map_wide's 128), the work list, its areas, the tier lists
struct MapWorkLayout
{
    size_t counts, ranges, masks, work, area, tiers, total;
};
MapWorkLayout map_work_layout(int maxBatch, size_t cap, int maskWords = 1)
{
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    MapWorkLayout l;
    l.counts = 0;
    l.ranges = up(16 * sizeof(unsigned));
    l.masks = l.ranges + up((size_t)maxBatch * sizeof(uint2));
    l.work = l.masks + up((size_t)maxBatch * CAPE_MAP_MAX_PLANES * maskWords * sizeof(unsigned long long));
    l.area = l.work + up(cap * sizeof(unsigned long long));
    l.tiers = l.area + up(cap * sizeof(double));
    l.total = l.tiers + up(3 * cap * sizeof(unsigned));
    return l;
}
constexpr size_t kMapWorkMax = (size_t)1 << 24;     // entries of the work list at most (448 MB of buffers)
constexpr size_t kMapAreasBudget = (size_t)1 << 30; // bytes of the dense inter-area table at most
// what cape_match_map and cape_match_map_shards pass to their kernels alike: the uploaded map, the work buffers inside `work`, the
// device's limits
void bind_map_call(cape::MatchMapParams& p, const cape_handle_s* h, unsigned char* work, const MapWorkLayout& lay, size_t cap)
{
    const auto& map = h->map;
    p.mapPlanes = map.planes;
    p.mapRings = map.rings;
    p.mapVertices = reinterpret_cast<const double2*>(map.vertices.get());
    p.nMap = map.n;
    p.skipWords = (map.n + 31) / 32;
    p.counts = reinterpret_cast<unsigned*>(work + lay.counts);
    p.frameRange = reinterpret_cast<uint2*>(work + lay.ranges);
    p.gateMasks = reinterpret_cast<unsigned long long*>(work + lay.masks);
    p.work = reinterpret_cast<unsigned long long*>(work + lay.work);
    p.workArea = reinterpret_cast<double*>(work + lay.area);
    p.tierLists = reinterpret_cast<unsigned*>(work + lay.tiers);
    p.workCapacity = cap;
    p.computeUnits = h->computeUnits;
    p.ldsLimitBytes = h->ldsLimit;
}
// the pinned twin's bytes of such a call: n x 16 doubles (the identity where no poses are given: the statements stay those of a pose),
// then the skip words
void fill_poses(void* stage, int n, const double* world_to_camera, size_t poseBytes, const uint32_t* skip, size_t skipBytes)
{
    double* pose = static_cast<double*>(stage);
    if (world_to_camera)
        std::memcpy(pose, world_to_camera, poseBytes);
    else
        for (int f = 0; f < n; ++f)
            for (int k = 0; k < 16; ++k)
                pose[16 * f + k] = (k % 5 == 0) ? 1.0 : 0.0;
    if (skipBytes)
        std::memcpy(static_cast<unsigned char*>(stage) + poseBytes, skip, skipBytes);
}
// the work buffers of cape_map_visibility, one allocation: counters, the work list, the tier lists
struct VisibilityWorkLayout
{
    size_t counts, work, tiers, total;
};
VisibilityWorkLayout visibility_work_layout(size_t cap)
{
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    VisibilityWorkLayout l;
    l.counts = 0;
    l.work = up(16 * sizeof(unsigned));
    l.tiers = l.work + up(cap * sizeof(unsigned long long));
    l.total = l.tiers + up(3 * cap * sizeof(unsigned));
    return l;
}
constexpr size_t kVisibilityWorkBudget = (size_t)1 << 30; // bytes of the visibility work list at most
// what the visibility kernels read of the handle, for cape_map_visibility and cape_map_step_visible: the front map, the camera, the device
cape::MapVisibilityParams bind_map_visibility(const cape_handle_s* h)
{
    cape::MapVisibilityParams p{};
    p.mapPlanes = h->map.planes;
    p.mapRings = h->map.rings;
    p.mapVertices = reinterpret_cast<const double2*>(h->map.vertices.get());
    p.nMap = h->map.n;
    p.skipWords = (h->map.n + 31) / 32;
    p.computeUnits = h->computeUnits;
    p.ldsLimitBytes = h->ldsLimit;
    p.width = h->cfg.width;
    p.height = h->cfg.height;
    p.fx = h->cfg.fx;
    p.fy = h->cfg.fy;
    p.cx = h->cfg.cx;
    p.cy = h->cfg.cy;
    return p;
}
// CAPE_MATCH_MAP_DEVICE_SKIP: the skip words of the last cape_map_visibility for a match call over n frames (or slots), or the
// reason there are none
int device_skip_words(const cape_handle_s* h, int n, const uint32_t* skip, const uint32_t** words)
{
    const auto& V = h->visibility;
    if (skip)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_MATCH_MAP_DEVICE_SKIP takes the skip words of cape_map_visibility: skip must be NULL");
    if (V.frames <= 0 || V.n != h->map.n)
        return fail(CAPE_ERR_CAPACITY, "CAPE_MATCH_MAP_DEVICE_SKIP: no cape_map_visibility has run since the last cape_map_upload");
    if (n > V.frames)
        return fail(CAPE_ERR_CAPACITY, "CAPE_MATCH_MAP_DEVICE_SKIP: the last cape_map_visibility covered fewer frames than this call");
    *words = V.skip;
    return CAPE_OK;
}
// the work buffers of cape_match_polygons_wide, one allocation: counters, per-frame ranges, the work list, its areas, the tier lists
struct WideWorkLayout
{
    size_t counts, ranges, work, area, tiers, total;
};
WideWorkLayout wide_work_layout(int maxBatch, size_t cap)
{
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    WideWorkLayout l;
    l.counts = 0;
    l.ranges = up(16 * sizeof(unsigned));
    l.work = l.ranges + up((size_t)maxBatch * sizeof(uint2));
    l.area = l.work + up(cap * sizeof(unsigned long long));
    l.tiers = l.area + up(cap * sizeof(double));
    l.total = l.tiers + up(3 * cap * sizeof(unsigned));
    return l;
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
constexpr uint32_t kMatchMapFlags = CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0 | CAPE_MATCH_MAP_AREAS | CAPE_MATCH_MAP_DEVICE_SKIP;
bool unit_norm(const double* v) // double_equal(norm, 1) as to_camera_space requires (polygon_coordinates.cpp:144-151)
{
    return std::abs(std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) - 1.0) <= std::numeric_limits<double>::epsilon();
}
double ring_area_signed_host(const double* r, uint32_t n) // the host class's shoelace, same order
{
    double s = 0;
    for (uint32_t i = 0, j = n - 1; i < n; j = i++)
        s += (r[2 * j] * r[2 * i + 1] - r[2 * i] * r[2 * j + 1]);
    return 0.5 * s;
}

// the results of the last cape_map_kalman still describe the current batch, match and measurements (a cape_extract clears the latter
// two; every other call that replaces an input clears kalmanFrames itself)
bool kalman_results_live(const cape_handle_s* h)
{
    const auto& K = h->kalman;
    return K.kalmanFrames > 0 && h->mapWide.matchFrames >= K.kalmanFrames && h->measure.frames >= K.kalmanFrames;
}

// ... and those of the last cape_map_union the Kalman results they were made from
bool union_results_live(const cape_handle_s* h)
{
    const auto& U = h->mapUnion;
    return U.unionFrames > 0 && kalman_results_live(h) && h->kalman.kalmanFrames >= U.unionFrames && U.kalmanRun == h->kalman.runs;
}

// The kernel parameters of the map update's calls, bound to the handle's buffers: cape_map_kalman, cape_map_union* and cape_map_commit
// run them on the first n frames of the batch-wide tables, cape_map_step on the one frame whose rows it has put at row 0 of them.
cape::MapKalmanParams bind_map_kalman(const cape_handle_s* h)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    const auto& K = h->kalman;
    const auto& W = h->mapWide;
    cape::MapKalmanParams p{};
    p.mapPlanes = h->map.planes;
    p.tracks = K.tracks;
    p.nMap = h->map.n;
    p.matchFrames = W.frames;
    p.match = W.match;
    p.mapOf = W.planes + (size_t)h->cfg.max_batch * WP;
    p.kept = W.kept;
    p.measurements = h->measure.rows;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows cape_map_measure allocated: a row of CAPE_MAX_PLANES per record)
    p.frames = K.frames;
    p.rows = K.rows;
    p.trackResults = K.trackResults;
    return p;
}
cape::MapUnionParams bind_map_union(const cape_handle_s* h)
{
    const auto& W = h->mapWide;
    const auto& M = h->measure;
    cape::MapUnionParams p{};
    p.mapPlanes = h->map.planes;
    p.mapRings = h->map.rings;
    p.mapVertices = reinterpret_cast<const double2*>(h->map.vertices.get());
    p.nMap = h->map.n;
    p.nMapRings = (unsigned)h->map.rings.size();
    p.nMapVertices = (unsigned long long)(h->map.vertices.size() / 2);
    p.matchFrames = W.frames;
    p.match = W.match;
    p.kept = W.kept;
    p.measurements = M.rows;
    p.worldVertices = reinterpret_cast<const double2*>(M.vertices.get());
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows and slabs cape_map_measure allocated: one per record)
    p.boundaryCapacity = h->boundaryCap;
    p.fusion = h->kalman.rows;
    p.rows = h->mapUnion.rows;
    p.vertices = reinterpret_cast<double2*>(h->mapUnion.vertices.get());
    return p;
}
// what a commit's destination set takes, to bounds the host knows: at most 128 appended planes of one ring each, a frame's slab of
// served rings, the world rings of the frame's chain
struct CommitBounds
{
    size_t planes, rings, vertices;
};
CommitBounds commit_bounds(const cape_handle_s* h)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    const size_t n = (size_t)h->map.n, cap = (size_t)h->boundaryCap;
    CommitBounds b;
    b.planes = std::min<size_t>(CAPE_MAP_MAX_PLANES, n + WP);
    b.rings = b.planes * (1 + CAPE_MAP_MAX_HOLES);
    b.vertices = (size_t)h->mapCommit.nVertices + SLAB + std::min<size_t>(WP * CAPE_MAP_MAX_RING, (size_t)(1 + h->chain.spillRecords) * cap);
    return b;
}
// workgroups of the commit's copy kernel: the planes of the new map at most
int commit_planes_bound(const cape_handle_s* h, const CommitBounds& b, uint32_t flags)
{
    return (int)std::min<size_t>(b.planes, (size_t)h->map.n + ((flags & CAPE_COMMIT_ADD_STAGED) ? (size_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES : 0));
}
// frame `frame` of the batch, whose rows are row `row` of the per-frame tables; withRings: the union's rings table belongs to its rows
cape::MapCommitParams bind_map_commit(const cape_handle_s* h, size_t row, int32_t frame, bool withRings, uint32_t flags, uint64_t nextId,
                                      const CommitBounds& b, cape_map_commit_result* header)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    const auto& map = h->map;
    const auto& K = h->kalman;
    const auto& U = h->mapUnion;
    const auto& X = h->mapCommit;
    cape::MapCommitParams p{};
    p.mapPlanes = map.planes;
    p.mapRings = map.rings;
    p.mapVertices = map.vertices;
    p.tracks = K.tracks;
    p.tags = X.tags;
    p.nMap = map.n;
    p.nMapRings = X.nRings;
    p.nMapVertices = X.nVertices;
    p.frame = frame;
    p.kalmanFrame = K.frames + row;
    p.trackResults = K.trackResults + row * (size_t)map.n;
    p.fusion = K.rows + row * WP;
    p.kept = h->mapWide.kept + row * WP;
    p.measurements = h->measure.rows;
    p.worldVertices = h->measure.vertices;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows and slabs cape_map_measure allocated: one per record)
    p.boundaryCapacity = h->boundaryCap;
    p.unionRows = U.rows + row * WP;
    p.ringRows = withRings ? h->mapUnionRings.rows + row * WP : nullptr;
    p.slab = U.vertices + row * SLAB * 2;
    p.flags = flags;
    p.nextId = nextId;
    p.outPlanes = X.planes;
    p.outRings = X.rings;
    p.outVertices = X.vertices;
    p.outTracks = X.tracks;
    p.outTags = X.tagsBack;
    p.planesCapacity = b.planes;
    p.ringsCapacity = b.rings;
    p.verticesCapacity = b.vertices;
    p.plan = X.plan;
    p.header = header;
    return p;
}
// the retired log's arrays take what `log` says, their contents kept (behind drain_handle: a call in flight may read them)
int grow_retired_log(cape_handle_s* h, const cape::MaintainLog& log)
{
    auto& R = h->mapMaintain;
    const auto drain = [h] { return drain_handle(h); };
    CAPE_HIP_TRY(R.planes.grow_keeping((size_t)log.planesCapacity, (size_t)R.nPlanes, drain));
    CAPE_HIP_TRY(R.tracks.grow_keeping((size_t)log.planesCapacity, (size_t)R.nPlanes, drain));
    CAPE_HIP_TRY(R.rings.grow_keeping((size_t)log.ringsCapacity, (size_t)R.nRings, drain));
    CAPE_HIP_TRY(R.vertices.grow_keeping((size_t)log.verticesCapacity * 2, (size_t)R.nVertices * 2, drain));
    return CAPE_OK;
}
// the map, its tracks and their ids change places with another buffer set (the commit's back set, or the step's third one)
void swap_map_set(cape_handle_s* h, cape_handle_s::Buffer<cape_map_plane>& planes, cape_handle_s::Buffer<cape_map_ring>& rings,
                  cape_handle_s::Buffer<double>& vertices, cape_handle_s::Buffer<cape::MapTrackState>& tracks,
                  cape_handle_s::Buffer<cape::MapTrackTag>& tags)
{
    h->map.planes.swap(planes);
    h->map.rings.swap(rings);
    h->map.vertices.swap(vertices);
    h->kalman.tracks.swap(tracks);
    h->mapCommit.tags.swap(tags);
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
    h->kalman.kalmanFrames = 0;
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
    const WideWorkLayout lay = wide_work_layout(h->cfg.max_batch, cap);
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
    if (prev_to_cur)
    {
        // through the pinned twin like cape_match_polygons_pose's: n_frames x 16 doubles in the caller's memory order, read before
        // the call returns (entry 0 is read by a carried call only)
        const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
        CAPE_HIP_TRY(W.poses.ensure(B * 16));
        CAPE_HIP_TRY(W.posesTwin.upload(W.poses, poseBytes, B * 16 * sizeof(double), stream,
                                        [&](void* stage) { std::memcpy(stage, prev_to_cur, poseBytes); }));
        p.poses = W.poses;
    }
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
    p.counts = reinterpret_cast<unsigned*>(W.work + lay.counts);
    p.frameRange = reinterpret_cast<uint2*>(W.work + lay.ranges);
    p.work = reinterpret_cast<unsigned long long*>(W.work + lay.work);
    p.workArea = reinterpret_cast<double*>(W.work + lay.area);
    p.tierLists = reinterpret_cast<unsigned*>(W.work + lay.tiers);
    p.workCapacity = cap;
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

int cape_map_upload(cape_handle h, const cape_map_plane* planes, int32_t n_planes, const cape_map_ring* rings, int32_t n_rings,
                    const double* vertices, int64_t n_vertices)
{
    if (!h || n_planes < 0 || n_rings < 0 || n_vertices < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative count");
    if (n_planes > CAPE_MAP_MAX_PLANES)
        return fail(CAPE_ERR_CAPACITY, "more map planes than CAPE_MAP_MAX_PLANES");
    if ((n_planes > 0 && !planes) || (n_rings > 0 && !rings) || (n_vertices > 0 && !vertices))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    // validation, then the rings re-oriented like the host class does and laid out plane by plane
    std::vector<cape_map_plane> P(planes, planes + n_planes);
    std::vector<cape_map_ring> R;
    std::vector<double> V;
    for (int32_t j = 0; j < n_planes; ++j)
    {
        cape_map_plane& M = P[j];
        if (M.ring_count == 0 || (uint64_t)M.ring_first + M.ring_count > (uint64_t)n_rings)
            return fail(CAPE_ERR_INVALID_ARGUMENT, "map plane without an outer ring or with rings outside the ring array");
        if (M.ring_count > 1u + CAPE_MAP_MAX_HOLES)
            return fail(CAPE_ERR_CAPACITY, "more holes than CAPE_MAP_MAX_HOLES");
        if (!unit_norm(M.normal) || !unit_norm(M.x_axis) || !unit_norm(M.y_axis))
            return fail(CAPE_ERR_INVALID_ARGUMENT, "map plane normal or polygon axis is not unit");
        const uint32_t first = (uint32_t)R.size();
        for (uint32_t k = 0; k < M.ring_count; ++k)
        {
            const cape_map_ring in = rings[M.ring_first + k];
            if (in.vertex_count < 3 || (uint64_t)in.vertex_offset + in.vertex_count > (uint64_t)n_vertices)
                return fail(CAPE_ERR_INVALID_ARGUMENT, "map ring of fewer than 3 vertices or outside the vertex array");
            if (in.vertex_count > CAPE_MAP_MAX_RING)
                return fail(CAPE_ERR_CAPACITY, "map ring longer than CAPE_MAP_MAX_RING (simplify the polygon first)");
            const size_t at = V.size();
            V.insert(V.end(), vertices + 2 * (size_t)in.vertex_offset, vertices + 2 * ((size_t)in.vertex_offset + in.vertex_count));
            // outer ring clockwise (OpenRing constructor), holes counter-clockwise (add_hole)
            const double sa = ring_area_signed_host(V.data() + at, in.vertex_count);
            if (k == 0 ? sa > 0 : sa < 0)
                for (uint32_t a = 0, b = in.vertex_count - 1; a < b; ++a, --b)
                {
                    std::swap(V[at + 2 * a], V[at + 2 * b]);
                    std::swap(V[at + 2 * a + 1], V[at + 2 * b + 1]);
                }
            R.push_back(cape_map_ring {(uint32_t)(at / 2), in.vertex_count});
        }
        M.ring_first = first;
    }
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h)); // a cape_match_map in flight still reads the old map
    auto& map = h->map;
    map.n = -1; // (no map until the copies are through)
    h->visibility.frames = 0; // (the words of the old map)
    h->mapStepVisible.n = -1;
    h->kalman.tracksN = -1;   // (its tracks, the wide match against it and what cape_map_kalman made of them)
    h->kalman.matchedThisMap = false;
    h->kalman.kalmanFrames = 0;
    const auto drained = [] { return hipSuccess; };
    CAPE_HIP_TRY(map.planes.grow(P.size(), drained));
    CAPE_HIP_TRY(map.rings.grow(R.size(), drained));
    CAPE_HIP_TRY(map.vertices.grow(V.size(), drained));
    if (!P.empty())
    {
        CAPE_HIP_TRY(hipMemcpy(map.planes, P.data(), P.size() * sizeof(cape_map_plane), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(map.rings, R.data(), R.size() * sizeof(cape_map_ring), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(map.vertices, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    map.n = n_planes;
    h->mapCommit.nRings = (int)R.size(); // (cape_map_info / cape_map_download / cape_map_commit: what the ring and vertex buffers hold)
    h->mapCommit.nVertices = (long long)(V.size() / 2);
    return CAPE_OK;
}

int cape_match_map(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& map = h->map;
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (flags & ~kMatchMapFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    const bool keepAreas = (flags & CAPE_MATCH_MAP_AREAS) != 0;
    const size_t areaDoubles = (size_t)n_frames * map.n * CAPE_MAX_PLANES;
    if (keepAreas && areaDoubles * sizeof(double) > kMapAreasBudget)
        return fail(CAPE_ERR_CAPACITY, "the inter-area table of this call would exceed 1 GiB (fewer frames per call, or no CAPE_MATCH_MAP_AREAS)");
    map.matchFrames = 0;
    const uint32_t* deviceSkip = nullptr;
    if (flags & CAPE_MATCH_MAP_DEVICE_SKIP)
        if (const int rc = device_skip_words(h, n_frames, skip, &deviceSkip); rc != CAPE_OK)
            return rc;
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    const int B = h->cfg.max_batch;
    const int skipWords = (map.n + 31) / 32;
    const size_t poseCapacity = (size_t)B * 16 * sizeof(double) + (size_t)B * (CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t);
    const size_t cap = std::min((size_t)B * (size_t)std::max(map.n, 1) * CAPE_MAX_PLANES, kMapWorkMax);
    const MapWorkLayout lay = map_work_layout(B, cap);
    CAPE_HIP_TRY(map.frames.ensure((size_t)B));
    CAPE_HIP_TRY(map.match.ensure((size_t)B * CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(map.poses.ensure(poseCapacity));
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    CAPE_HIP_TRY(map.work.grow(lay.total, drain));
    if (keepAreas)
        CAPE_HIP_TRY(map.areas.grow(areaDoubles, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    // the poses, then the skip bits, travel through the pinned twin like cape_match_polygons_pose's: n_frames x 16 doubles, then
    // n_frames x skipWords words
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
    const size_t skipBytes = skip ? (size_t)n_frames * skipWords * sizeof(uint32_t) : 0;
    CAPE_HIP_TRY(map.posesTwin.upload(map.poses, poseBytes + skipBytes, poseCapacity, stream,
                                      [&](void* stage) { fill_poses(stage, n_frames, world_to_camera, poseBytes, skip, skipBytes); }));
    cape::MatchMapParams p;
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    bind_map_call(p, h, map.work, lay, cap);
    p.poses = reinterpret_cast<const double*>(map.poses.get());
    p.skip = deviceSkip ? deviceSkip : skipBytes ? reinterpret_cast<const uint32_t*>(map.poses + poseBytes) : nullptr;
    p.frames = map.frames;
    p.match = map.match;
    p.areas = keepAreas ? map.areas.get() : nullptr;
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match_map(p, n_frames, stream));
    map.matchFrames = n_frames;
    h->lastMapMatcher = cape_handle_s::kMapMatchRecords;
    map.matchN = map.n;
    map.matchAreas = keepAreas;
    return CAPE_OK;
}

int cape_copy_map_matches(cape_handle h, int32_t n_frames, cape_frame_map_match* frames, int32_t* match, double* inter_area)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& map = h->map;
    if (n_frames > map.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_match_map of the current batch");
    if (inter_area && n_frames > 0 && !map.matchAreas)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_match_map did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)n_frames * map.matchN;
    CAPE_HIP_TRY(copy_out(frames, map.frames, 0, (size_t)n_frames));
    CAPE_HIP_TRY(copy_out(match, map.match, 0, n));
    CAPE_HIP_TRY(copy_out(inter_area, map.areas, 0, n * CAPE_MAX_PLANES));
    return CAPE_OK;
}

int cape_match_map_wide(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    const auto& map = h->map;
    auto& W = h->mapWide;
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (flags & ~kMatchMapFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    const bool keepAreas = (flags & CAPE_MATCH_MAP_AREAS) != 0;
    const size_t areaDoubles = (size_t)n_frames * map.n * WP;
    if (keepAreas && areaDoubles * sizeof(double) > kMapAreasBudget)
        return fail(CAPE_ERR_CAPACITY, "the inter-area table of this call would exceed 1 GiB (fewer frames per call, or no CAPE_MATCH_MAP_AREAS)");
    W.matchFrames = 0;
    h->kalman.kalmanFrames = 0; // (cape_map_kalman's results belong to the match this call replaces)
    const uint32_t* deviceSkip = nullptr;
    if (flags & CAPE_MATCH_MAP_DEVICE_SKIP)
        if (const int rc = device_skip_words(h, n_frames, skip, &deviceSkip); rc != CAPE_OK)
            return rc;
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const int B = h->cfg.max_batch;
    const int skipWords = (map.n + 31) / 32;
    const size_t poseCapacity = (size_t)B * 16 * sizeof(double) + (size_t)B * (CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t);
    const size_t cap = std::min((size_t)B * (size_t)std::max(map.n, 1) * WP, kMapWorkMax);
    const MapWorkLayout lay = map_work_layout(B, cap, 2);
    CAPE_HIP_TRY(W.frames.ensure((size_t)B));
    CAPE_HIP_TRY(W.match.ensure((size_t)B * CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(W.planes.ensure(2 * (size_t)B * WP));
    CAPE_HIP_TRY(W.kept.ensure((size_t)B * WP));
    CAPE_HIP_TRY(W.poses.ensure(poseCapacity));
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    CAPE_HIP_TRY(W.work.grow(lay.total, drain));
    if (keepAreas)
        CAPE_HIP_TRY(W.areas.grow(areaDoubles, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    // the poses, then the skip bits, through the pinned twin as in cape_match_map
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
    const size_t skipBytes = skip ? (size_t)n_frames * skipWords * sizeof(uint32_t) : 0;
    CAPE_HIP_TRY(W.posesTwin.upload(W.poses, poseBytes + skipBytes, poseCapacity, stream,
                                    [&](void* stage) { fill_poses(stage, n_frames, world_to_camera, poseBytes, skip, skipBytes); }));
    cape::MatchMapParams p;
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.maxBatch = B;
    p.nRecords = B + h->chain.spillRecords;
    bind_map_call(p, h, W.work, lay, cap);
    p.poses = reinterpret_cast<const double*>(W.poses.get());
    p.skip = deviceSkip ? deviceSkip : skipBytes ? reinterpret_cast<const uint32_t*>(W.poses + poseBytes) : nullptr;
    p.frames = nullptr;
    p.framesWide = W.frames;
    p.match = W.match;
    p.segCur = W.planes;
    p.mapOf = W.planes + (size_t)B * WP;
    p.keptIndex = W.kept;
    p.areas = keepAreas ? W.areas.get() : nullptr;
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match_map_wide(p, n_frames, stream));
    W.matchFrames = n_frames;
    h->lastMapMatcher = cape_handle_s::kMapMatchWide;
    W.matchN = map.n;
    W.matchAreas = keepAreas;
    h->kalman.matchedThisMap = true;
    return CAPE_OK;
}

int cape_copy_map_matches_wide(cape_handle h, int32_t n_frames, cape_frame_map_match_wide* frames, int32_t* match, int32_t* seg_cur,
                               int32_t* map_of, double* inter_area)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& W = h->mapWide;
    if (n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_match_map_wide of the current batch");
    if (inter_area && n_frames > 0 && !W.matchAreas)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_match_map_wide did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t B = (size_t)h->cfg.max_batch, n = (size_t)n_frames * W.matchN;
    CAPE_HIP_TRY(copy_out(frames, W.frames, 0, (size_t)n_frames));
    CAPE_HIP_TRY(copy_out(match, W.match, 0, n));
    CAPE_HIP_TRY(copy_out(seg_cur, W.planes, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(map_of, W.planes, B * WP, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(inter_area, W.areas, 0, n * WP));
    return CAPE_OK;
}

int cape_match_map_shards(cape_handle h, const void* shards_dev, int32_t n_shards, const cape_gather_layout* layout,
                          const cape_gather_polygon_layout* polygon_layout, const double* world_to_camera, const uint32_t* skip,
                          uint32_t flags, void* stream_)
{
    if (!h || !shards_dev || !layout || !polygon_layout || n_shards < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, shards or layout, or fewer than one shard");
    if (h->map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (flags & ~kMatchMapFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    // the sections the kernels read lie inside one shard, on 16-byte boundaries and one behind the other in the order the pack writes
    // them (the shards follow each other at bytes_per_rank)
    const cape_gather_layout& L = *layout;
    const cape_gather_polygon_layout& PL = *polygon_layout;
    uint64_t end = 0; // of the sections accepted so far
    const auto section_fits = [&](uint64_t offset, int64_t count, uint64_t size) {
        if (offset % 16 != 0 || count < 0 || offset < end || offset > L.bytes_per_rank || (uint64_t)count > (L.bytes_per_rank - offset) / size)
            return false;
        end = offset + (uint64_t)count * size;
        return true;
    };
    if (L.bytes_per_rank % 16 != 0 || reinterpret_cast<uintptr_t>(shards_dev) % 16 != 0 || L.frames_capacity < 1 || L.cells < 0 ||
        PL.polygons_capacity != L.planes_capacity || !section_fits(0, 1, sizeof(cape_packed_header)) ||
        !section_fits(L.frames_offset, L.frames_capacity, sizeof(cape_packed_frame)) ||
        !section_fits(L.planes_offset, L.planes_capacity, sizeof(cape_packed_plane)) ||
        !section_fits(PL.polygon_header_offset, 1, sizeof(cape_packed_polygon_header)) ||
        !section_fits(PL.polygons_offset, PL.polygons_capacity, sizeof(cape_polygon)) ||
        !section_fits(PL.vertices_offset, PL.vertices_capacity, 2 * sizeof(double)))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the layout's sections do not fit bytes_per_rank, overlap or are not 16-byte aligned (pass the layouts "
                                               "of cape_gather_configure_polygons, and 16-byte aligned shards)");
    if ((int64_t)n_shards * L.frames_capacity > std::numeric_limits<int32_t>::max())
        return fail(CAPE_ERR_CAPACITY, "n_shards x frames_capacity exceeds an int32");
    const int nSlots = n_shards * L.frames_capacity;
    auto& S = h->shardMatch;
    const int nMap = h->map.n;
    const bool keepAreas = (flags & CAPE_MATCH_MAP_AREAS) != 0;
    const size_t areaDoubles = (size_t)nSlots * nMap * CAPE_MAX_PLANES;
    if (keepAreas && areaDoubles * sizeof(double) > kMapAreasBudget)
        return fail(CAPE_ERR_CAPACITY, "the inter-area table of this call would exceed 1 GiB (fewer shards per call, or no CAPE_MATCH_MAP_AREAS)");
    const uint32_t* deviceSkip = nullptr;
    if (flags & CAPE_MATCH_MAP_DEVICE_SKIP)
        if (const int rc = device_skip_words(h, nSlots, skip, &deviceSkip); rc != CAPE_OK)
            return rc;
    CAPE_ON_DEVICE(h);
    S.slots = 0; // (the buffers of the last call's results may be replaced below)
    const int skipWords = (nMap + 31) / 32;
    const size_t poseBytes = (size_t)nSlots * 16 * sizeof(double);
    const size_t skipBytes = skip ? (size_t)nSlots * skipWords * sizeof(uint32_t) : 0;
    const size_t cap = std::min((size_t)nSlots * (size_t)std::max(nMap, 1) * CAPE_MAX_PLANES, kMapWorkMax);
    const MapWorkLayout lay = map_work_layout(nSlots, cap);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    if (S.poses.size() < poseBytes + skipBytes)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        S.posesTwin = cape::abi::PinnedTwin{};
        CAPE_HIP_TRY(S.poses.alloc(poseBytes + (size_t)nSlots * (CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t)));
    }
    CAPE_HIP_TRY(S.frames.grow((size_t)nSlots, drain));
    CAPE_HIP_TRY(S.match.grow((size_t)nSlots * std::max(nMap, 1), drain));
    CAPE_HIP_TRY(S.kept.grow((size_t)nSlots * CAPE_MAX_PLANES, drain));
    CAPE_HIP_TRY(S.work.grow(lay.total, drain));
    if (keepAreas)
        CAPE_HIP_TRY(S.areas.grow(areaDoubles, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    CAPE_HIP_TRY(S.posesTwin.upload(S.poses, poseBytes + skipBytes, S.poses.size(), stream,
                                    [&](void* stage) { fill_poses(stage, nSlots, world_to_camera, poseBytes, skip, skipBytes); }));
    cape::MatchMapParams p{};
    bind_map_call(p, h, S.work, lay, cap);
    p.poses = reinterpret_cast<const double*>(S.poses.get());
    p.skip = deviceSkip ? deviceSkip : skipBytes ? reinterpret_cast<const uint32_t*>(S.poses + poseBytes) : nullptr;
    p.frames = S.frames;
    p.match = S.match;
    p.areas = keepAreas ? S.areas.get() : nullptr;
    p.shards = static_cast<const unsigned char*>(shards_dev);
    p.shardBytes = (size_t)L.bytes_per_rank;
    p.framesOffset = (size_t)L.frames_offset;
    p.planesOffset = (size_t)L.planes_offset;
    p.polygonHeaderOffset = (size_t)PL.polygon_header_offset;
    p.polygonsOffset = (size_t)PL.polygons_offset;
    p.verticesOffset = (size_t)PL.vertices_offset;
    p.framesCapacity = L.frames_capacity;
    p.planesCapacity = L.planes_capacity;
    p.verticesCapacity = PL.vertices_capacity;
    p.cells = L.cells;
    p.keptIndex = S.kept;
    set_match_thresholds(p, flags);
    CAPE_HIP_TRY(cape::launch_match_map(p, nSlots, stream));
    S.slots = nSlots;
    h->lastMapMatcher = cape_handle_s::kMapMatchShards;
    S.matchN = nMap;
    S.matchAreas = keepAreas;
    return CAPE_OK;
}

int cape_copy_shard_map_matches(cape_handle h, int32_t n_slots, cape_frame_map_match* frames, int32_t* match, double* inter_area)
{
    if (!h || n_slots < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& S = h->shardMatch;
    if (n_slots > S.slots)
        return fail(CAPE_ERR_CAPACITY, "n_slots exceeds the slots of the last cape_match_map_shards");
    if (inter_area && n_slots > 0 && !S.matchAreas)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_match_map_shards did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)");
    if (n_slots == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)n_slots * S.matchN;
    CAPE_HIP_TRY(copy_out(frames, S.frames, 0, (size_t)n_slots));
    CAPE_HIP_TRY(copy_out(match, S.match, 0, n));
    CAPE_HIP_TRY(copy_out(inter_area, S.areas, 0, n * CAPE_MAX_PLANES));
    return CAPE_OK;
}

int cape_map_visibility(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* moving, void* stream_)
{
    if (!h || n_frames < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or fewer than one frame");
    if (h->map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    auto& V = h->visibility;
    const int nMap = h->map.n;
    V.frames = 0;
    const size_t cap = (size_t)n_frames * (size_t)nMap;
    if (cap * sizeof(unsigned long long) > kVisibilityWorkBudget)
        return fail(CAPE_ERR_CAPACITY, "the work list of this call (n_frames x n_map entries) would exceed 1 GiB (fewer frames per call)");
    if (nMap == 0)
    {
        // an empty map: no words
        V.frames = n_frames;
        V.n = 0;
        return CAPE_OK;
    }
    CAPE_ON_DEVICE(h);
    const int skipWords = (nMap + 31) / 32;
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double);
    const size_t movingBytes = moving ? (size_t)skipWords * sizeof(uint32_t) : 0;
    const VisibilityWorkLayout lay = visibility_work_layout(cap);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them, or a match call reading the words
    if (V.poses.size() < poseBytes + movingBytes)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        V.posesTwin = cape::abi::PinnedTwin{};
        CAPE_HIP_TRY(V.poses.alloc(poseBytes + (size_t)(CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t)));
    }
    CAPE_HIP_TRY(V.skip.grow((size_t)n_frames * (CAPE_MAP_MAX_PLANES / 32), drain));
    CAPE_HIP_TRY(V.work.grow(lay.total, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    CAPE_HIP_TRY(V.posesTwin.upload(V.poses, poseBytes + movingBytes, V.poses.size(), stream,
                                    [&](void* stage) { fill_poses(stage, n_frames, world_to_camera, poseBytes, moving, movingBytes); }));
    cape::MapVisibilityParams p = bind_map_visibility(h);
    p.poses = reinterpret_cast<const double*>(V.poses.get());
    p.moving = movingBytes ? reinterpret_cast<const uint32_t*>(V.poses + poseBytes) : nullptr;
    p.skip = V.skip;
    p.counts = reinterpret_cast<unsigned*>(V.work + lay.counts);
    p.work = reinterpret_cast<unsigned long long*>(V.work + lay.work);
    p.tierLists = reinterpret_cast<unsigned*>(V.work + lay.tiers);
    p.workCapacity = cap;
    CAPE_HIP_TRY(cape::launch_map_visibility(p, n_frames, stream));
    V.frames = n_frames;
    V.n = nMap;
    return CAPE_OK;
}

int cape_copy_map_visibility(cape_handle h, int32_t n_frames, uint32_t* skip_out, int64_t* n_undecided)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& V = h->visibility;
    if (n_frames > V.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_visibility on the current map");
    if (n_undecided)
        *n_undecided = 0;
    if (V.frames == 0 || V.n == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(skip_out, V.skip, 0, (size_t)n_frames * ((V.n + 31) / 32)));
    if (n_undecided)
    {
        unsigned long long count = 0;
        CAPE_HIP_TRY(hipMemcpy(&count, V.work.get() + 8 * sizeof(unsigned), sizeof(count), hipMemcpyDeviceToHost));
        *n_undecided = (int64_t)count;
    }
    return CAPE_OK;
}

int cape_map_measure(cape_handle h, int32_t n_frames, const double* camera_to_world, const double* pose_covariance, void* stream_)
{
    if (!h || n_frames < 0 || !pose_covariance)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, negative frame count or no pose covariance (the zero matrix is not a valid covariance)");
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    auto& M = h->measure;
    M.frames = 0;
    h->kalman.kalmanFrames = 0; // (cape_map_kalman's results belong to the rows this call replaces)
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const size_t B = (size_t)h->cfg.max_batch, nRecords = B + (size_t)h->chain.spillRecords; // a row / slab per record, spill pool included
    const size_t slab = (size_t)h->boundaryCap * 2;
    const bool fresh = !M.rows || !M.vertices;
    CAPE_HIP_TRY(M.rows.ensure(nRecords * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(M.vertices.ensure(nRecords * slab));
    CAPE_HIP_TRY(M.poses.ensure(B * 25));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (fresh)
    {
        // (rows and slabs of records outside the chains of a call's frames are never written: they read as zeros)
        CAPE_HIP_TRY(hipMemsetAsync(M.rows, 0, nRecords * CAPE_MAX_PLANES * sizeof(cape_plane_measurement), stream));
        CAPE_HIP_TRY(hipMemsetAsync(M.vertices, 0, nRecords * slab * sizeof(double), stream));
    }
    // the poses (the identity where none are given), then the pose covariances, through the pinned twin like cape_match_map_wide's
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double), covBytes = (size_t)n_frames * 9 * sizeof(double);
    CAPE_HIP_TRY(M.posesTwin.upload(M.poses, poseBytes + covBytes, B * 25 * sizeof(double), stream, [&](void* stage) {
        fill_poses(stage, n_frames, camera_to_world, poseBytes, nullptr, 0);
        std::memcpy(static_cast<unsigned char*>(stage) + poseBytes, pose_covariance, covBytes);
    }));
    cape::MapMeasureParams p{};
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.maxBatch = h->cfg.max_batch;
    p.nRecords = (int)nRecords;
    p.poses = M.poses;
    p.poseCov = M.poses + (size_t)n_frames * 16;
    p.rows = M.rows;
    p.worldVertices = reinterpret_cast<double2*>(M.vertices.get());
    CAPE_HIP_TRY(cape::launch_map_measure(p, n_frames, stream));
    M.frames = n_frames;
    return CAPE_OK;
}

int cape_device_map_measurements(cape_handle h, cape_plane_measurement** rows, double** world_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (h->measure.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no measurements of the current batch: cape_map_measure has not run since the last cape_build_polygons");
    if (rows)
        *rows = h->measure.rows;
    if (world_vertices)
        *world_vertices = h->measure.vertices;
    return CAPE_OK;
}

int cape_copy_map_measurements(cape_handle h, int32_t n_frames, cape_plane_measurement* rows, double* world_vertices)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& M = h->measure;
    if (n_frames > M.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_measure of the current batch");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)n_frames;
    CAPE_HIP_TRY(copy_out(rows, M.rows, 0, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(world_vertices, M.vertices, 0, n * (size_t)h->boundaryCap * 2));
    return CAPE_OK;
}

int cape_copy_spill_measurements(cape_handle h, int32_t first, int32_t count, cape_plane_measurement* rows, double* world_vertices)
{
    if (!h || first < 0 || count < 0 || first > h->chain.spillRecords || count > h->chain.spillRecords - first)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / spill record range");
    const auto& M = h->measure;
    if (M.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure has run on the current batch");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t at = (size_t)h->cfg.max_batch + (size_t)first, n = (size_t)count, cap = (size_t)h->boundaryCap;
    CAPE_HIP_TRY(copy_out(rows, M.rows, at * CAPE_MAX_PLANES, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(world_vertices, M.vertices, at * cap * 2, n * cap * 2));
    return CAPE_OK;
}

int cape_map_upload_tracks(cape_handle h, const cape_map_track* tracks, int32_t n)
{
    if (!h || n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative count");
    if (h->map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (n != h->map.n)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the tracks are parallel to the planes of the uploaded map: n must equal its plane count");
    if (n > 0 && !tracks)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    std::vector<cape::MapTrackState> T((size_t)n);
    std::vector<cape::MapTrackTag> G((size_t)n); // (id and result: cape_map_commit keeps them, cape_map_download returns them)
    for (int32_t j = 0; j < n; ++j)
    {
        std::memcpy(T[j].covariance, tracks[j].covariance, sizeof(T[j].covariance));
        T[j].successiveMatched = tracks[j].successive_matched;
        T[j].failedTracking = tracks[j].failed_tracking;
        T[j].flags = tracks[j].flags;
        T[j].pad = 0;
        G[j] = cape::MapTrackTag {tracks[j].id, tracks[j].result, 0u};
    }
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h)); // a cape_map_kalman in flight still reads the old tracks
    auto& K = h->kalman;
    K.tracksN = -1;
    K.kalmanFrames = 0;
    CAPE_HIP_TRY(K.tracks.grow(T.size(), [] { return hipSuccess; }));
    CAPE_HIP_TRY(h->mapCommit.tags.grow(G.size(), [] { return hipSuccess; }));
    if (n > 0)
    {
        CAPE_HIP_TRY(hipMemcpy(K.tracks, T.data(), T.size() * sizeof(cape::MapTrackState), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(h->mapCommit.tags, G.data(), G.size() * sizeof(cape::MapTrackTag), hipMemcpyHostToDevice));
    }
    K.tracksN = n;
    return CAPE_OK;
}

int cape_map_kalman(cape_handle h, int32_t n_frames, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& K = h->kalman;
    const auto& W = h->mapWide;
    const auto& M = h->measure;
    const int nMap = h->map.n;
    K.kalmanFrames = 0;
    if (nMap < 0 || K.tracksN != nMap)
        return fail(CAPE_ERR_CAPACITY, "no tracks for the uploaded map (cape_map_upload, then cape_map_upload_tracks)");
    if (!K.matchedThisMap || W.matchN != nMap || n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "no cape_match_map_wide of the current batch against the uploaded map covers n_frames");
    if (n_frames > M.frames)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure of the current batch covers n_frames");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be writing them
    CAPE_HIP_TRY(K.frames.grow((size_t)n_frames, drain));
    CAPE_HIP_TRY(K.rows.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(K.trackResults.grow((size_t)n_frames * (size_t)std::max(nMap, 1), drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    CAPE_HIP_TRY(cape::launch_map_kalman(bind_map_kalman(h), n_frames, stream));
    K.kalmanFrames = n_frames;
    K.kalmanN = nMap;
    ++K.runs; // (cape_map_union's results belong to the rows this call replaced)
    return CAPE_OK;
}

int cape_device_map_kalman(cape_handle h, cape_frame_map_kalman** frames, cape_plane_fusion** rows, cape_map_track_result** track_results)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!kalman_results_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_kalman has run on the current batch, map, match and measurements");
    if (frames)
        *frames = h->kalman.frames;
    if (rows)
        *rows = h->kalman.rows;
    if (track_results)
        *track_results = h->kalman.trackResults;
    return CAPE_OK;
}

int cape_copy_map_kalman(cape_handle h, int32_t n_frames, cape_frame_map_kalman* frames, cape_plane_fusion* rows,
                         cape_map_track_result* track_results)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& K = h->kalman;
    if (n_frames > (kalman_results_live(h) ? K.kalmanFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_kalman on the current batch, map, match and measurements");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(frames, K.frames, 0, (size_t)n_frames));
    CAPE_HIP_TRY(copy_out(rows, K.rows, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(track_results, K.trackResults, 0, (size_t)n_frames * (size_t)K.kalmanN));
    return CAPE_OK;
}

// cape_map_union, cape_map_union_holes and cape_map_union_cut: the same preconditions, rows and slab; the kernels of the last two
// and their rings table
enum MapUnionMode { kUnionPlain, kUnionWithHoles, kUnionWithCuts };
static int map_union(cape_handle h, int32_t n_frames, void* stream_, MapUnionMode mode)
{
    const bool holes = mode != kUnionPlain;
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& U = h->mapUnion;
    const auto& K = h->kalman;
    U.unionFrames = 0;
    h->mapUnionRings.current = false;
    if (!kalman_results_live(h) || n_frames > K.kalmanFrames || K.kalmanN != h->map.n)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_kalman on the current batch, map, tracks and measurements covers n_frames");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be writing them
    CAPE_HIP_TRY(U.rows.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(U.vertices.grow((size_t)n_frames * SLAB * 2, drain));
    if (holes)
        CAPE_HIP_TRY(h->mapUnionRings.rows.grow((size_t)n_frames * WP, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    const cape::MapUnionParams p = bind_map_union(h);
    CAPE_HIP_TRY(mode == kUnionWithCuts    ? cape::launch_map_union_cut(p, h->mapUnionRings.rows, n_frames, stream)
                 : mode == kUnionWithHoles ? cape::launch_map_union_holes(p, h->mapUnionRings.rows, n_frames, stream)
                                           : cape::launch_map_union(p, n_frames, stream));
    U.unionFrames = n_frames;
    U.kalmanRun = K.runs;
    h->mapUnionRings.current = holes;
    return CAPE_OK;
}

int cape_map_union(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionPlain); }
int cape_map_union_holes(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionWithHoles); }
int cape_map_union_cut(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionWithCuts); }

int cape_device_map_union_rings(cape_handle h, cape_plane_union_rings** rings)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!union_results_live(h) || !h->mapUnionRings.current)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union_holes or cape_map_union_cut has run on the current batch, map, match, measurements and Kalman results, or a cape_map_union has replaced its rows");
    if (rings)
        *rings = h->mapUnionRings.rows;
    return CAPE_OK;
}

int cape_copy_map_union_rings(cape_handle h, int32_t n_frames, cape_plane_union_rings* rings)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& U = h->mapUnion;
    if (n_frames > (union_results_live(h) && h->mapUnionRings.current ? U.unionFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_union_holes or cape_map_union_cut on the current batch, map, match, measurements and Kalman results (a cape_map_union replaces its rows)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(rings, h->mapUnionRings.rows, 0, (size_t)n_frames * WP));
    return CAPE_OK;
}

int cape_device_map_union(cape_handle h, cape_plane_union** rows, double** vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!union_results_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union has run on the current batch, map, match, measurements and Kalman results");
    if (rows)
        *rows = h->mapUnion.rows;
    if (vertices)
        *vertices = h->mapUnion.vertices;
    return CAPE_OK;
}

int cape_copy_map_union(cape_handle h, int32_t n_frames, cape_plane_union* rows, double* vertices)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& U = h->mapUnion;
    if (n_frames > (union_results_live(h) ? U.unionFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_union on the current batch, map, match, measurements and Kalman results");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(rows, U.rows, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(vertices, U.vertices, 0, (size_t)n_frames * SLAB * 2));
    return CAPE_OK;
}

// cape_map_commit: the sequential step of a tracking loop.  Two launches behind the union, then the one small read that tells the host
// the new map's sizes: front and back buffers are swapped here, on the host, only if the header says DONE.
int cape_map_commit(cape_handle h, int32_t frame, uint32_t flags, uint64_t* next_id, cape_map_commit_result* out, void* stream_)
{
    if (!h || !out || !next_id || frame < 0 || (flags & ~(uint32_t)CAPE_COMMIT_ADD_STAGED))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result or next_id, a negative frame or an unknown flag");
    auto& map = h->map;
    auto& K = h->kalman;
    auto& U = h->mapUnion;
    auto& X = h->mapCommit;
    if (!union_results_live(h) || frame >= U.unionFrames || K.kalmanN != map.n || K.tracksN != map.n)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union, cape_map_union_holes or cape_map_union_cut on the current batch, map, match, measurements and Kalman results covers `frame`");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the back buffers, to bounds the host knows
    const CommitBounds bounds = commit_bounds(h);
    const auto drain = [h] { return drain_handle(h); }; // (a back buffer was the front one of an earlier map: a call in flight may read it)
    CAPE_HIP_TRY(X.planes.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.rings.grow(bounds.rings, drain));
    CAPE_HIP_TRY(X.vertices.grow(bounds.vertices * 2, drain));
    CAPE_HIP_TRY(X.tracks.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.tagsBack.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(X.header.ensure(1));
    if (!X.headerHost)
        CAPE_HIP_TRY(X.headerHost.alloc_host(1, hipHostMallocDefault));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_commit_result result{};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        const cape::MapCommitParams p = bind_map_commit(h, (size_t)frame, frame, h->mapUnionRings.current, flags, *next_id, bounds, X.header);
        CAPE_HIP_TRY(cape::launch_map_commit(p, commit_planes_bound(h, bounds, flags), stream));
        CAPE_HIP_TRY(hipMemcpyAsync(X.headerHost, X.header, sizeof(cape_map_commit_result), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: the header, and with it both kernels
        result = *X.headerHost.get();
    }
    if (result.flags & CAPE_COMMIT_DONE)
    {
        swap_map_set(h, X.planes, X.rings, X.vertices, X.tracks, X.tagsBack);
        map.n = result.n_planes;
        X.nRings = result.n_rings;
        X.nVertices = result.n_vertices;
        K.tracksN = result.n_planes; // the committed tracks are those of the new map
        // what cape_map_upload invalidates: the words of the old map, the wide match against it and what was made of them
        h->visibility.frames = 0;
        K.matchedThisMap = false;
        K.kalmanFrames = 0;
        *next_id = result.next_id;
    }
    *out = result;
    return CAPE_OK;
}

int cape_map_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (h->map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (n_planes)
        *n_planes = h->map.n;
    if (n_rings)
        *n_rings = h->mapCommit.nRings;
    if (n_vertices)
        *n_vertices = h->mapCommit.nVertices;
    return CAPE_OK;
}

int cape_map_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                      double* vertices, int64_t vertices_capacity, cape_map_track* tracks)
{
    if (!h || planes_capacity < 0 || rings_capacity < 0 || vertices_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& map = h->map;
    const auto& X = h->mapCommit;
    if (map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (map.n > planes_capacity || X.nRings > rings_capacity || X.nVertices > vertices_capacity)
        return fail(CAPE_ERR_CAPACITY, "an array is too small for the device map (cape_map_info tells its sizes)");
    if ((map.n > 0 && !planes) || (X.nRings > 0 && !rings) || (X.nVertices > 0 && !vertices))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)map.n;
    if (n == 0)
        return CAPE_OK;
    CAPE_HIP_TRY(hipMemcpy(planes, map.planes, n * sizeof(cape_map_plane), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(rings, map.rings, (size_t)X.nRings * sizeof(cape_map_ring), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(vertices, map.vertices, (size_t)X.nVertices * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (tracks)
    {
        std::memset(tracks, 0, n * sizeof(cape_map_track)); // (the zero track per plane if none were uploaded for this map)
        if (h->kalman.tracksN == map.n)
        {
            std::vector<cape::MapTrackState> T(n);
            std::vector<cape::MapTrackTag> G(n);
            CAPE_HIP_TRY(hipMemcpy(T.data(), h->kalman.tracks, n * sizeof(cape::MapTrackState), hipMemcpyDeviceToHost));
            CAPE_HIP_TRY(hipMemcpy(G.data(), X.tags, n * sizeof(cape::MapTrackTag), hipMemcpyDeviceToHost));
            for (size_t j = 0; j < n; ++j)
            {
                std::memcpy(tracks[j].covariance, T[j].covariance, sizeof(T[j].covariance));
                tracks[j].successive_matched = T[j].successiveMatched;
                tracks[j].failed_tracking = T[j].failedTracking;
                tracks[j].flags = T[j].flags;
                tracks[j].result = G[j].result;
                tracks[j].id = G[j].id;
            }
        }
    }
    return CAPE_OK;
}

// cape_map_maintain: PROMOTE, DROP and LOST executed on the device map.  Like the commit: two launches, then the one small read that
// tells the host the new sizes; front and back buffers are swapped here, on the host, only if the header says DONE.
int cape_map_maintain(cape_handle h, uint32_t flags, cape_map_maintain_result* out, void* stream_)
{
    if (!h || !out || flags != 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or result, or a flag (none is defined)");
    auto& map = h->map;
    auto& K = h->kalman;
    auto& X = h->mapCommit;
    auto& R = h->mapMaintain;
    if (map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (K.tracksN != map.n)
        return fail(CAPE_ERR_CAPACITY, "no tracks are current for the map (cape_map_upload_tracks, or a DONE cape_map_commit)");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the back buffers and the log, to bounds the host knows: the new map is no larger than the old one, and the log takes at most
    // the whole map on top of what it holds
    const size_t n = (size_t)map.n, nRings = (size_t)X.nRings, nVertices = (size_t)X.nVertices;
    const auto drain = [h] { return drain_handle(h); }; // (a back buffer was the front one of an earlier map: a call in flight may read it)
    CAPE_HIP_TRY(X.planes.grow(n, drain));
    CAPE_HIP_TRY(X.rings.grow(nRings, drain));
    CAPE_HIP_TRY(X.vertices.grow(nVertices * 2, drain));
    CAPE_HIP_TRY(X.tracks.grow(n, drain));
    CAPE_HIP_TRY(X.tagsBack.grow(n, drain));
    const cape::MaintainLog log = cape::maintain_log_bounds(cape::MaintainCursor {R.nPlanes, R.nRings, R.nVertices}, n, nRings, nVertices);
    if (const int rc = grow_retired_log(h, log); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(R.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(R.header.ensure(1));
    if (!R.headerHost)
        CAPE_HIP_TRY(R.headerHost.alloc_host(1, hipHostMallocDefault));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_maintain_result result{};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        cape::MapMaintainParams p{};
        p.mapPlanes = map.planes;
        p.mapRings = map.rings;
        p.mapVertices = map.vertices;
        p.tracks = K.tracks;
        p.tags = X.tags;
        p.nMap = map.n;
        p.nMapRings = X.nRings;
        p.nMapVertices = X.nVertices;
        p.outPlanes = X.planes;
        p.outRings = X.rings;
        p.outVertices = X.vertices;
        p.outTracks = X.tracks;
        p.outTags = X.tagsBack;
        p.planesCapacity = n;
        p.ringsCapacity = nRings;
        p.verticesCapacity = nVertices;
        p.logPlanes = R.planes;
        p.logRings = R.rings;
        p.logVertices = R.vertices;
        p.logTracks = R.tracks;
        p.log = log;
        p.plan = R.plan;
        p.header = R.header;
        CAPE_HIP_TRY(cape::launch_map_maintain(p, stream));
        CAPE_HIP_TRY(hipMemcpyAsync(R.headerHost, R.header, sizeof(cape_map_maintain_result), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: the header, and with it both kernels
        result = *R.headerHost.get();
    }
    if (result.flags & CAPE_MAINTAIN_DONE)
    {
        swap_map_set(h, X.planes, X.rings, X.vertices, X.tracks, X.tagsBack);
        map.n = result.n_planes;
        X.nRings = result.n_rings;
        X.nVertices = result.n_vertices;
        K.tracksN = result.n_planes; // the tracks are those of the new map
        R.nPlanes = result.n_retired;
        R.nRings = result.n_retired_rings;
        R.nVertices = result.n_retired_vertices;
        // what a DONE commit invalidates: the words of the old map, the wide match against it and what was made of them
        h->visibility.frames = 0;
        K.matchedThisMap = false;
        K.kalmanFrames = 0;
    }
    *out = result;
    return CAPE_OK;
}

int cape_map_retired_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (n_planes)
        *n_planes = h->mapMaintain.nPlanes;
    if (n_rings)
        *n_rings = h->mapMaintain.nRings;
    if (n_vertices)
        *n_vertices = h->mapMaintain.nVertices;
    return CAPE_OK;
}

int cape_map_retired_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                              double* vertices, int64_t vertices_capacity, cape_map_track* tracks)
{
    if (!h || planes_capacity < 0 || rings_capacity < 0 || vertices_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& R = h->mapMaintain;
    if (R.nPlanes > planes_capacity || R.nRings > rings_capacity || R.nVertices > vertices_capacity)
        return fail(CAPE_ERR_CAPACITY, "an array is too small for the retired log (cape_map_retired_info tells its sizes)");
    if ((R.nPlanes > 0 && !planes) || (R.nRings > 0 && !rings) || (R.nVertices > 0 && !vertices))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    if (R.nPlanes == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(hipMemcpy(planes, R.planes, (size_t)R.nPlanes * sizeof(cape_map_plane), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(rings, R.rings, (size_t)R.nRings * sizeof(cape_map_ring), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(vertices, R.vertices, (size_t)R.nVertices * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (tracks)
        CAPE_HIP_TRY(hipMemcpy(tracks, R.tracks, (size_t)R.nPlanes * sizeof(cape_map_track), hipMemcpyDeviceToHost));
    return CAPE_OK;
}

int cape_map_retired_clear(cape_handle h)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    auto& R = h->mapMaintain;
    if (R.nPlanes > 0)
    {
        CAPE_ON_DEVICE(h);
        CAPE_HIP_TRY(drain_handle(h));
    }
    R.nPlanes = R.nRings = 0;
    R.nVertices = 0;
    return CAPE_OK;
}

} // extern "C"

namespace {

// what cape_map_step_visible reports beside the step's result
struct StepVisibleCounts
{
    int32_t nMap = 0, nMoving = 0, nListed = 0;
    int64_t nUndecided = 0;
};

// cape_map_step and cape_map_step_visible: one frame through match, Kalman step, union with cuts, commit and maintenance, the last
// decided on the device from the commit's header.  Every buffer is grown before the first launch; one copy brings both headers back,
// one wait ends the call; the host learns which buffer set holds the map from the same function the maintenance kernels took their
// source from.  visible == nullptr: the gate reads the caller's skip words (or none).  Else they are decided ahead of the gate, on
// the same stream, from the pose row the gate reads and the front set's planes and tracks, into MapStepVisible::skip; their
// counters come back in a second small copy before the one wait.
int map_step_body(cape_handle h, int32_t frame, const double* world_to_camera, const uint32_t* skip, StepVisibleCounts* visible, uint32_t match_flags,
                  uint32_t commit_flags, uint64_t* next_id, cape_map_step_result* out, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    constexpr uint32_t kStepMatchFlags = CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0;
    if (!h || !out || !next_id || !world_to_camera || frame < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result, next_id or pose, or a negative frame");
    if (match_flags & (CAPE_MATCH_MAP_AREAS | CAPE_MATCH_MAP_DEVICE_SKIP))
        return fail(CAPE_ERR_INVALID_ARGUMENT, visible ? "cape_map_step_visible takes neither CAPE_MATCH_MAP_AREAS nor CAPE_MATCH_MAP_DEVICE_SKIP (it decides the words itself)"
                                                       : "cape_map_step takes neither CAPE_MATCH_MAP_AREAS nor CAPE_MATCH_MAP_DEVICE_SKIP (the visibility words do not survive a commit)");
    if ((match_flags & ~kStepMatchFlags) || (commit_flags & ~(uint32_t)CAPE_COMMIT_ADD_STAGED))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match or commit flag");
    auto& map = h->map;
    auto& W = h->mapWide;
    auto& K = h->kalman;
    auto& U = h->mapUnion;
    auto& X = h->mapCommit;
    auto& R = h->mapMaintain;
    auto& S = h->mapStep;
    auto& SV = h->mapStepVisible;
    if (map.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (K.tracksN != map.n)
        return fail(CAPE_ERR_CAPACITY, "no tracks are current for the map (cape_map_upload_tracks, or a DONE commit, maintenance or step)");
    if (frame >= h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "`frame` lies beyond the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (frame >= h->measure.frames)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure of the current batch covers `frame`");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the step works in row 0 of the batch-wide tables of the three calls it stands for: whatever they held is gone from here on
    W.matchFrames = 0;
    K.kalmanFrames = 0;
    U.unionFrames = 0;
    h->mapUnionRings.current = false;
    // ---- every buffer of the five steps, before the first launch
    const int B = h->cfg.max_batch, nMap = map.n, skipWords = (nMap + 31) / 32;
    const size_t n = (size_t)nMap;
    const size_t poseCapacity = (size_t)B * 16 * sizeof(double) + (size_t)B * (CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t);
    const size_t workCap = std::min((size_t)B * (size_t)std::max(nMap, 1) * WP, kMapWorkMax);
    const MapWorkLayout lay = map_work_layout(B, workCap, 2);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    CAPE_HIP_TRY(W.frames.ensure((size_t)B));
    CAPE_HIP_TRY(W.match.ensure((size_t)B * CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(W.planes.ensure(2 * (size_t)B * WP));
    CAPE_HIP_TRY(W.kept.ensure((size_t)B * WP));
    CAPE_HIP_TRY(W.poses.ensure(poseCapacity));
    CAPE_HIP_TRY(W.work.grow(lay.total, drain));
    CAPE_HIP_TRY(K.frames.grow(1, drain));
    CAPE_HIP_TRY(K.rows.grow(WP, drain));
    CAPE_HIP_TRY(K.trackResults.grow(std::max<size_t>(n, 1), drain));
    CAPE_HIP_TRY(U.rows.grow(WP, drain));
    CAPE_HIP_TRY(U.vertices.grow(SLAB * 2, drain));
    CAPE_HIP_TRY(h->mapUnionRings.rows.grow(WP, drain));
    // the commit's destination and the maintenance's, both to the commit's bounds: the committed map is the largest of the three
    const CommitBounds bounds = commit_bounds(h);
    CAPE_HIP_TRY(X.planes.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.rings.grow(bounds.rings, drain));
    CAPE_HIP_TRY(X.vertices.grow(bounds.vertices * 2, drain));
    CAPE_HIP_TRY(X.tracks.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.tagsBack.grow(bounds.planes, drain));
    CAPE_HIP_TRY(X.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(S.planes.grow(bounds.planes, drain));
    CAPE_HIP_TRY(S.rings.grow(bounds.rings, drain));
    CAPE_HIP_TRY(S.vertices.grow(bounds.vertices * 2, drain));
    CAPE_HIP_TRY(S.tracks.grow(bounds.planes, drain));
    CAPE_HIP_TRY(S.tags.grow(bounds.planes, drain));
    // ... and the log, for the committed map's bounds in place of a map's sizes (the kernels derive the log's capacities from the
    // committed sizes, which are no larger)
    const cape::MaintainCursor held{R.nPlanes, R.nRings, R.nVertices};
    if (const int rc = grow_retired_log(h, cape::maintain_log_bounds(held, bounds.planes, bounds.rings, bounds.vertices)); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(R.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(S.header.ensure(1));
    if (!S.headerHost)
        CAPE_HIP_TRY(S.headerHost.alloc_host(1, hipHostMallocDefault));
    // ... and what the visibility kernels take: one frame's words, work list and tier lists, the counters' pinned twin
    const VisibilityWorkLayout visLay = visibility_work_layout(n);
    const bool decide = visible && nMap > 0; // (an empty map has no words: no kernel runs for them)
    if (visible)
    {
        SV.n = -1; // (whatever words it held: gone from here on)
        CAPE_HIP_TRY(SV.skip.grow(CAPE_MAP_MAX_PLANES / 32, drain));
        CAPE_HIP_TRY(SV.work.grow(visLay.total, drain));
        if (!SV.countsHost)
            CAPE_HIP_TRY(SV.countsHost.alloc_host(16, hipHostMallocDefault));
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_step_result result{};
    unsigned counts[16] = {};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        // ---- the wide match of frame `frame`: its pose and skip words at row 0, its chain found through the chain base
        const size_t poseBytes = 16 * sizeof(double), skipBytes = skip ? (size_t)skipWords * sizeof(uint32_t) : 0;
        CAPE_HIP_TRY(W.posesTwin.upload(W.poses, poseBytes + skipBytes, poseCapacity, stream,
                                        [&](void* stage) { fill_poses(stage, 1, world_to_camera, poseBytes, skip, skipBytes); }));
        cape::MatchMapParams pm;
        pm.records = h->res.records;
        pm.polygons = h->poly.polygons;
        pm.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
        pm.boundaryCapacity = h->boundaryCap;
        pm.maxBatch = B;
        pm.nRecords = B + h->chain.spillRecords;
        bind_map_call(pm, h, W.work, lay, workCap);
        pm.poses = reinterpret_cast<const double*>(W.poses.get());
        pm.skip = skipBytes ? reinterpret_cast<const uint32_t*>(W.poses + poseBytes) : nullptr;
        if (decide)
        {
            // ---- the frame's skip words, from the pose row the gate reads and the FRONT set's planes and tracks
            cape::MapVisibilityParams pv = bind_map_visibility(h);
            pv.poses = pm.poses;
            pv.skip = SV.skip;
            pv.counts = reinterpret_cast<unsigned*>(SV.work + visLay.counts);
            pv.work = reinterpret_cast<unsigned long long*>(SV.work + visLay.work);
            pv.tierLists = reinterpret_cast<unsigned*>(SV.work + visLay.tiers);
            pv.workCapacity = n;
            CAPE_HIP_TRY(cape::launch_map_step_visibility(pv, K.tracks, stream));
            pm.skip = SV.skip;
        }
        pm.frames = nullptr;
        pm.framesWide = W.frames;
        pm.match = W.match;
        pm.segCur = W.planes;
        pm.mapOf = W.planes + (size_t)B * WP;
        pm.keptIndex = W.kept;
        pm.areas = nullptr;
        pm.chainBase = frame;
        set_match_thresholds(pm, match_flags);
        CAPE_HIP_TRY(cape::launch_match_map_wide(pm, 1, stream));
        h->lastMapMatcher = cape_handle_s::kMapMatchWide;
        // ---- the Kalman step and the union with cuts on the same rows
        CAPE_HIP_TRY(cape::launch_map_kalman(bind_map_kalman(h), 1, stream));
        ++K.runs; // (cape_map_union's results belong to the rows this call replaced)
        CAPE_HIP_TRY(cape::launch_map_union_cut(bind_map_union(h), h->mapUnionRings.rows, 1, stream));
        // ---- the commit: front set -> back set
        cape_map_step_result* header = S.header.get();
        const cape::MapCommitParams pc = bind_map_commit(h, 0, frame, true, commit_flags, *next_id, bounds, &header->commit);
        CAPE_HIP_TRY(cape::launch_map_commit(pc, commit_planes_bound(h, bounds, commit_flags), stream));
        // ---- the maintenance behind it: back set -> third set, its sizes and whether it runs read from the commit's header
        cape::MapStepParams ps{};
        ps.commit = &header->commit;
        cape::MapMaintainParams& p = ps.maintain;
        p.mapPlanes = X.planes;
        p.mapRings = X.rings;
        p.mapVertices = X.vertices;
        p.tracks = X.tracks;
        p.tags = X.tagsBack;
        p.outPlanes = S.planes;
        p.outRings = S.rings;
        p.outVertices = S.vertices;
        p.outTracks = S.tracks;
        p.outTags = S.tags;
        p.logPlanes = R.planes;
        p.logRings = R.rings;
        p.logVertices = R.vertices;
        p.logTracks = R.tracks;
        p.log.held = held;
        p.plan = R.plan;
        p.header = &header->maintain;
        CAPE_HIP_TRY(cape::launch_map_step_maintain(ps, commit_planes_bound(h, bounds, commit_flags), stream));
        CAPE_HIP_TRY(hipMemcpyAsync(S.headerHost, S.header, sizeof(cape_map_step_result), hipMemcpyDeviceToHost, stream));
        if (decide)
            CAPE_HIP_TRY(hipMemcpyAsync(SV.countsHost, SV.work + visLay.counts, sizeof(counts), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: both headers, and with them every kernel
        result = *S.headerHost.get();
        if (decide)
            std::memcpy(counts, SV.countsHost.get(), sizeof(counts));
    }
    if (visible)
    {
        // the words stand for the map as the call found it, whatever becomes of it below
        SV.n = nMap;
        visible->nMap = nMap;
        visible->nMoving = (int32_t)counts[10];
        visible->nListed = (int32_t)counts[11];
        unsigned long long undecided = 0;
        std::memcpy(&undecided, counts + 8, sizeof(undecided));
        visible->nUndecided = (int64_t)undecided;
    }
    // ---- where the map lies now, and what it holds
    const cape::StepMapState after = cape::step_map_after(result.commit, result.maintain);
    if (after.set == cape::kStepSetBack)
        swap_map_set(h, X.planes, X.rings, X.vertices, X.tracks, X.tagsBack);
    else if (after.set == cape::kStepSetThird)
        swap_map_set(h, S.planes, S.rings, S.vertices, S.tracks, S.tags);
    if (after.set != cape::kStepSetFront)
    {
        map.n = after.planes;
        X.nRings = after.rings;
        X.nVertices = after.vertices;
        K.tracksN = after.planes; // the tracks are those of the new map
        h->visibility.frames = 0; // (the words of the old map)
        *next_id = result.commit.next_id;
    }
    if (result.maintain.flags & CAPE_MAINTAIN_DONE)
    {
        R.nPlanes = result.maintain.n_retired;
        R.nRings = result.maintain.n_retired_rings;
        R.nVertices = result.maintain.n_retired_vertices;
    }
    K.matchedThisMap = false; // (the one-frame match is the step's own: a cape_map_kalman needs a cape_match_map_wide of its frames)
    *out = result;
    return CAPE_OK;
}

} // namespace

extern "C" {

int cape_map_step(cape_handle h, int32_t frame, const double* world_to_camera, const uint32_t* skip, uint32_t match_flags, uint32_t commit_flags,
                  uint64_t* next_id, cape_map_step_result* out, void* stream)
{
    return map_step_body(h, frame, world_to_camera, skip, nullptr, match_flags, commit_flags, next_id, out, stream);
}

// cape_map_step_visible: cape_map_step with the frame's skip words decided on the device, ahead of the gate, from the tracks' moving
// bits and the map as the call finds it
int cape_map_step_visible(cape_handle h, int32_t frame, const double* world_to_camera, uint32_t match_flags, uint32_t commit_flags,
                          uint64_t* next_id, cape_map_step_visible_result* out, void* stream)
{
    if (!out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result, next_id or pose, or a negative frame");
    StepVisibleCounts counts;
    cape_map_step_result step{};
    if (const int rc = map_step_body(h, frame, world_to_camera, nullptr, &counts, match_flags, commit_flags, next_id, &step, stream); rc != CAPE_OK)
        return rc;
    cape_map_step_visible_result result{};
    result.step = step;
    result.n_map = counts.nMap;
    result.n_moving = counts.nMoving;
    result.n_listed = counts.nListed;
    result.n_undecided = counts.nUndecided;
    *out = result;
    return CAPE_OK;
}

int cape_map_step_skip_words(cape_handle h, uint32_t* words, int32_t words_capacity, int32_t* n_map)
{
    if (!h || words_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& SV = h->mapStepVisible;
    if (SV.n < 0)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_step_visible has run since the last cape_map_upload");
    if (n_map)
        *n_map = SV.n;
    const int nWords = (SV.n + 31) / 32;
    if (nWords > words_capacity)
        return fail(CAPE_ERR_CAPACITY, "words_capacity is too small for the words of the last cape_map_step_visible ((n_map + 31) / 32)");
    if (nWords == 0)
        return CAPE_OK;
    if (!words)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null words");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(words, SV.skip, 0, (size_t)nWords));
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
