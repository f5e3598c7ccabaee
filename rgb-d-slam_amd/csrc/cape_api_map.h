// Private header of the map's entry points (cape_api_map_match.hip, cape_api_map_update.hip; cape_api_geometry.hip shares the work
// layout and the thresholds): the work layouts, the one body of the map matchers, what the visibility kernels read of the handle,
// the maintenance's parameters, and the two statements of a changed map -- which set holds it, and what it invalidates.  Host code
// only; every function is inline and defined here once.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/cape_hip.h"

namespace cape::abi {

// ---- the work buffers of the matchers and of the visibility kernels: one allocation each, its sections on 256-byte boundaries in
// the order of the struct's members.  (No HIP call and no handle up to CAPE_API_MAP_LAYOUTS_ONLY: tests/host/map_work_layout.cpp
// compiles this part alone.)
constexpr size_t work_section(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// cape_match_map*: counters, per-frame ranges, the gate masks (maskWords 64-bit words per map plane: one for frames of up to 64 kept
// planes, two for cape_match_map_wide's 128, none for cape_match_polygons_wide, which has no map), the work list, its areas, the
// tier lists.  cape_debug_map_match_lists reads the counters at the buffer's start.
struct MapWorkLayout
{
    size_t counts, ranges, masks, work, area, tiers, total;
};
constexpr MapWorkLayout map_work_layout(int maxBatch, size_t cap, int maskWords)
{
    MapWorkLayout l{};
    l.counts = 0;
    l.ranges = work_section(16 * sizeof(unsigned));
    l.masks = l.ranges + work_section((size_t)maxBatch * sizeof(uint2));
    l.work = l.masks + work_section((size_t)maxBatch * CAPE_MAP_MAX_PLANES * maskWords * sizeof(unsigned long long));
    l.area = l.work + work_section(cap * sizeof(unsigned long long));
    l.tiers = l.area + work_section(cap * sizeof(double));
    l.total = l.tiers + work_section(3 * cap * sizeof(unsigned));
    return l;
}
// cape_map_visibility and cape_map_step_visible: counters, the work list, the tier lists
struct VisibilityWorkLayout
{
    size_t counts, work, tiers, total;
};
constexpr VisibilityWorkLayout visibility_work_layout(size_t cap)
{
    VisibilityWorkLayout l{};
    l.counts = 0;
    l.work = work_section(16 * sizeof(unsigned));
    l.tiers = l.work + work_section(cap * sizeof(unsigned long long));
    l.total = l.tiers + work_section(3 * cap * sizeof(unsigned));
    return l;
}
constexpr size_t kMapWorkMax = (size_t)1 << 24;           // entries of a map matcher's work list at most (448 MB of buffers)
constexpr size_t kMapAreasBudget = (size_t)1 << 30;       // bytes of a dense inter-area table at most
constexpr size_t kVisibilityWorkBudget = (size_t)1 << 30; // bytes of the visibility work list at most

} // namespace cape::abi

#ifndef CAPE_API_MAP_LAYOUTS_ONLY

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cape_handle.h"

namespace cape::abi {

// parameters::matching (src/parameters.hpp:89-95), evaluated on the host like the reference's function-local statics
template <typename Params> void set_match_thresholds(Params& p, uint32_t flags)
{
    p.flags = flags;
    p.minCosAngle = std::abs(std::cos(20.0 * M_PI / 180.0));
    p.maxDistance = 100.0;
    const double planeMinimalOverlap = static_cast<double>(0.4f);
    p.minOverlap = (flags & CAPE_MATCH_ADVANCED) ? planeMinimalOverlap / 2 : planeMinimalOverlap;
}

// the pinned twin's bytes of a map call: n x 16 doubles (the identity where no poses are given: the statements stay those of a pose),
// then the skip words
inline void fill_poses(void* stage, int n, const double* world_to_camera, size_t poseBytes, const uint32_t* skip, size_t skipBytes)
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

// CAPE_MATCH_MAP_DEVICE_SKIP: the skip words of the last cape_map_visibility for a match call over n frames (or slots), or the
// reason there are none
inline int device_skip_words(const cape_handle_s* h, int n, const uint32_t* skip, const uint32_t** words)
{
    const auto& V = h->visibility;
    if (skip)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_MATCH_MAP_DEVICE_SKIP takes the skip words of cape_map_visibility: skip must be NULL");
    if (V.frames <= 0 || V.n != h->maps.n)
        return fail(CAPE_ERR_CAPACITY, "CAPE_MATCH_MAP_DEVICE_SKIP: no cape_map_visibility has run since the last cape_map_upload");
    if (n > V.frames)
        return fail(CAPE_ERR_CAPACITY, "CAPE_MATCH_MAP_DEVICE_SKIP: the last cape_map_visibility covered fewer frames than this call");
    *words = V.skip;
    return CAPE_OK;
}

// the pair list (PairList, cape_internal.h) in a work buffer: the sections of a matcher's layout, or of the visibility kernels', whose
// list has neither areas nor ranges
inline cape::PairList bind_pair_list(unsigned char* work, const MapWorkLayout& lay, size_t cap)
{
    return {reinterpret_cast<unsigned long long*>(work + lay.work), reinterpret_cast<double*>(work + lay.area), reinterpret_cast<unsigned*>(work + lay.tiers),
            reinterpret_cast<unsigned*>(work + lay.counts), reinterpret_cast<uint2*>(work + lay.ranges), cap};
}
inline cape::PairList bind_pair_list(unsigned char* work, const VisibilityWorkLayout& lay, size_t cap)
{
    return {reinterpret_cast<unsigned long long*>(work + lay.work), nullptr, reinterpret_cast<unsigned*>(work + lay.tiers), reinterpret_cast<unsigned*>(work + lay.counts),
            nullptr, cap};
}

// what the visibility kernels read of the handle, for cape_map_visibility and cape_map_step_visible: the front map, the camera, the
// device, and the sections of the call's work buffer
inline cape::MapVisibilityParams bind_map_visibility(const cape_handle_s* h, unsigned char* work, const VisibilityWorkLayout& lay, size_t cap)
{
    cape::MapVisibilityParams p{};
    p.list = bind_pair_list(work, lay, cap);
    p.mapPlanes = h->maps.front.planes;
    p.mapRings = h->maps.front.rings;
    p.mapVertices = reinterpret_cast<const double2*>(h->maps.front.vertices.get());
    p.nMap = h->maps.n;
    p.skipWords = (h->maps.n + 31) / 32;
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

// ---- the map matchers: cape_match_map, cape_match_map_wide, cape_match_map_shards and the match of cape_map_step

constexpr uint32_t kMatchMapFlags = CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0 | CAPE_MATCH_MAP_AREAS | CAPE_MATCH_MAP_DEVICE_SKIP;

// the caller's group of the handle, in this order; a null buffer is a table that matcher does not write
struct MapMatchBuffers
{
    cape_handle_s::Buffer<unsigned char>* poses; // the call's poses, then its skip words
    PinnedTwin* twin;
    cape_handle_s::Buffer<cape_frame_map_match>* frames;
    cape_handle_s::Buffer<cape_frame_map_match_wide>* framesWide; // the wide kernels: per-frame results here and in `planes`
    cape_handle_s::Buffer<int32_t>*match, *planes;                // planes (wide): seg_cur, then map_of
    cape_handle_s::Buffer<uint2>* kept;
    cape_handle_s::Buffer<double>* areas;
    cape_handle_s::Buffer<unsigned char>* work;
    // what run_map_match records of the call: the frames (or slots) the results cover -- 0 while the buffers may change hands --,
    // the map planes of the call, whether it kept the dense table
    int *resultFrames, *matchN;
    bool* matchAreas;
};
// what differs between the map matchers
struct MapMatchCall
{
    int n;                // frames (or slots) of the call
    int layoutFrames;     // frames the buffers and the work layout are sized for: max_batch, or the call's slots
    const double* poses;  // n x 16, or null: the identity
    const uint32_t* skip; // the caller's words, or null
    uint32_t flags;
    bool growToCall = false;              // buffers grown to the call behind drain_handle (shards); else allocated once, for max_batch
    int planesPerFrame = CAPE_MAX_PLANES; // kept planes of a frame at most: 64, or 128 over the frame's record chain (wide)
    const void* shards = nullptr;         // the planes come out of gathered shards of these layouts instead of the handle's records
    const cape_gather_layout* shardLayout = nullptr;
    const cape_gather_polygon_layout* polygonLayout = nullptr;
    int chainBase = 0; // cape_map_step: the call's frame 0 is this frame of the batch
    cape_handle_s::LastMapMatcher tag = cape_handle_s::kNoMapMatch;
    MapMatchBuffers b{};
    // the sizes of the call (prepare_map_match): its bytes in the pose buffer, the work list's entries and the work layout
    size_t poseBytes = 0, skipBytes = 0, cap = 0;
    MapWorkLayout lay{};

    bool wide() const { return b.framesWide != nullptr; }
    bool keep_areas() const { return (flags & CAPE_MATCH_MAP_AREAS) != 0; }
    size_t area_doubles(int nMap) const { return (size_t)n * nMap * planesPerFrame; }
};

// cape_match_map_wide's call on the handle's MapWide group: the batch's first n frames, or, with a chain base, cape_map_step's one
inline MapMatchCall wide_map_match_call(cape_handle_s* h, int n, const double* poses, const uint32_t* skip, uint32_t flags)
{
    auto& W = h->mapWide;
    MapMatchCall c{n, h->cfg.max_batch, poses, skip, flags};
    c.planesPerFrame = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    c.tag = cape_handle_s::kMapMatchWide;
    c.b = {&W.poses, &W.posesTwin, nullptr, &W.frames, &W.match, &W.planes, &W.kept, &W.areas, &W.work, &W.matchFrames, &W.matchN, &W.matchAreas};
    return c;
}

// the checks the matchers share once their own arguments are through: a map, the flags, the 1 GiB budget of the dense table
inline int check_map_match(const cape_handle_s* h, const MapMatchCall& c, const char* budgetMessage)
{
    if (h->maps.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (c.flags & ~kMatchMapFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match flag");
    if (c.keep_areas() && c.area_doubles(h->maps.n) * sizeof(double) > kMapAreasBudget)
        return fail(CAPE_ERR_CAPACITY, budgetMessage);
    return CAPE_OK;
}

// every buffer of the call, sized before anything is enqueued (behind drain_handle where one is replaced: an earlier call may
// still be working in it)
inline int prepare_map_match(cape_handle_s* h, MapMatchCall& c)
{
    const int nMap = h->maps.n;
    const size_t B = (size_t)c.layoutFrames, P = (size_t)c.planesPerFrame;
    c.poseBytes = (size_t)c.n * 16 * sizeof(double);
    c.skipBytes = c.skip ? (size_t)c.n * ((nMap + 31) / 32) * sizeof(uint32_t) : 0;
    c.cap = std::min(B * (size_t)std::max(nMap, 1) * P, kMapWorkMax);
    c.lay = map_work_layout(c.layoutFrames, c.cap, (c.planesPerFrame + 63) / 64); // a bit per kept plane in a map plane's gate mask
    const size_t poseCapacity = B * 16 * sizeof(double) + B * (CAPE_MAP_MAX_PLANES / 32) * sizeof(uint32_t);
    const auto drain = [h] { return drain_handle(h); };
    const auto sized = [&](auto* buffer, size_t n) { return !buffer ? hipSuccess : c.growToCall ? buffer->grow(n, drain) : buffer->ensure(n); };
    if (c.growToCall && c.b.poses->size() < c.poseBytes + c.skipBytes)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        *c.b.twin = PinnedTwin{};
        CAPE_HIP_TRY(c.b.poses->alloc(poseCapacity));
    }
    CAPE_HIP_TRY(sized(c.b.frames, B));
    CAPE_HIP_TRY(sized(c.b.framesWide, B));
    CAPE_HIP_TRY(sized(c.b.match, B * (c.growToCall ? (size_t)std::max(nMap, 1) : (size_t)CAPE_MAP_MAX_PLANES)));
    CAPE_HIP_TRY(sized(c.b.planes, 2 * B * P));
    CAPE_HIP_TRY(sized(c.b.kept, B * P));
    CAPE_HIP_TRY(c.b.poses->ensure(poseCapacity));
    CAPE_HIP_TRY(c.b.work->grow(c.lay.total, drain));
    if (c.keep_areas())
        CAPE_HIP_TRY(c.b.areas->grow(c.area_doubles(nMap), drain));
    return CAPE_OK;
}

// The poses, then the skip words, through the pinned twin (n x 16 doubles, then n x skipWords words: read before the call returns,
// like cape_match_polygons_pose's), the kernels' parameters bound to the front map and the call's buffers, and the launch.
// `between` runs behind the upload and ahead of the gate with the bound parameters: cape_map_step_visible decides the skip words
// there, from the pose row the gate reads.
template <typename Between> int enqueue_map_match(cape_handle_s* h, const MapMatchCall& c, const uint32_t* deviceSkip, hipStream_t stream, Between between)
{
    auto& poses = *c.b.poses;
    CAPE_HIP_TRY(c.b.twin->upload(poses, c.poseBytes + c.skipBytes, poses.size(), stream,
                                  [&](void* stage) { fill_poses(stage, c.n, c.poses, c.poseBytes, c.skip, c.skipBytes); }));
    const auto& front = h->maps.front;
    unsigned char* work = c.b.work->get();
    cape::MatchMapParams p{};
    if (c.shards)
    {
        const cape_gather_layout& L = *c.shardLayout;
        const cape_gather_polygon_layout& PL = *c.polygonLayout;
        p.shards = static_cast<const unsigned char*>(c.shards);
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
    }
    else
    {
        p.records = h->res.records;
        p.polygons = h->poly.polygons;
        p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
        p.boundaryCapacity = h->boundaryCap;
    }
    if (c.wide())
    {
        // the planes of a frame's whole record chain: the spill pool lies behind the batch
        p.maxBatch = h->cfg.max_batch;
        p.nRecords = h->cfg.max_batch + h->chain.spillRecords;
        p.framesWide = c.b.framesWide->get();
        p.segCur = c.b.planes->get();
        p.mapOf = c.b.planes->get() + (size_t)c.layoutFrames * (size_t)c.planesPerFrame;
    }
    p.chainBase = c.chainBase;
    p.mapPlanes = front.planes;
    p.mapRings = front.rings;
    p.mapVertices = reinterpret_cast<const double2*>(front.vertices.get());
    p.nMap = h->maps.n;
    p.skipWords = (h->maps.n + 31) / 32;
    p.poses = reinterpret_cast<const double*>(poses.get());
    p.skip = deviceSkip ? deviceSkip : c.skipBytes ? reinterpret_cast<const uint32_t*>(poses + c.poseBytes) : nullptr;
    p.frames = c.b.frames ? c.b.frames->get() : nullptr;
    p.match = c.b.match->get();
    p.keptIndex = c.b.kept ? c.b.kept->get() : nullptr;
    p.areas = c.keep_areas() ? c.b.areas->get() : nullptr;
    p.list = bind_pair_list(work, c.lay, c.cap);
    p.gateMasks = reinterpret_cast<unsigned long long*>(work + c.lay.masks);
    p.computeUnits = h->computeUnits;
    p.ldsLimitBytes = h->ldsLimit;
    set_match_thresholds(p, c.flags);
    if (const int rc = between(p); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(c.wide() ? cape::launch_match_map_wide(p, c.n, stream) : cape::launch_match_map(p, c.n, stream));
    h->lastMapMatcher = c.tag; // (cape_debug_map_match_lists: whose work buffer holds the counters of the last call)
    return CAPE_OK;
}

// One map-matcher call behind its entry point's own checks: the device words of CAPE_MATCH_MAP_DEVICE_SKIP, then prepare and
// enqueue on the caller's stream.  settle: the call reads record chains, which a one-frame handle may still have to finish.
inline int run_map_match(cape_handle_s* h, MapMatchCall& c, bool settle, void* stream_)
{
    const uint32_t* deviceSkip = nullptr;
    if (c.flags & CAPE_MATCH_MAP_DEVICE_SKIP)
        if (const int rc = device_skip_words(h, c.n, c.skip, &deviceSkip); rc != CAPE_OK)
            return rc;
    if (c.n == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    if (settle)
        CAPE_SETTLE_RESULTS(h);
    *c.b.resultFrames = 0; // (the buffers of the last call's results may be replaced below)
    if (const int rc = prepare_map_match(h, c); rc != CAPE_OK)
        return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (const int rc = enqueue_map_match(h, c, deviceSkip, stream, [](cape::MatchMapParams&) { return CAPE_OK; }); rc != CAPE_OK)
        return rc;
    *c.b.resultFrames = c.n;
    *c.b.matchN = h->maps.n;
    *c.b.matchAreas = c.keep_areas();
    return CAPE_OK;
}

// ---- a changed map

struct MapSizes
{
    int planes = 0, rings = 0;
    long long vertices = 0;
};

// `from` holds the new map, of these sizes, with its tracks and their ids: it changes places with the front set
inline void adopt_map(cape_handle_s* h, MapSet& from, const MapSizes& sizes)
{
    auto& M = h->maps;
    M.front.swap(from);
    M.n = sizes.planes;
    M.nRings = sizes.rings;
    M.nVertices = sizes.vertices;
    M.tracksN = sizes.planes; // the set's tracks are those of the new map
}

// What a changed map invalidates, for every call that changes it: the words cape_map_visibility decided for the old map, the wide
// match against it and what cape_map_kalman (and with it the unions) and the pose stage made of that.  An upload brings no tracks, and ends the words
// of cape_map_step_visible too; behind a commit, a maintenance or a step those words stay readable -- they stand for the map that
// step found -- and the new set's tracks are current (adopt_map).
inline void invalidate_for_new_map(cape_handle_s* h, bool uploaded = false)
{
    h->visibility.frames = 0;
    h->kalman.matchedThisMap = false;
    invalidate_frame_results(h);
    if (uploaded)
    {
        h->mapStepVisible.n = -1;
        h->maps.tracksN = -1;
    }
}

// the maintenance's parameters: `from` with a map of `sizes` -> `to`, which takes as much; the log's arrays, plan and header.
// cape_map_step passes no sizes and of the log only what it holds: its kernels read the rest off the commit's header
inline cape::MapMaintainParams bind_map_maintain(const cape_handle_s* h, const MapSet& from, const MapSet& to, const MapSizes& sizes,
                                                 const cape::MaintainLog& log, cape::MaintainPlanRow* plan, cape_map_maintain_result* header)
{
    const auto& R = h->mapMaintain;
    cape::MapMaintainParams p{};
    p.mapPlanes = from.planes;
    p.mapRings = from.rings;
    p.mapVertices = from.vertices;
    p.tracks = from.tracks;
    p.tags = from.tags;
    p.nMap = sizes.planes;
    p.nMapRings = sizes.rings;
    p.nMapVertices = sizes.vertices;
    p.outPlanes = to.planes;
    p.outRings = to.rings;
    p.outVertices = to.vertices;
    p.outTracks = to.tracks;
    p.outTags = to.tags;
    p.planesCapacity = (unsigned long long)sizes.planes;
    p.ringsCapacity = (unsigned long long)sizes.rings;
    p.verticesCapacity = (unsigned long long)sizes.vertices;
    p.logPlanes = R.planes;
    p.logRings = R.rings;
    p.logVertices = R.vertices;
    p.logTracks = R.tracks;
    p.log = log;
    p.plan = plan;
    p.header = header;
    return p;
}

} // namespace cape::abi

#endif // CAPE_API_MAP_LAYOUTS_ONLY
