// C ABI, host side: the device map as data -- upload, tracks, sizes, download -- and the calls that read it without changing it:
// the three map matchers (N2 against a persistent map; their one body is cape_api_map.h's) and the visibility words.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "cape_api_map.h"

using namespace cape::abi;

namespace {

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

constexpr const char* kFewerFrames = "the inter-area table of this call would exceed 1 GiB (fewer frames per call, or no CAPE_MATCH_MAP_AREAS)";

// What the three cape_copy_*map_matches* share behind the entry point's own check: the two refusals (the results cover `live` frames
// or slots; the call kept the dense table or not), the drain and the copies of the three tables every map matcher writes -- rows of
// matchN map planes, the dense table planesPerFrame wide
template <typename Frame>
int copy_map_matches(cape_handle_s* h, int32_t n, int live, bool keptAreas, size_t matchN, size_t planesPerFrame, const char* beyond, const char* noAreas,
                     const cape_handle_s::Buffer<Frame>& framesOf, const cape_handle_s::Buffer<int32_t>& matchOf,
                     const cape_handle_s::Buffer<double>& areasOf, Frame* frames, int32_t* match, double* inter_area)
{
    if (n > live)
        return fail(CAPE_ERR_CAPACITY, beyond);
    if (inter_area && n > 0 && !keptAreas)
        return fail(CAPE_ERR_INVALID_ARGUMENT, noAreas);
    if (n == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(frames, framesOf, 0, (size_t)n));
    CAPE_HIP_TRY(copy_out(match, matchOf, 0, (size_t)n * matchN));
    CAPE_HIP_TRY(copy_out(inter_area, areasOf, 0, (size_t)n * matchN * planesPerFrame));
    return CAPE_OK;
}

} // namespace

extern "C" {

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
    auto& M = h->maps;
    M.n = -1; // (no map until the copies are through)
    invalidate_for_new_map(h, true);
    // (the front set's planes, rings and vertices at their exact sizes; its tracks are cape_map_upload_tracks')
    const auto drained = [] { return hipSuccess; };
    CAPE_HIP_TRY(M.front.planes.grow(P.size(), drained));
    CAPE_HIP_TRY(M.front.rings.grow(R.size(), drained));
    CAPE_HIP_TRY(M.front.vertices.grow(V.size(), drained));
    if (!P.empty())
    {
        CAPE_HIP_TRY(hipMemcpy(M.front.planes, P.data(), P.size() * sizeof(cape_map_plane), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(M.front.rings, R.data(), R.size() * sizeof(cape_map_ring), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(M.front.vertices, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    M.n = n_planes;
    M.nRings = (int)R.size(); // (what the ring and vertex buffers hold)
    M.nVertices = (long long)(V.size() / 2);
    return CAPE_OK;
}

int cape_map_upload_tracks(cape_handle h, const cape_map_track* tracks, int32_t n)
{
    if (!h || n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative count");
    if (h->maps.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (n != h->maps.n)
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
    auto& M = h->maps;
    M.tracksN = -1;
    invalidate_frame_results(h);
    CAPE_HIP_TRY(M.front.tracks.grow(T.size(), [] { return hipSuccess; }));
    CAPE_HIP_TRY(M.front.tags.grow(G.size(), [] { return hipSuccess; }));
    if (n > 0)
    {
        CAPE_HIP_TRY(hipMemcpy(M.front.tracks, T.data(), T.size() * sizeof(cape::MapTrackState), hipMemcpyHostToDevice));
        CAPE_HIP_TRY(hipMemcpy(M.front.tags, G.data(), G.size() * sizeof(cape::MapTrackTag), hipMemcpyHostToDevice));
    }
    M.tracksN = n;
    return CAPE_OK;
}

int cape_map_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (h->maps.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (n_planes)
        *n_planes = h->maps.n;
    if (n_rings)
        *n_rings = h->maps.nRings;
    if (n_vertices)
        *n_vertices = h->maps.nVertices;
    return CAPE_OK;
}

int cape_map_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                      double* vertices, int64_t vertices_capacity, cape_map_track* tracks)
{
    if (!h || planes_capacity < 0 || rings_capacity < 0 || vertices_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& M = h->maps;
    if (M.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (M.n > planes_capacity || M.nRings > rings_capacity || M.nVertices > vertices_capacity)
        return fail(CAPE_ERR_CAPACITY, "an array is too small for the device map (cape_map_info tells its sizes)");
    if ((M.n > 0 && !planes) || (M.nRings > 0 && !rings) || (M.nVertices > 0 && !vertices))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)M.n;
    if (n == 0)
        return CAPE_OK;
    CAPE_HIP_TRY(hipMemcpy(planes, M.front.planes, n * sizeof(cape_map_plane), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(rings, M.front.rings, (size_t)M.nRings * sizeof(cape_map_ring), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(vertices, M.front.vertices, (size_t)M.nVertices * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (tracks)
    {
        std::memset(tracks, 0, n * sizeof(cape_map_track)); // (the zero track per plane if none were uploaded for this map)
        if (M.tracksN == M.n)
        {
            std::vector<cape::MapTrackState> T(n);
            std::vector<cape::MapTrackTag> G(n);
            CAPE_HIP_TRY(hipMemcpy(T.data(), M.front.tracks, n * sizeof(cape::MapTrackState), hipMemcpyDeviceToHost));
            CAPE_HIP_TRY(hipMemcpy(G.data(), M.front.tags, n * sizeof(cape::MapTrackTag), hipMemcpyDeviceToHost));
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

int cape_match_map(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& map = h->map;
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    MapMatchCall c{n_frames, h->cfg.max_batch, world_to_camera, skip, flags};
    c.tag = cape_handle_s::kMapMatchRecords;
    c.b = {&map.poses, &map.posesTwin, &map.frames, nullptr, &map.match, nullptr, nullptr, &map.areas, &map.work, &map.matchFrames, &map.matchN, &map.matchAreas};
    if (const int rc = check_map_match(h, c, kFewerFrames); rc != CAPE_OK)
        return rc;
    map.matchFrames = 0;
    return run_map_match(h, c, false, stream);
}

int cape_copy_map_matches(cape_handle h, int32_t n_frames, cape_frame_map_match* frames, int32_t* match, double* inter_area)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& map = h->map;
    return copy_map_matches(h, n_frames, map.matchFrames, map.matchAreas, map.matchN, CAPE_MAX_PLANES,
                            "n_frames exceeds the frames of the last cape_match_map of the current batch",
                            "the last cape_match_map did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)", map.frames, map.match, map.areas,
                            frames, match, inter_area);
}

int cape_match_map_wide(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, uint32_t flags, void* stream)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& W = h->mapWide;
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    MapMatchCall c = wide_map_match_call(h, n_frames, world_to_camera, skip, flags);
    if (const int rc = check_map_match(h, c, kFewerFrames); rc != CAPE_OK)
        return rc;
    W.matchFrames = 0;
    invalidate_frame_results(h); // (cape_map_kalman's and cape_map_pose_score's results belong to the match this call replaces)
    if (const int rc = run_map_match(h, c, true, stream); rc != CAPE_OK || n_frames == 0)
        return rc;
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
    if (const int rc = copy_map_matches(h, n_frames, W.matchFrames, W.matchAreas, W.matchN, WP,
                                        "n_frames exceeds the frames of the last cape_match_map_wide of the current batch",
                                        "the last cape_match_map_wide did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)", W.frames, W.match,
                                        W.areas, frames, match, inter_area);
        rc != CAPE_OK || n_frames == 0)
        return rc;
    CAPE_ON_DEVICE(h); // (drained above: the two tables of the wide kernels)
    CAPE_HIP_TRY(copy_out(seg_cur, W.planes, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(map_of, W.planes, (size_t)h->cfg.max_batch * WP, (size_t)n_frames * WP));
    return CAPE_OK;
}

int cape_match_map_shards(cape_handle h, const void* shards_dev, int32_t n_shards, const cape_gather_layout* layout,
                          const cape_gather_polygon_layout* polygon_layout, const double* world_to_camera, const uint32_t* skip,
                          uint32_t flags, void* stream)
{
    if (!h || !shards_dev || !layout || !polygon_layout || n_shards < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, shards or layout, or fewer than one shard");
    auto& S = h->shardMatch;
    MapMatchCall c{0, 0, world_to_camera, skip, flags}; // (its slots: once the layout is through)
    c.growToCall = true;
    c.shards = shards_dev;
    c.shardLayout = layout;
    c.polygonLayout = polygon_layout;
    c.tag = cape_handle_s::kMapMatchShards;
    c.b = {&S.poses, &S.posesTwin, &S.frames, nullptr, &S.match, nullptr, &S.kept, &S.areas, &S.work, &S.slots, &S.matchN, &S.matchAreas};
    constexpr const char* kFewerShards = "the inter-area table of this call would exceed 1 GiB (fewer shards per call, or no CAPE_MATCH_MAP_AREAS)";
    if (const int rc = check_map_match(h, c, kFewerShards); rc != CAPE_OK) // (the map and the flags: the table once the slots are known)
        return rc;
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
    c.n = c.layoutFrames = n_shards * L.frames_capacity; // the call's slots: nothing here depends on max_batch
    if (const int rc = check_map_match(h, c, kFewerShards); rc != CAPE_OK)
        return rc;
    return run_map_match(h, c, false, stream);
}

int cape_copy_shard_map_matches(cape_handle h, int32_t n_slots, cape_frame_map_match* frames, int32_t* match, double* inter_area)
{
    if (!h || n_slots < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad argument");
    const auto& S = h->shardMatch;
    return copy_map_matches(h, n_slots, S.slots, S.matchAreas, S.matchN, CAPE_MAX_PLANES, "n_slots exceeds the slots of the last cape_match_map_shards",
                            "the last cape_match_map_shards did not keep the inter-area table (CAPE_MATCH_MAP_AREAS)", S.frames, S.match, S.areas,
                            frames, match, inter_area);
}

int cape_map_visibility(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* moving, void* stream_)
{
    if (!h || n_frames < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or fewer than one frame");
    if (h->maps.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    auto& V = h->visibility;
    const int nMap = h->maps.n;
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
    cape::MapVisibilityParams p = bind_map_visibility(h, V.work, lay, cap);
    p.poses = reinterpret_cast<const double*>(V.poses.get());
    p.moving = movingBytes ? reinterpret_cast<const uint32_t*>(V.poses + poseBytes) : nullptr;
    p.skip = V.skip;
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

} // extern "C"
