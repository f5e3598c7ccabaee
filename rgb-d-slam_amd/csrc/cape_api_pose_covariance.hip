// C ABI, host side: the pose's covariance behind the refit -- compute_pose_variance as vary, solve on the varied planes and reduce
// (cape_pose_covariance.hip).  It reads what cape_map_pose_solve reads and, with CAPE_POSE_COVARIANCE_FROM_SOLUTION, that call's refit rows
// and selection in device memory; it writes the buffers of cape_handle_s::PoseCovariance and, where they are not current, the stage's pair
// rows (enqueue_pose_pairs).
#include <algorithm>
#include <cstring>

#include "cape_api_pose.h"

using namespace cape::abi;

namespace {

constexpr uint32_t kPoseCovarianceFlags = CAPE_POSE_COVARIANCE_DEVICE_INPUT | CAPE_POSE_COVARIANCE_FROM_SOLUTION | CAPE_POSE_COVARIANCE_TABLE |
                                          CAPE_POSE_COVARIANCE_KEEP_SAMPLES;
constexpr uint32_t kPoseDrawFlags = CAPE_POSE_COVARIANCE_DEVICE_INPUT | CAPE_POSE_DRAW_UNIFORMS;
constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;

} // namespace

extern "C" {

int cape_map_pose_covariance(cape_handle h, int32_t n_frames, int32_t n_iterations, const double* x, const uint32_t* subsets, const double* deviates,
                             uint64_t seed, uint32_t frame_base, const cape_pose_solve_params* params, uint32_t flags, void* stream_)
{
    // (what needs no handle comes first)
    if (n_iterations < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "n_iterations must be at least 1");
    if (flags & ~kPoseCovarianceFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown pose-covariance flag");
    const bool fromSolution = (flags & CAPE_POSE_COVARIANCE_FROM_SOLUTION) != 0, deviceInput = (flags & CAPE_POSE_COVARIANCE_DEVICE_INPUT) != 0;
    const bool fromTable = (flags & CAPE_POSE_COVARIANCE_TABLE) != 0, keep = (flags & CAPE_POSE_COVARIANCE_KEEP_SAMPLES) != 0;
    if (fromTable && !deviates)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_POSE_COVARIANCE_TABLE with a null table");
    cape::PoseSolveSettings settings;
    if (!cape::pose_solve_settings(params, settings))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "a pose-solve parameter is NaN, negative or out of range");
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (!fromSolution && n_frames > 0 && (!x || !subsets))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null x or subsets");
    auto& P = h->poseCovariance;
    const auto& S = h->poseSolve;
    P.frames = 0;
    if (const int rc = check_pose_inputs(h, n_frames); rc != CAPE_OK)
        return rc;
    if (fromSolution && (!pose_solutions_live(h) || !S.fromSelection || n_frames > S.frames || !pose_selection_live(h) || n_frames > S.selectFrames))
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_solve(CAPE_POSE_SOLVE_FROM_SELECTION) covers n_frames");
    const size_t iterations = (size_t)n_iterations, groups = (iterations + cape::kPoseCovGroupIterations - 1) / cape::kPoseCovGroupIterations;
    if (groups > 65535)
        return fail(CAPE_ERR_CAPACITY, "more than 65 535 x 256 iterations");
    const size_t sampleRows = (size_t)n_frames * iterations;
    if (keep && sampleRows > (size_t)CAPE_POSE_COVARIANCE_MAX_KEPT)
        return fail(CAPE_ERR_CAPACITY, "CAPE_POSE_COVARIANCE_KEEP_SAMPLES beyond CAPE_POSE_COVARIANCE_MAX_KEPT sample rows");
    // the slab: 128 pair slots x 4 doubles x iterations per frame, as many frames as the budget takes
    const unsigned long long budget = P.budget ? P.budget : CAPE_POSE_COVARIANCE_DEFAULT_BUDGET;
    const size_t frameDoubles = WP * 4 * iterations;
    const size_t fit = (size_t)(budget / (frameDoubles * sizeof(double)));
    if (fit == 0)
        return fail(CAPE_ERR_CAPACITY, "one frame's varied planes (4096 x n_iterations bytes) exceed the slab's budget");
    if (n_frames == 0)
        return CAPE_OK;
    const size_t chunk = std::min(fit, (size_t)n_frames);
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    const size_t tableDoubles = iterations * WP * 4;
    const PoseInputRoute route = fromSolution ? PoseInputRoute::kFromResults : deviceInput ? PoseInputRoute::kDevice : PoseInputRoute::kHost;
    const bool uploadTable = fromTable && !deviceInput;
    if (route == PoseInputRoute::kHost)
        if (const int rc = reserve_pose_input(h, P, (size_t)n_frames); rc != CAPE_OK)
            return rc;
    if (uploadTable && P.table.size() < tableDoubles)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        P.tableTwin = PinnedTwin{};
        CAPE_HIP_TRY(P.table.alloc(tableDoubles));
    }
    if (const int rc = reserve_pose_pairs(h); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(P.frameRows.grow((size_t)n_frames * sizeof(cape::PoseCovFrame), drain));
    CAPE_HIP_TRY(P.slab.grow(chunk * frameDoubles, drain));
    CAPE_HIP_TRY(P.samples.grow(sampleRows * sizeof(cape::PoseCovSample), drain));
    if (keep)
        CAPE_HIP_TRY(P.kept.grow(sampleRows, drain));
    CAPE_HIP_TRY(P.rows.grow((size_t)n_frames, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::PoseCovParams p{};
    if (const int rc = bind_pose_input(P, route, (size_t)n_frames, x, subsets, stream, &p.x, &p.subsets); rc != CAPE_OK)
        return rc;
    if (uploadTable)
        CAPE_HIP_TRY(P.tableTwin.upload(P.table, tableDoubles * sizeof(double), P.table.size() * sizeof(double), stream,
                                        [&](void* stage) { std::memcpy(stage, deviates, tableDoubles * sizeof(double)); }));
    if (keep) // (the rows of a refused frame are never written)
        CAPE_HIP_TRY(hipMemsetAsync(P.kept, 0, sampleRows * sizeof(cape_pose_solution), stream));
    if (const int rc = enqueue_pose_pairs(h, n_frames, stream); rc != CAPE_OK)
        return rc;
    p.frameInfo = h->posePairs.frameInfo;
    p.features = h->posePairs.features;
    if (fromSolution)
        p.solutions = S.solutions, p.selection = S.selection;
    p.table = !fromTable ? nullptr : (deviceInput ? deviates : P.table.get());
    p.seed = seed;
    p.frameBase = frame_base;
    p.nIterations = n_iterations;
    p.settings = settings;
    p.frames = reinterpret_cast<cape::PoseCovFrame*>(P.frameRows.get());
    p.slab = P.slab;
    p.samples = reinterpret_cast<cape::PoseCovSample*>(P.samples.get());
    p.kept = keep ? P.kept.get() : nullptr;
    p.rows = P.rows;
    // ---- chunks of frames through the slab, one behind the other on the stream: the sizes are the host's, nothing is waited for
    for (size_t first = 0; first < (size_t)n_frames; first += chunk)
    {
        p.firstFrame = (int)first;
        p.chunkFrames = (int)std::min(chunk, (size_t)n_frames - first);
        CAPE_HIP_TRY(cape::launch_map_pose_covariance_chunk(p, stream));
    }
    CAPE_HIP_TRY(cape::launch_map_pose_covariance_reduce(p, n_frames, stream));
    P.frames = n_frames;
    P.iterations = n_iterations;
    P.keptSamples = keep;
    return CAPE_OK;
}

int cape_copy_pose_covariance(cape_handle h, int32_t n_frames, cape_pose_covariance* rows)
{
    CAPE_POSE_COPY_OUT(h, n_frames, pose_covariance_live(h) ? h->poseCovariance.frames : 0,
                       "n_frames exceeds the frames of the last cape_map_pose_covariance on the current batch, map, tracks and match");
    CAPE_HIP_TRY(copy_out(rows, h->poseCovariance.rows, 0, (size_t)n_frames));
    return CAPE_OK;
}

int cape_copy_pose_covariance_samples(cape_handle h, int32_t n_frames, cape_pose_solution* samples)
{
    CAPE_POSE_COPY_OUT(h, n_frames, pose_covariance_live(h) ? h->poseCovariance.frames : 0,
                       "n_frames exceeds the frames of the last cape_map_pose_covariance on the current batch, map, tracks and match",
                       if (!h->poseCovariance.keptSamples)
                           return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_map_pose_covariance did not keep its samples (CAPE_POSE_COVARIANCE_KEEP_SAMPLES)"));
    const auto& P = h->poseCovariance;
    CAPE_HIP_TRY(copy_out(samples, P.kept, 0, (size_t)n_frames * (size_t)P.iterations));
    return CAPE_OK;
}

int cape_pose_covariance_device(cape_handle h, const cape_pose_covariance** rows)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!pose_covariance_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_pose_covariance has run on the current batch, map, tracks and match");
    if (rows)
        *rows = h->poseCovariance.rows;
    return CAPE_OK;
}

int cape_pose_draw_deviates(cape_handle h, uint64_t seed, uint32_t frame, int32_t n_iterations, double* out, uint32_t flags)
{
    if (!h || !out || n_iterations < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or table, or n_iterations < 1");
    if (flags & ~kPoseDrawFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown draw flag");
    if ((size_t)n_iterations > (size_t)65535 * cape::kPoseCovGroupIterations)
        return fail(CAPE_ERR_CAPACITY, "more than 65 535 x 256 iterations");
    const bool toDevice = (flags & CAPE_POSE_COVARIANCE_DEVICE_INPUT) != 0, uniforms = (flags & CAPE_POSE_DRAW_UNIFORMS) != 0;
    auto& P = h->poseCovariance;
    const size_t doubles = (size_t)n_iterations * WP * 4;
    CAPE_ON_DEVICE(h);
    const auto drain = [h] { return drain_handle(h); };
    if (!toDevice)
        CAPE_HIP_TRY(P.drawn.grow(doubles, drain));
    hipStream_t stream = nullptr;
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        CAPE_HIP_TRY(cape::launch_pose_draw_deviates(seed, frame, n_iterations, uniforms, toDevice ? out : P.drawn.get(), stream));
    }
    CAPE_HIP_TRY(drain_handle(h)); // (synchronous either way: the table is there when the call returns)
    if (!toDevice)
        CAPE_HIP_TRY(hipMemcpy(out, P.drawn.get(), doubles * sizeof(double), hipMemcpyDeviceToHost));
    return CAPE_OK;
}

int cape_set_pose_covariance_budget(cape_handle h, uint64_t bytes)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    h->poseCovariance.budget = bytes;
    return CAPE_OK;
}

} // extern "C"
