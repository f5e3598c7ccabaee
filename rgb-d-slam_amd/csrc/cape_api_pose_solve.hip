// C ABI, host side: the pose solver between the match and the update -- Levenberg-Marquardt per (frame, hypothesis) on the frame's
// map matches, the RANSAC bookkeeping over the scored hypotheses and the refit from the selection (cape_pose_solve.hip).  It reads what
// cape_map_pose_score reads, that call's score rows for the selection, and writes only the buffers of cape_handle_s::PoseSolve.
#include <algorithm>
#include <cstring>

#include "cape_api_map.h"

using namespace cape::abi;

namespace {

constexpr uint32_t kPoseSolveFlags = CAPE_POSE_SOLVE_DEVICE_INPUT | CAPE_POSE_SOLVE_FROM_SELECTION;

} // namespace

extern "C" {

int cape_map_pose_solve(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* x0, const uint32_t* subsets,
                        const cape_pose_solve_params* params, uint32_t flags, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    // (what needs no handle comes first)
    if (n_hypotheses < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "n_hypotheses must be at least 1");
    if (flags & ~kPoseSolveFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown pose-solve flag");
    const bool fromSelection = (flags & CAPE_POSE_SOLVE_FROM_SELECTION) != 0, deviceInput = (flags & CAPE_POSE_SOLVE_DEVICE_INPUT) != 0;
    if (fromSelection && n_hypotheses != 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_POSE_SOLVE_FROM_SELECTION solves one problem per frame: n_hypotheses must be 1");
    cape::PoseSolveSettings settings;
    if (!cape::pose_solve_settings(params, settings))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "a pose-solve parameter is NaN, negative or out of range");
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (!fromSelection && n_frames > 0 && (!x0 || !subsets))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null x0 or subsets");
    auto& P = h->poseSolve;
    const auto& W = h->mapWide;
    const int nMap = h->maps.n;
    const int selectFrames = pose_selection_live(h) ? P.selectFrames : 0;
    P.frames = 0;
    if (!fromSelection) // (the selection was made over the rows this call replaces)
        P.selectFrames = 0;
    if (nMap < 0 || h->maps.tracksN != nMap)
        return fail(CAPE_ERR_CAPACITY, "no tracks for the uploaded map (cape_map_upload, then cape_map_upload_tracks)");
    if (!h->kalman.matchedThisMap || W.matchN != nMap || n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "no cape_match_map_wide of the current batch against the uploaded map covers n_frames");
    if (fromSelection && n_frames > selectFrames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_select covers n_frames");
    const size_t rowsPerFrame = (size_t)n_hypotheses, rows = (size_t)n_frames * rowsPerFrame;
    if ((rowsPerFrame + cape::kPoseSolveGroupProblems - 1) / cape::kPoseSolveGroupProblems > 65535)
        return fail(CAPE_ERR_CAPACITY, "more than 65 535 x 256 hypotheses per frame");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    const size_t x0Bytes = rows * 6 * sizeof(double), inputBytes = x0Bytes + rows * 4 * sizeof(uint32_t);
    const bool upload = !fromSelection && !deviceInput;
    if (upload && P.input.size() < inputBytes)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        P.inputTwin = PinnedTwin{};
        CAPE_HIP_TRY(P.input.alloc(inputBytes));
    }
    CAPE_HIP_TRY(P.frameInfo.grow((size_t)n_frames, drain));
    CAPE_HIP_TRY(P.features.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(P.solutions.grow(rows, drain));
    CAPE_HIP_TRY(P.poses.grow(rows * 16, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (upload)
        CAPE_HIP_TRY(P.inputTwin.upload(P.input, inputBytes, P.input.size(), stream, [&](void* stage) {
            std::memcpy(stage, x0, x0Bytes);
            std::memcpy(static_cast<unsigned char*>(stage) + x0Bytes, subsets, inputBytes - x0Bytes);
        }));
    // ---- the frame's pairs and feature rows: the pairs kernel of cape_map_pose_score, into this call's rows
    cape::PoseScoreParams pairs{};
    pairs.mapPlanes = h->maps.front.planes;
    pairs.tracks = h->maps.front.tracks;
    pairs.tags = h->maps.front.tags;
    pairs.nMap = nMap;
    pairs.matchFrames = W.frames;
    pairs.match = W.match;
    pairs.kept = W.kept;
    pairs.records = h->res.records;
    pairs.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the batch's records, then the spill pool's)
    pairs.frameInfo = P.frameInfo;
    pairs.features = P.features;
    CAPE_HIP_TRY(cape::launch_map_pose_pairs(pairs, n_frames, stream));
    cape::PoseSolveParams p{};
    p.frameInfo = P.frameInfo;
    p.features = P.features;
    if (fromSelection)
        p.selection = P.selection;
    else if (deviceInput)
        p.x0 = x0, p.subsets = subsets;
    else
    {
        p.x0 = reinterpret_cast<const double*>(P.input.get());
        p.subsets = reinterpret_cast<const uint32_t*>(P.input.get() + x0Bytes);
    }
    p.nProblems = n_hypotheses;
    p.settings = settings;
    p.solutions = P.solutions;
    p.poses = P.poses;
    CAPE_HIP_TRY(cape::launch_map_pose_solve(p, n_frames, stream));
    P.frames = n_frames;
    P.problems = n_hypotheses;
    P.fromSelection = fromSelection;
    return CAPE_OK;
}

int cape_copy_pose_solutions(cape_handle h, int32_t n_frames, cape_pose_solution* solutions, double* world_to_camera)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& P = h->poseSolve;
    if (n_frames > (pose_solutions_live(h) ? P.frames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_pose_solve on the current batch, map, tracks and match");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t rows = (size_t)n_frames * (size_t)P.problems;
    CAPE_HIP_TRY(copy_out(solutions, P.solutions, 0, rows));
    CAPE_HIP_TRY(copy_out(world_to_camera, P.poses, 0, rows * 16));
    return CAPE_OK;
}

int cape_pose_solve_device(cape_handle h, const cape_pose_solution** solutions, const double** world_to_camera)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!pose_solutions_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_pose_solve has run on the current batch, map, tracks and match");
    if (solutions)
        *solutions = h->poseSolve.solutions;
    if (world_to_camera)
        *world_to_camera = h->poseSolve.poses;
    return CAPE_OK;
}

int cape_map_pose_select(cape_handle h, int32_t n_frames, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& P = h->poseSolve;
    const auto& S = h->poseScore;
    P.selectFrames = 0;
    if (!pose_solutions_live(h) || P.fromSelection || n_frames > P.frames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_solve over hypotheses covers n_frames");
    if (!pose_scores_live(h) || n_frames > S.frames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_score covers n_frames");
    if (S.hypotheses != P.problems)
        return fail(CAPE_ERR_CAPACITY, "the current cape_map_pose_score and cape_map_pose_solve differ in n_hypotheses");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); };
    CAPE_HIP_TRY(P.selection.grow((size_t)n_frames, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::PoseSelectParams p{};
    p.scores = S.scores;
    p.solutions = P.solutions;
    p.nHypotheses = P.problems;
    p.selection = P.selection;
    CAPE_HIP_TRY(cape::launch_map_pose_select(p, n_frames, stream));
    P.selectFrames = n_frames;
    return CAPE_OK;
}

int cape_copy_pose_selection(cape_handle h, int32_t n_frames, cape_pose_selection* selection)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& P = h->poseSolve;
    if (n_frames > (pose_selection_live(h) ? P.selectFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_pose_select on the current batch, map, tracks and match");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(selection, P.selection, 0, (size_t)n_frames));
    return CAPE_OK;
}

} // extern "C"
