// The pairs of ONE frame for the host twins of the pose stage (pose_score.cpp, pose_solve.cpp, pose_covariance.cpp): the argument
// checks on the map, the match and the detected planes, the pair list, the feature rows and what the solve reads of them -- what the
// device's pairs kernel and pose_rows_stage make, through the same statements of csrc/cape_pose_score.h and csrc/cape_pose_solve.h.
#pragma once
#include <cstdint>
#include <vector>

#include "cape_hip.h"
#include "cape_host_map.h"
#include "../csrc/cape_pose_solve.h" // the rules, shared with the kernels

namespace cape_host {

struct PosePairs
{
    std::vector<cape_pose_feature> features; // 128 rows, zeros at and beyond nPairs
    std::vector<double> planes;              // PoseSolveRows::planes: 8 per pair
    std::vector<int> kept;                   // PoseSolveRows::kept
    int32_t nPairs = 0, nInvalid = 0;
};

// CAPE_ERR_INVALID_ARGUMENT for a null or negative-sized map or plane table, more than 128 detected planes, a frame flag other than
// CAPE_MATCH_EXACT_OVERFLOW, a missing array and a match entry outside [-1, detected->n)
inline int build_pose_pairs(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags, PosePairs& out)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    if (!map || !detected || map->n_planes < 0 || detected->n < 0 || detected->n > WP || (frame_flags & ~(uint32_t)CAPE_MATCH_EXACT_OVERFLOW))
        return CAPE_ERR_INVALID_ARGUMENT;
    const bool reports = !(frame_flags & CAPE_MATCH_EXACT_OVERFLOW);
    const int32_t nMap = reports ? map->n_planes : 0;
    if (nMap > 0 && (!map->planes || !map->tracks || !match))
        return CAPE_ERR_INVALID_ARGUMENT;
    if (detected->n > 0 && !detected->planes)
        return CAPE_ERR_INVALID_ARGUMENT;
    for (int32_t j = 0; j < nMap; ++j)
        if (match[j] < -1 || match[j] >= detected->n)
            return CAPE_ERR_INVALID_ARGUMENT;
    std::vector<int32_t> pairs((size_t)WP);
    out.nPairs = nMap > 0 ? cape::pose_pairs_serial(match, nMap, pairs.data()) : 0;
    out.nInvalid = 0;
    out.features.assign((size_t)WP, cape_pose_feature{});
    out.planes.assign((size_t)WP * 8, 0.0);
    out.kept.assign((size_t)WP, 0);
    for (int k = 0; k < out.nPairs; ++k)
    {
        const int32_t j = pairs[k], i = match[j];
        cape_pose_feature& F = out.features[k];
        const cape_map_plane& M = map->planes[j];
        for (int c = 0; c < 4; ++c)
            F.matched[c] = detected->planes[4 * (size_t)i + c];
        F.map_plane[0] = M.normal[0], F.map_plane[1] = M.normal[1], F.map_plane[2] = M.normal[2], F.map_plane[3] = M.d;
        cape::pose_feature_stddev(map->tracks[j].covariance, F.stddev);
        F.map_id = map->tracks[j].id;
        F.map_index = j;
        F.kept_plane = i;
        out.nInvalid += cape::pose_feature_valid(F) ? 0 : 1;
        cape::pose_rows_fill(F, k, out.planes.data(), out.kept.data());
    }
    return CAPE_OK;
}

} // namespace cape_host
