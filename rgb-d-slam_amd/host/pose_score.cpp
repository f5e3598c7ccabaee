// cape_host_pose_score (cape_host_map.h): the host twin of cape_map_pose_score for ONE frame -- the pair list, the feature rows and
// every hypothesis' sums through the statements of csrc/cape_pose_score.h, which the device kernels compile too; the map plane goes
// through utils::plane_to_camera of the host class.  Serial: pair after pair, hypothesis after hypothesis.
#include <cstring>
#include <limits>
#include <vector>

#include "boundary_polygon.hpp"
#include "cape_hip.h"
#include "cape_host_map.h"
#include "../csrc/cape_pose_score.h" // the rules, shared with the kernels

extern "C" int cape_host_pose_score(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                                    int32_t n_hypotheses, const double* world_to_camera, cape_pose_score* scores_out,
                                    cape_pose_feature* features_out, double* residuals_out)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    if (!map || !detected || map->n_planes < 0 || detected->n < 0 || detected->n > WP || n_hypotheses < 1 || !world_to_camera ||
        (frame_flags & ~(uint32_t)CAPE_MATCH_EXACT_OVERFLOW))
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
    // ---- the pairs and their feature rows
    std::vector<int32_t> pairs((size_t)WP);
    const int nPairs = nMap > 0 ? cape::pose_pairs_serial(match, nMap, pairs.data()) : 0;
    std::vector<cape_pose_feature> features((size_t)WP);
    std::memset(features.data(), 0, features.size() * sizeof(cape_pose_feature));
    int32_t nInvalid = 0;
    for (int k = 0; k < nPairs; ++k)
    {
        const int32_t j = pairs[k], i = match[j];
        cape_pose_feature& F = features[k];
        const cape_map_plane& M = map->planes[j];
        for (int c = 0; c < 4; ++c)
            F.matched[c] = detected->planes[4 * (size_t)i + c];
        F.map_plane[0] = M.normal[0], F.map_plane[1] = M.normal[1], F.map_plane[2] = M.normal[2], F.map_plane[3] = M.d;
        cape::pose_feature_stddev(map->tracks[j].covariance, F.stddev);
        F.map_id = map->tracks[j].id;
        F.map_index = j;
        F.kept_plane = i;
        nInvalid += cape::pose_feature_valid(F) ? 0 : 1;
    }
    if (features_out)
        std::memcpy(features_out, features.data(), features.size() * sizeof(cape_pose_feature));
    if (residuals_out)
        std::memset(residuals_out, 0, (size_t)n_hypotheses * WP * 7 * sizeof(double));
    // ---- every hypothesis over the pairs in order
    for (int32_t h = 0; h < n_hypotheses; ++h)
    {
        const double* T = world_to_camera + 16 * (size_t)h;
        cape::PoseScoreSums S;
        for (int k = 0; k < nPairs; ++k)
        {
            const cape_pose_feature& F = features[k];
            double qn[3], qd;
            rgbd_slam::utils::plane_to_camera(F.map_plane, F.map_plane[3], T, qn, &qd);
            double signedDistance[4], reduced[3];
            cape::pose_pair_distances(F.matched, F.matched[3], qn, qd, signedDistance, reduced);
            cape::pose_score_add(S, F.kept_plane, signedDistance, reduced);
            if (residuals_out)
            {
                double* r = residuals_out + ((size_t)h * WP + k) * 7;
                for (int c = 0; c < 4; ++c)
                    r[c] = signedDistance[c];
                for (int c = 0; c < 3; ++c)
                    r[4 + c] = reduced[c];
            }
        }
        if (scores_out)
            scores_out[h] = cape::pose_score_row(S, nPairs, nInvalid, frame_flags & CAPE_MATCH_EXACT_OVERFLOW);
    }
    return CAPE_OK;
}
