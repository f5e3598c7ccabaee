// cape_host_pose_score (cape_host_map.h): the host twin of cape_map_pose_score for ONE frame -- the pair list and the feature rows
// (pose_pairs.h) and every hypothesis' sums through the statements of csrc/cape_pose_score.h, which the device kernels compile too; the map plane goes
// through utils::plane_to_camera of the host class.  Serial: pair after pair, hypothesis after hypothesis.
#include <cstring>
#include <vector>

#include "boundary_polygon.hpp"
#include "pose_pairs.h"

extern "C" int cape_host_pose_score(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                                    int32_t n_hypotheses, const double* world_to_camera, cape_pose_score* scores_out,
                                    cape_pose_feature* features_out, double* residuals_out)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    if (n_hypotheses < 1 || !world_to_camera)
        return CAPE_ERR_INVALID_ARGUMENT;
    cape_host::PosePairs P;
    if (const int rc = cape_host::build_pose_pairs(map, match, detected, frame_flags, P); rc != CAPE_OK)
        return rc;
    const std::vector<cape_pose_feature>& features = P.features;
    const int nPairs = P.nPairs, nInvalid = P.nInvalid;
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
