// cape_host_pose_solve / cape_host_pose_select (cape_host_map.h): the host twins of cape_map_pose_solve and cape_map_pose_select for ONE
// frame -- the pair list and the feature rows as cape_host_pose_score builds them, then every problem through pose_solve_problem of
// csrc/cape_pose_solve.h, which the device kernel compiles too; the map plane goes through utils::plane_to_camera of the host class.
// Serial: problem after problem.
#include <cstring>
#include <vector>

#include "boundary_polygon.hpp"
#include "cape_hip.h"
#include "cape_host_map.h"
#include "../csrc/cape_pose_solve.h" // the rules, shared with the kernels

namespace {

struct HostPlaneToCamera
{
    void operator()(const double* T, const double* normal, double d, double qn[3], double& qd) const
    {
        // (the host function reads the twelve entries of the first three rows)
        rgbd_slam::utils::plane_to_camera(normal, d, T, qn, &qd);
    }
};

} // namespace

extern "C" int cape_host_pose_solve(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                                    int32_t n_problems, const double* x0, const uint32_t* subsets, const cape_pose_selection* selection,
                                    const cape_pose_solve_params* params, cape_pose_solution* solutions_out, double* world_to_camera_out,
                                    int32_t* n_rank_deficient_out)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    cape::PoseSolveSettings settings;
    if (!map || !detected || map->n_planes < 0 || detected->n < 0 || detected->n > WP || n_problems < 1 ||
        (frame_flags & ~(uint32_t)CAPE_MATCH_EXACT_OVERFLOW) || !cape::pose_solve_settings(params, settings))
        return CAPE_ERR_INVALID_ARGUMENT;
    if (selection ? n_problems != 1 : (!x0 || !subsets))
        return CAPE_ERR_INVALID_ARGUMENT;
    std::vector<cape_pose_score> scoreRow(1);
    std::vector<cape_pose_feature> features((size_t)WP);
    static const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    // the pairs, the feature rows, n_pairs and n_invalid: those of the score twin
    const int rc = cape_host_pose_score(map, match, detected, frame_flags, 1, kIdentity, scoreRow.data(), features.data(), nullptr);
    if (rc != CAPE_OK)
        return rc;
    std::vector<double> planes((size_t)WP * 8);
    std::vector<int> kept((size_t)WP);
    const int nPairs = scoreRow[0].n_pairs;
    for (int k = 0; k < nPairs; ++k)
    {
        for (int c = 0; c < 4; ++c)
            planes[8 * (size_t)k + c] = features[k].matched[c], planes[8 * (size_t)k + 4 + c] = features[k].map_plane[c];
        kept[k] = features[k].kept_plane;
    }
    int32_t nRankDeficient = 0;
    for (int32_t i = 0; i < n_problems; ++i)
    {
        const double* start = selection ? selection->x : x0 + 6 * (size_t)i;
        const uint32_t* words = selection ? selection->inlier_words : subsets + 4 * (size_t)i;
        const bool selected = !selection || selection->best >= 0;
        cape::PoseSolveRows rows;
        rows.planes = planes.data(), rows.kept = kept.data(), rows.nPairs = selected ? nPairs : 0;
        rows.subsetLo = (unsigned long long)words[0] | ((unsigned long long)words[1] << 32);
        rows.subsetHi = (unsigned long long)words[2] | ((unsigned long long)words[3] << 32);
        double T[12];
        cape_pose_solution r = cape::pose_solve_problem(rows, scoreRow[0].n_invalid, frame_flags & CAPE_MATCH_EXACT_OVERFLOW, start, settings,
                                                        HostPlaneToCamera{}, T);
        if (!selected)
            r.status = CAPE_POSE_SOLVE_NO_SELECTION;
        nRankDeficient += (r.flags & CAPE_POSE_SOLVE_RANK_DEFICIENT) ? 1 : 0;
        if (solutions_out)
            solutions_out[i] = r;
        if (world_to_camera_out)
            cape::pose_matrix16(T, world_to_camera_out + 16 * (size_t)i);
    }
    if (n_rank_deficient_out)
        *n_rank_deficient_out = nRankDeficient;
    return CAPE_OK;
}

extern "C" int cape_host_pose_select(int32_t n_hypotheses, const cape_pose_score* scores, const cape_pose_solution* solutions,
                                     cape_pose_selection* selection_out)
{
    if (n_hypotheses < 1 || !scores || !solutions || !selection_out)
        return CAPE_ERR_INVALID_ARGUMENT;
    *selection_out = cape::pose_select_frame(scores, solutions, n_hypotheses);
    return CAPE_OK;
}
