// cape_host_pose_solve / cape_host_pose_select (cape_host_map.h): the host twins of cape_map_pose_solve and cape_map_pose_select for ONE
// frame -- the pair list and the rows of pose_pairs.h, which cape_host_pose_score builds too, then every problem through pose_solve_problem of
// csrc/cape_pose_solve.h, which the device kernel compiles too; the map plane goes through utils::plane_to_camera of the host class.
// Serial: problem after problem.
#include <cstring>
#include <vector>

#include "boundary_polygon.hpp"
#include "pose_pairs.h"

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
    cape::PoseSolveSettings settings;
    if (n_problems < 1 || !cape::pose_solve_settings(params, settings))
        return CAPE_ERR_INVALID_ARGUMENT;
    if (selection ? n_problems != 1 : (!x0 || !subsets))
        return CAPE_ERR_INVALID_ARGUMENT;
    cape_host::PosePairs P;
    if (const int rc = cape_host::build_pose_pairs(map, match, detected, frame_flags, P); rc != CAPE_OK)
        return rc;
    int32_t nRankDeficient = 0;
    for (int32_t i = 0; i < n_problems; ++i)
    {
        const double* start = selection ? selection->x : x0 + 6 * (size_t)i;
        const uint32_t* words = selection ? selection->inlier_words : subsets + 4 * (size_t)i;
        const bool selected = !selection || selection->best >= 0;
        cape::PoseSolveRows rows;
        rows.planes = P.planes.data(), rows.kept = P.kept.data(), rows.nPairs = selected ? P.nPairs : 0;
        cape::pose_subset(words, rows.subsetLo, rows.subsetHi);
        double T[12];
        cape_pose_solution r = cape::pose_solve_problem(rows, P.nInvalid, frame_flags & CAPE_MATCH_EXACT_OVERFLOW, start, settings,
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
