// cape_map_step: the hand-off from a frame's commit to the maintenance behind it, without the host in between.  One plain function
// says which buffer set holds the map after (commit header, maintain header) and with which counts; the step's two kernels
// (cape_map_maintain.hip) take their source from it with the maintain header still all zero, the host (cape_api_map_update.hip) does
// its bookkeeping with it after the one wait, and tests/host/map_step_plan.cpp compiles it between the two serial plans.
//
// Like cape_map_commit.h and cape_map_maintain.h: __host__ __device__ with hipcc, plain inline functions with any other compiler.
#pragma once
#include "cape_map_commit.h"
#include "cape_map_maintain.h"

namespace cape {

// The three buffer sets of a step (planes, rings, vertices, tracks, tags each).  The commit reads FRONT and writes BACK; the
// maintenance reads BACK and writes THIRD: no kernel of the call writes a set that another one of the call still reads.
enum : uint32_t
{
    kStepSetFront = 0, // the map as the call finds it
    kStepSetBack = 1,  // the committed map
    kStepSetThird = 2  // the maintained map
};

struct StepMapState
{
    uint32_t set;          // kStepSet*: where the map and its tracks lie
    int32_t planes, rings; // what they hold
    int64_t vertices;
};

// The map after a commit that reported `c` and a maintenance behind it that reported `m` -- all zero where it has not run (yet):
// that is what the step's kernels pass, and the state they get is their source.  A commit that is not DONE leaves the map where it
// was (c's sizes are the old ones then); a maintenance that is not DONE (nothing due, a refusal, not run) leaves the committed map.
CAPE_MAINTAIN_FN StepMapState step_map_after(const cape_map_commit_result& c, const cape_map_maintain_result& m)
{
    if (!(c.flags & CAPE_COMMIT_DONE))
        return StepMapState {kStepSetFront, c.n_planes, c.n_rings, c.n_vertices};
    if (!(m.flags & CAPE_MAINTAIN_DONE))
        return StepMapState {kStepSetBack, c.n_planes, c.n_rings, c.n_vertices};
    return StepMapState {kStepSetThird, m.n_planes, m.n_rings, m.n_vertices};
}

#if defined(__HIPCC__)
// cape_map_step's two kernels (cape_map_maintain.hip): cape_map_maintain's, with the source's counts, the capacities that follow
// from them and the decision to run at all taken from the commit's header in device memory
struct MapStepParams
{
    // what the host knows: the source buffers (the commit's BACK set), the destination (the THIRD set), the log's arrays and what the
    // log holds, plan and header.  nMap, nMapRings, nMapVertices, the three capacities and the log's capacities are NOT read: the
    // kernels derive them from the commit's header as cape_map_maintain's host side derives them from the map's sizes
    MapMaintainParams maintain;
    const cape_map_commit_result* commit; // device memory: written by the commit's plan kernel earlier on the stream
};
#endif

} // namespace cape
