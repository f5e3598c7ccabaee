// cape_map_step_visible: who owns which map plane and who writes which skip word in the one-frame classify kernel
// (cape_map_classify_one_kernel, cape_map_visibility.hip).  The kernel and tests/host/map_step_visible_words.cpp both compile these
// functions; nothing else decides an index there beyond "lane l takes the ring's vertices l, l + 64, ..".
//
//   * A workgroup owns kStepVisGroupPlanes = 64 consecutive map planes, i.e. the two skip words 2g and 2g + 1 of group g, and nobody
//     else writes them.  ceil(n_map / 64) groups cover every word exactly once; the last group has no second word where
//     ceil(n_map / 32) is odd.
//   * Inside a group, plane slot k (plane j = 64 g + k) belongs to wave k % kStepVisGroupWaves, which takes its slots in rounds
//     k / kStepVisGroupWaves = 0, 1, ..; the lanes of that wave split the ring's vertices.
//   * A word starts with every bit of a plane below n_map set and every bit beyond n_map clear: step_vis_present(g, n_map) is the
//     group's 64 such bits, and a word is its low or its high half.  The visible kernels later only clear bits.
//
// Like cape_map_step.h: __host__ __device__ with hipcc, plain inline functions with any other compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAPE_STEP_VIS_FN __host__ __device__ __forceinline__
#else
#define CAPE_STEP_VIS_FN inline
#endif

namespace cape {

constexpr int kStepVisGroupPlanes = 64; // map planes of a workgroup: two skip words
constexpr int kStepVisGroupWaves = 8;   // waves of a workgroup: 8 plane slots each
constexpr int kStepVisRounds = kStepVisGroupPlanes / kStepVisGroupWaves;

// workgroups of the launch (0 for an empty map: nothing is launched)
CAPE_STEP_VIS_FN int step_vis_groups(int nMap) { return (nMap + kStepVisGroupPlanes - 1) / kStepVisGroupPlanes; }
// the plane that wave `wave` of group `group` takes in round `round` (it may lie at or beyond n_map: the wave has none then)
CAPE_STEP_VIS_FN int step_vis_plane(int group, int wave, int round) { return group * kStepVisGroupPlanes + round * kStepVisGroupWaves + wave; }
// ... and the bit of the group's 64 that stands for it
CAPE_STEP_VIS_FN int step_vis_slot(int wave, int round) { return round * kStepVisGroupWaves + wave; }
// the inverse, for the stand-alone program: which group, wave and round own plane j
CAPE_STEP_VIS_FN int step_vis_group_of(int j) { return j / kStepVisGroupPlanes; }
CAPE_STEP_VIS_FN int step_vis_wave_of(int j) { return (j % kStepVisGroupPlanes) % kStepVisGroupWaves; }
CAPE_STEP_VIS_FN int step_vis_round_of(int j) { return (j % kStepVisGroupPlanes) / kStepVisGroupWaves; }
// bit k set = plane 64 g + k exists
CAPE_STEP_VIS_FN unsigned long long step_vis_present(int group, int nMap)
{
    const int left = nMap - group * kStepVisGroupPlanes;
    return left >= kStepVisGroupPlanes ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}
// The words group g writes, given the 64 bits it has decided to start set: word 2g always, word 2g + 1 where the map has one.
// Returns how many it wrote.
CAPE_STEP_VIS_FN int step_vis_store_words(uint32_t* words, int skipWords, int group, unsigned long long bits)
{
    const int w = 2 * group;
    words[w] = (uint32_t)bits;
    if (w + 1 >= skipWords)
        return 1;
    words[w + 1] = (uint32_t)(bits >> 32);
    return 2;
}

} // namespace cape
