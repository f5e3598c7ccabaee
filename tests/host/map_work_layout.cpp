// The work layouts of the map's entry points (csrc/cape_api_map.h: map_work_layout for the map matchers and, without mask words, for
// cape_match_polygons_wide; visibility_work_layout for the visibility kernels) compiled for the HOST against a table of offsets
// recorded from the three layout functions these two replace -- the map matchers', the wide polygon matcher's own and the visibility
// kernels' -- at batch sizes 1, 2 and 4 096, capacities 1, 255, 256, 257 and kMapWorkMax and 0, 1 and 2 mask words.  Buffer offsets
// are behaviour: cape_debug_map_match_lists reads the counters at a fixed place, and a section that moved or shrank is a kernel
// writing into its neighbour.  Asserted per row: every section on a 256-byte boundary, the sections in the documented order, none
// overlapping the next (a section is at least what its entries take; the mask section is empty without mask words), and every
// offset the recorded one.  Under the address and undefined-behaviour sanitizers.  A stand-alone program: tests/host/hip_stub
// stands in for the HIP runtime header.  Build and run from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc
//       -o map_work_layout.exe tests/host/map_work_layout.cpp && ./map_work_layout.exe
#include <cstddef>
#include <cstdio>

#define CAPE_API_MAP_LAYOUTS_ONLY
#include "cape_api_map.h"

namespace {

using namespace cape::abi;

int failures = 0;
#define CHECK(cond, ...)                         \
    do                                           \
    {                                            \
        if (!(cond))                             \
        {                                        \
            ++failures;                          \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                   \
        }                                        \
    } while (0)

// recorded: {max_batch, capacity, mask words, {counts, ranges, masks, work, area, tiers, total}}
struct MapRow
{
    int batch;
    size_t cap;
    int maskWords;
    size_t at[7];
};
const MapRow kMapRows[] = {
    {1, 1u, 0, {0u, 256u, 512u, 512u, 768u, 1024u, 1280u}},
    {1, 1u, 1, {0u, 256u, 512u, 8704u, 8960u, 9216u, 9472u}},
    {1, 1u, 2, {0u, 256u, 512u, 16896u, 17152u, 17408u, 17664u}},
    {1, 255u, 0, {0u, 256u, 512u, 512u, 2560u, 4608u, 7680u}},
    {1, 255u, 1, {0u, 256u, 512u, 8704u, 10752u, 12800u, 15872u}},
    {1, 255u, 2, {0u, 256u, 512u, 16896u, 18944u, 20992u, 24064u}},
    {1, 256u, 0, {0u, 256u, 512u, 512u, 2560u, 4608u, 7680u}},
    {1, 256u, 1, {0u, 256u, 512u, 8704u, 10752u, 12800u, 15872u}},
    {1, 256u, 2, {0u, 256u, 512u, 16896u, 18944u, 20992u, 24064u}},
    {1, 257u, 0, {0u, 256u, 512u, 512u, 2816u, 5120u, 8448u}},
    {1, 257u, 1, {0u, 256u, 512u, 8704u, 11008u, 13312u, 16640u}},
    {1, 257u, 2, {0u, 256u, 512u, 16896u, 19200u, 21504u, 24832u}},
    {1, 16777216u, 0, {0u, 256u, 512u, 512u, 134218240u, 268435968u, 469762560u}},
    {1, 16777216u, 1, {0u, 256u, 512u, 8704u, 134226432u, 268444160u, 469770752u}},
    {1, 16777216u, 2, {0u, 256u, 512u, 16896u, 134234624u, 268452352u, 469778944u}},
    {2, 1u, 0, {0u, 256u, 512u, 512u, 768u, 1024u, 1280u}},
    {2, 1u, 1, {0u, 256u, 512u, 16896u, 17152u, 17408u, 17664u}},
    {2, 1u, 2, {0u, 256u, 512u, 33280u, 33536u, 33792u, 34048u}},
    {2, 255u, 0, {0u, 256u, 512u, 512u, 2560u, 4608u, 7680u}},
    {2, 255u, 1, {0u, 256u, 512u, 16896u, 18944u, 20992u, 24064u}},
    {2, 255u, 2, {0u, 256u, 512u, 33280u, 35328u, 37376u, 40448u}},
    {2, 256u, 0, {0u, 256u, 512u, 512u, 2560u, 4608u, 7680u}},
    {2, 256u, 1, {0u, 256u, 512u, 16896u, 18944u, 20992u, 24064u}},
    {2, 256u, 2, {0u, 256u, 512u, 33280u, 35328u, 37376u, 40448u}},
    {2, 257u, 0, {0u, 256u, 512u, 512u, 2816u, 5120u, 8448u}},
    {2, 257u, 1, {0u, 256u, 512u, 16896u, 19200u, 21504u, 24832u}},
    {2, 257u, 2, {0u, 256u, 512u, 33280u, 35584u, 37888u, 41216u}},
    {2, 16777216u, 0, {0u, 256u, 512u, 512u, 134218240u, 268435968u, 469762560u}},
    {2, 16777216u, 1, {0u, 256u, 512u, 16896u, 134234624u, 268452352u, 469778944u}},
    {2, 16777216u, 2, {0u, 256u, 512u, 33280u, 134251008u, 268468736u, 469795328u}},
    {4096, 1u, 0, {0u, 256u, 33024u, 33024u, 33280u, 33536u, 33792u}},
    {4096, 1u, 1, {0u, 256u, 33024u, 33587456u, 33587712u, 33587968u, 33588224u}},
    {4096, 1u, 2, {0u, 256u, 33024u, 67141888u, 67142144u, 67142400u, 67142656u}},
    {4096, 255u, 0, {0u, 256u, 33024u, 33024u, 35072u, 37120u, 40192u}},
    {4096, 255u, 1, {0u, 256u, 33024u, 33587456u, 33589504u, 33591552u, 33594624u}},
    {4096, 255u, 2, {0u, 256u, 33024u, 67141888u, 67143936u, 67145984u, 67149056u}},
    {4096, 256u, 0, {0u, 256u, 33024u, 33024u, 35072u, 37120u, 40192u}},
    {4096, 256u, 1, {0u, 256u, 33024u, 33587456u, 33589504u, 33591552u, 33594624u}},
    {4096, 256u, 2, {0u, 256u, 33024u, 67141888u, 67143936u, 67145984u, 67149056u}},
    {4096, 257u, 0, {0u, 256u, 33024u, 33024u, 35328u, 37632u, 40960u}},
    {4096, 257u, 1, {0u, 256u, 33024u, 33587456u, 33589760u, 33592064u, 33595392u}},
    {4096, 257u, 2, {0u, 256u, 33024u, 67141888u, 67144192u, 67146496u, 67149824u}},
    {4096, 16777216u, 0, {0u, 256u, 33024u, 33024u, 134250752u, 268468480u, 469795072u}},
    {4096, 16777216u, 1, {0u, 256u, 33024u, 33587456u, 167805184u, 302022912u, 503349504u}},
    {4096, 16777216u, 2, {0u, 256u, 33024u, 67141888u, 201359616u, 335577344u, 536903936u}},
};
// recorded from the wide polygon matcher's own layout: {max_batch, capacity, {counts, ranges, work, area, tiers, total}}
struct WideRow
{
    int batch;
    size_t cap;
    size_t at[6];
};
const WideRow kWideRows[] = {
    {1, 1u, {0u, 256u, 512u, 768u, 1024u, 1280u}},
    {1, 255u, {0u, 256u, 512u, 2560u, 4608u, 7680u}},
    {1, 256u, {0u, 256u, 512u, 2560u, 4608u, 7680u}},
    {1, 257u, {0u, 256u, 512u, 2816u, 5120u, 8448u}},
    {1, 16777216u, {0u, 256u, 512u, 134218240u, 268435968u, 469762560u}},
    {2, 1u, {0u, 256u, 512u, 768u, 1024u, 1280u}},
    {2, 255u, {0u, 256u, 512u, 2560u, 4608u, 7680u}},
    {2, 256u, {0u, 256u, 512u, 2560u, 4608u, 7680u}},
    {2, 257u, {0u, 256u, 512u, 2816u, 5120u, 8448u}},
    {2, 16777216u, {0u, 256u, 512u, 134218240u, 268435968u, 469762560u}},
    {4096, 1u, {0u, 256u, 33024u, 33280u, 33536u, 33792u}},
    {4096, 255u, {0u, 256u, 33024u, 35072u, 37120u, 40192u}},
    {4096, 256u, {0u, 256u, 33024u, 35072u, 37120u, 40192u}},
    {4096, 257u, {0u, 256u, 33024u, 35328u, 37632u, 40960u}},
    {4096, 16777216u, {0u, 256u, 33024u, 134250752u, 268468480u, 469795072u}},
};
// recorded: {capacity, {counts, work, tiers, total}}
struct VisibilityRow
{
    size_t cap;
    size_t at[4];
};
const VisibilityRow kVisibilityRows[] = {
    {1u, {0u, 256u, 512u, 768u}},
    {255u, {0u, 256u, 2304u, 5376u}},
    {256u, {0u, 256u, 2304u, 5376u}},
    {257u, {0u, 256u, 2560u, 5888u}},
    {16777216u, {0u, 256u, 134217984u, 335544576u}},
};

// sections at[0 .. count): aligned, in order, each at least `bytes[k]` long, the last ending at at[count]
void check_sections(const char* what, const size_t* at, const size_t* bytes, int count)
{
    CHECK(at[0] == 0, "%s: the counters do not start the buffer", what);
    for (int k = 0; k <= count; ++k)
        CHECK(at[k] % 256 == 0, "%s: offset %d = %zu is not 256-byte aligned", what, k, at[k]);
    for (int k = 0; k < count; ++k)
        CHECK(at[k] + bytes[k] <= at[k + 1] && at[k + 1] - at[k] < bytes[k] + 256, "%s: section %d at %zu takes %zu bytes, the next starts at %zu", what, k,
              at[k], bytes[k], at[k + 1]);
}

} // namespace

int main()
{
    static_assert(kMapWorkMax == (size_t)1 << 24, "the recorded rows end at kMapWorkMax");
    static_assert(map_work_layout(4096, 257, 0).work == map_work_layout(4096, 257, 0).masks, "no mask words: no mask section");
    char what[96];
    int rows = 0;
    for (const MapRow& r : kMapRows)
    {
        const MapWorkLayout l = map_work_layout(r.batch, r.cap, r.maskWords);
        const size_t at[7] = {l.counts, l.ranges, l.masks, l.work, l.area, l.tiers, l.total};
        const size_t bytes[6] = {16 * sizeof(unsigned), (size_t)r.batch * 8, (size_t)r.batch * CAPE_MAP_MAX_PLANES * r.maskWords * 8, r.cap * 8, r.cap * 8,
                                 3 * r.cap * 4};
        std::snprintf(what, sizeof(what), "map_work_layout(%d, %zu, %d)", r.batch, r.cap, r.maskWords);
        check_sections(what, at, bytes, 6);
        for (int k = 0; k < 7; ++k)
            CHECK(at[k] == r.at[k], "%s: offset %d is %zu, recorded %zu", what, k, at[k], r.at[k]);
        ++rows;
    }
    for (const WideRow& r : kWideRows)
    {
        // what cape_match_polygons_wide binds: the layout without mask words, its mask section empty
        const MapWorkLayout l = map_work_layout(r.batch, r.cap, 0);
        const size_t at[6] = {l.counts, l.ranges, l.work, l.area, l.tiers, l.total};
        std::snprintf(what, sizeof(what), "map_work_layout(%d, %zu, 0) for the wide polygon matcher", r.batch, r.cap);
        CHECK(l.masks == l.work, "%s: a mask section of %zu bytes", what, l.work - l.masks);
        for (int k = 0; k < 6; ++k)
            CHECK(at[k] == r.at[k], "%s: offset %d is %zu, recorded %zu", what, k, at[k], r.at[k]);
        ++rows;
    }
    for (const VisibilityRow& r : kVisibilityRows)
    {
        const VisibilityWorkLayout l = visibility_work_layout(r.cap);
        const size_t at[4] = {l.counts, l.work, l.tiers, l.total};
        const size_t bytes[3] = {16 * sizeof(unsigned), r.cap * 8, 3 * r.cap * 4};
        std::snprintf(what, sizeof(what), "visibility_work_layout(%zu)", r.cap);
        check_sections(what, at, bytes, 3);
        for (int k = 0; k < 4; ++k)
            CHECK(at[k] == r.at[k], "%s: offset %d is %zu, recorded %zu", what, k, at[k], r.at[k]);
        ++rows;
    }
    std::printf("rows: %d (map %zu, wide %zu, visibility %zu)\n", rows, sizeof(kMapRows) / sizeof(kMapRows[0]), sizeof(kWideRows) / sizeof(kWideRows[0]),
                sizeof(kVisibilityRows) / sizeof(kVisibilityRows[0]));
    std::printf("offsets that differ from the recorded ones or break a rule: %d\n", failures);
    return failures ? 1 : 0;
}
