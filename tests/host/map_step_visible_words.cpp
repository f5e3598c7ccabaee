// The ownership and word rules of cape_map_step_visible's one-frame classify kernel (csrc/cape_map_step_visible.h) compiled for the
// HOST and driven serially, the way the kernel drives them: for every group of the launch, every wave of the group and every round
// of the wave the plane step_vis_plane names is decided once (moving, listed or ruled out, drawn per plane), the group's bits are
// joined, step_vis_store_words writes the group's words from step_vis_present, the listed planes go to the work list and the visible
// ones among them have their bit cleared, as the visible kernels clear it.  Compared with a naive loop over the bits: bit j set
// <=> j < n_map and (moving[j] or not (candidate[j] and visible[j])).  Asserted per n_map in {0, 1, 31, 32, 33, 63, 64, 65, 255, 256,
// 257, 1023, 1024}: every plane below n_map is visited exactly once and none at or beyond it is decided, every one of the
// ceil(n_map / 32) words is written exactly once and no other, the bits beyond n_map in the last word are 0, the inverse functions
// name the owner that visited the plane, and the work list holds each listed plane once and nothing else.  Under the address and
// undefined-behaviour sanitizers.  A stand-alone program.  Build and run from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Irgb-d-slam_amd/csrc
//       -o map_step_visible_words.exe tests/host/map_step_visible_words.cpp && ./map_step_visible_words.exe
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cape_map_step_visible.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                      \
    do                                        \
    {                                         \
        if (!(cond))                          \
        {                                     \
            ++failures;                       \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                \
        }                                     \
    } while (0)

int popcount64(unsigned long long v)
{
    int c = 0;
    for (; v; v &= v - 1)
        ++c;
    return c;
}

bool one_map(int nMap, std::mt19937& rng)
{
    using namespace cape;
    const int before = failures;
    const int skipWords = (nMap + 31) / 32;
    std::vector<uint8_t> moving(nMap), candidate(nMap), visible(nMap);
    for (int j = 0; j < nMap; ++j)
    {
        moving[j] = rng() % 4 == 0;
        candidate[j] = rng() % 3 != 0;
        visible[j] = rng() % 2 == 0;
    }
    // exactly the words the call owns, between guard words that nobody may touch
    std::vector<uint32_t> buffer(skipWords + 2, 0xDEADBEEFu);
    uint32_t* words = buffer.data() + 1;
    std::vector<int> wordWrites(skipWords, 0), visits(nMap, 0);
    std::vector<unsigned long long> work;
    int nMoving = 0, nListed = 0;
    const int groups = step_vis_groups(nMap);
    CHECK(groups == (nMap + 63) / 64, "n_map %d: %d groups", nMap, groups);
    for (int g = 0; g < groups; ++g)
    {
        unsigned long long listedBits = 0, movingBits = 0;
        for (int w = 0; w < kStepVisGroupWaves; ++w)
            for (int r = 0; r < kStepVisRounds; ++r)
            {
                const int j = step_vis_plane(g, w, r);
                if (j >= nMap)
                    break; // (the kernel's wave leaves its rounds here: every later round's plane lies beyond too)
                ++visits[j];
                CHECK(step_vis_group_of(j) == g && step_vis_wave_of(j) == w && step_vis_round_of(j) == r, "plane %d: the inverse names another owner", j);
                CHECK(g * kStepVisGroupPlanes + step_vis_slot(w, r) == j, "plane %d: its slot is bit %d of group %d", j, step_vis_slot(w, r), g);
                const unsigned long long bit = 1ull << step_vis_slot(w, r);
                CHECK(!((listedBits | movingBits) & bit), "plane %d: its bit is taken", j);
                if (moving[j])
                    movingBits |= bit;
                else if (candidate[j])
                    listedBits |= bit;
            }
        // a wave that broke off must not have left a plane below n_map to a later round
        for (int w = 0; w < kStepVisGroupWaves; ++w)
            for (int r = 0; r < kStepVisRounds; ++r)
                if (step_vis_plane(g, w, r) < nMap)
                    CHECK(visits[step_vis_plane(g, w, r)] == 1, "plane %d was left out", step_vis_plane(g, w, r));
        const int wrote = step_vis_store_words(words, skipWords, g, step_vis_present(g, nMap));
        for (int k = 0; k < wrote; ++k)
        {
            CHECK(2 * g + k < skipWords, "group %d writes word %d of %d", g, 2 * g + k, skipWords);
            if (2 * g + k < skipWords)
                ++wordWrites[2 * g + k];
        }
        nMoving += popcount64(movingBits);
        nListed += popcount64(listedBits);
        for (int lane = 0; lane < 64; ++lane)
            if ((listedBits >> lane) & 1ull)
                work.push_back((unsigned long long)(unsigned)(g * kStepVisGroupPlanes + lane));
    }
    CHECK(buffer.front() == 0xDEADBEEFu && buffer.back() == 0xDEADBEEFu, "n_map %d: a word outside the call's was written", nMap);
    for (int j = 0; j < nMap; ++j)
        CHECK(visits[j] == 1, "n_map %d: plane %d decided %d times", nMap, j, visits[j]);
    for (int w = 0; w < skipWords; ++w)
        CHECK(wordWrites[w] == 1, "n_map %d: word %d written %d times", nMap, w, wordWrites[w]);
    // the initial words: every bit below n_map set, the bits beyond clear
    for (int b = 0; b < skipWords * 32; ++b)
        CHECK((((words[b >> 5] >> (b & 31)) & 1u) != 0) == (b < nMap), "n_map %d: initial bit %d", nMap, b);
    // the work list: each listed plane once, nothing else, within the list's n_map entries
    CHECK((int)work.size() == nListed && nListed <= nMap, "n_map %d: %zu entries for %d listed planes", nMap, work.size(), nListed);
    std::vector<int> listedTimes(nMap, 0);
    for (const unsigned long long e : work)
    {
        CHECK((e >> 32) == 0 && (int)(e & 0xFFFFFFFFu) < nMap, "n_map %d: entry %llx", nMap, e);
        if ((int)(e & 0xFFFFFFFFu) < nMap)
            ++listedTimes[(int)(e & 0xFFFFFFFFu)];
    }
    int wantMoving = 0;
    for (int j = 0; j < nMap; ++j)
    {
        CHECK(listedTimes[j] == ((!moving[j] && candidate[j]) ? 1 : 0), "n_map %d: plane %d listed %d times", nMap, j, listedTimes[j]);
        wantMoving += moving[j];
    }
    CHECK(nMoving == wantMoving, "n_map %d: %d moving planes counted, %d drawn", nMap, nMoving, wantMoving);
    // the visible kernels: a listed plane that is visible has its bit cleared
    for (const unsigned long long e : work)
    {
        const int j = (int)(e & 0xFFFFFFFFu);
        if (j < nMap && visible[j])
            words[j >> 5] &= ~(1u << (j & 31));
    }
    // ... against the naive loop
    for (int b = 0; b < skipWords * 32; ++b)
    {
        const bool want = b < nMap && (moving[b] || !(candidate[b] && visible[b]));
        CHECK((((words[b >> 5] >> (b & 31)) & 1u) != 0) == want, "n_map %d: bit %d", nMap, b);
    }
    if (skipWords > 0 && nMap % 32)
        CHECK((words[skipWords - 1] >> (nMap % 32)) == 0u, "n_map %d: bits beyond n_map in the last word", nMap);
    std::printf("n_map %4d: %2d groups, %2d words, %4d moving, %4d listed\n", nMap, groups, skipWords, nMoving, nListed);
    return failures == before;
}

} // namespace

int main()
{
    std::mt19937 rng(20);
    const int sizes[] = {0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024};
    int maps = 0, wrong = 0;
    for (const int n : sizes)
        for (int rep = 0; rep < 4; ++rep, ++maps)
            wrong += one_map(n, rng) ? 0 : 1;
    std::printf("maps: %d; sizes: %zu\n", maps, sizeof(sizes) / sizeof(sizes[0]));
    std::printf("maps whose words differ from the naive loop or break a rule: %d\n", wrong);
    return wrong == 0 && failures == 0 ? 0 : 1;
}
