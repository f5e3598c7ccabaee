// The pair list of cape_map_pose_score (csrc/cape_pose_score.h) compiled for the HOST: the serial statement of the list
// (pose_pairs_serial: the map planes in ascending order whose match names a kept plane) against the pairs kernel's way to the same
// list, restated lane by lane -- the map planes taken 64 at a time, lane l holding plane chunk + l, a ballot over the chunk, the
// pair's slot = the pairs of the chunks before + the ballot's bits below the lane (pose_pair_slot), one writer per slot, then lanes k
// and k + 64 zeroing the slots at and beyond n_pairs.  Asserted per map size in {0, 1, 63, 64, 65, 128, 1023, 1024} and pair count in
// {0, 1, 64, 65, 128} (where the map has as many planes): both lists are equal, every slot below n_pairs is written exactly once and
// none at or beyond it, every slot of the 128 is either written or zeroed and never both, nothing outside the frame's 128 rows is
// touched, n_pairs is the ballots' sum.  A match table that names more than 128 pairs (not one the wide match writes) stores the
// first 128 and drops the rest, in both statements.  Under the address and undefined-behaviour sanitizers.  A stand-alone program:
// tests/host/hip_stub stands in for the HIP runtime header.  Build and run from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc
//       -o pose_score_pairs.exe tests/host/pose_score_pairs.cpp && ./pose_score_pairs.exe
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "cape_pose_score.h"

namespace {

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

int popcount64(unsigned long long v)
{
    int c = 0;
    for (; v; v &= v - 1)
        ++c;
    return c;
}

constexpr int WP = cape::kPoseScoreMaxPairs;
constexpr int32_t kGuard = -77, kUnwritten = -1;

// nPairs of the nMap planes carry a match (more than 128 only where the caller asks for the overflow case)
bool one_frame(int nMap, int nPairs, std::mt19937& rng)
{
    using namespace cape;
    const int before = failures;
    std::vector<int32_t> match(nMap, -1);
    {
        std::vector<int> planes(nMap), keptPlanes(WP);
        std::iota(planes.begin(), planes.end(), 0);
        std::iota(keptPlanes.begin(), keptPlanes.end(), 0);
        std::shuffle(planes.begin(), planes.end(), rng);
        std::shuffle(keptPlanes.begin(), keptPlanes.end(), rng);
        for (int k = 0; k < nPairs; ++k)
            match[planes[k]] = keptPlanes[k % WP];
        // what is no pair: -1, any other negative number, a kept plane at or beyond 128
        for (int j = 0; j < nMap; ++j)
            if (match[j] < 0 && rng() % 4 == 0)
                match[j] = rng() % 2 ? -(int32_t)(rng() % 1000) - 1 : WP + (int32_t)(rng() % 1000);
    }
    // ---- the serial statement
    std::vector<int32_t> serial(WP + 2, kGuard);
    const int nSerial = pose_pairs_serial(match.data(), nMap, serial.data() + 1);
    CHECK(serial.front() == kGuard && serial.back() == kGuard, "n_map %d: the serial list wrote outside its 128 entries", nMap);
    CHECK(nSerial == std::min(nPairs, WP), "n_map %d: %d pairs listed, %d made", nMap, nSerial, nPairs);
    // ---- the kernel's way: rows[k] = the map plane whose lane wrote slot k, between guard rows
    std::vector<int32_t> rows(WP + 2, kUnwritten);
    rows.front() = rows.back() = kGuard;
    std::vector<int> writes(WP, 0), zeroed(WP, 0);
    int base = 0;
    for (int jb = 0; jb < nMap; jb += 64)
    {
        unsigned long long ballot = 0;
        for (int lane = 0; lane < 64; ++lane)
        {
            const int j = jb + lane;
            const int32_t i = j < nMap ? match[j] : -1; // (the lanes beyond the map read nothing)
            if (pose_is_pair(i))
                ballot |= 1ull << lane;
        }
        for (int lane = 0; lane < 64; ++lane)
        {
            if (!((ballot >> lane) & 1ull))
                continue;
            const int k = pose_pair_slot(ballot, lane, base);
            CHECK(k >= base && k < base + popcount64(ballot), "n_map %d: lane %d of chunk %d got slot %d", nMap, lane, jb, k);
            if (k < WP)
            {
                ++writes[k];
                rows[1 + k] = jb + lane;
            }
        }
        base += popcount64(ballot);
    }
    const int nKernel = std::min(base, WP);
    for (int s = 0; s < 2; ++s)
        for (int lane = 0; lane < 64; ++lane)
        {
            const int k = lane + 64 * s;
            if (k >= nKernel)
            {
                ++zeroed[k];
                rows[1 + k] = kUnwritten;
            }
        }
    CHECK(rows.front() == kGuard && rows.back() == kGuard, "n_map %d: a row outside the frame's 128 was touched", nMap);
    CHECK(base == nPairs && nKernel == nSerial, "n_map %d: the ballots count %d pairs, the serial list %d of %d", nMap, base, nSerial, nPairs);
    for (int k = 0; k < WP; ++k)
    {
        CHECK(writes[k] == (k < nKernel ? 1 : 0), "n_map %d: slot %d written %d times", nMap, k, writes[k]);
        CHECK(zeroed[k] == (k < nKernel ? 0 : 1), "n_map %d: slot %d zeroed %d times", nMap, k, zeroed[k]);
        CHECK(rows[1 + k] == (k < nSerial ? serial[1 + k] : kUnwritten), "n_map %d: slot %d holds map plane %d, the serial list %d", nMap, k,
              rows[1 + k], k < nSerial ? serial[1 + k] : kUnwritten);
        if (k > 0 && k < nKernel)
            CHECK(rows[1 + k] > rows[k], "n_map %d: slot %d is not in map order", nMap, k);
        if (k < nKernel)
            CHECK(pose_is_pair(match[rows[1 + k]]), "n_map %d: slot %d names a plane without a pair", nMap, k);
    }
    std::printf("n_map %4d: %3d pairs made, %3d listed\n", nMap, nPairs, nKernel);
    return failures == before;
}

} // namespace

int main()
{
    std::mt19937 rng(31);
    const int sizes[] = {0, 1, 63, 64, 65, 128, 1023, 1024}, counts[] = {0, 1, 64, 65, 128};
    int frames = 0, wrong = 0, full = 0;
    for (const int n : sizes)
        for (const int c : counts)
            if (c <= n)
                for (int rep = 0; rep < 4; ++rep, ++frames)
                {
                    wrong += one_frame(n, c, rng) ? 0 : 1;
                    full += c == 128;
                }
    // beyond what the wide match writes: more pairs than rows
    int overflow = 0;
    for (const int c : {129, 200, 1024})
        for (int rep = 0; rep < 2; ++rep, ++overflow)
            wrong += one_frame(1024, c, rng) ? 0 : 1;
    // the lane masks at their ends
    CHECK(cape::pose_pair_slot(~0ull, 0, 5) == 5 && cape::pose_pair_slot(~0ull, 63, 5) == 68 && cape::pose_pair_slot(1ull << 63, 63, 0) == 0,
          "pose_pair_slot at lanes 0 and 63");
    std::printf("frames: %d; with 128 pairs: %d; with more than 128: %d\n", frames, full, overflow);
    std::printf("frames whose kernel list differs from the serial one or breaks a rule: %d\n", wrong);
    return wrong == 0 && failures == 0 ? 0 : 1;
}
