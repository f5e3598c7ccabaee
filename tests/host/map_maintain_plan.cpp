// The plan of cape_map_maintain (csrc/cape_map_maintain.h: maintain_plane, maintain_count, maintain_row, maintain_result and the serial
// scan maintain_plan_serial over them) compiled for the HOST, and the plan KERNEL's scans restated as it does them -- four planes per
// lane, an inclusive scan over the 64 lanes of a wave, the waves' totals through a table, the three sequences' starts -- compared with
// the serial plan row for row on random maps of 0, 1, 255, 256, 257 and 1024 planes, under the address and undefined-behaviour
// sanitizers.  A stand-alone program: tests/host/hip_stub stands in for the HIP runtime header.  Build and run from the repository
// root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc
//       -o map_maintain_plan.exe tests/host/map_maintain_plan.cpp && ./map_maintain_plan.exe
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cape_map_maintain.h"

namespace {

constexpr int kLanes = 256, kWave = 64, kWaves = kLanes / kWave, kPerLane = 4;
constexpr int kWords = 3 * (int)cape::kMaintainSequences + 4; // planes, rings, vertices of each sequence; promoted, refused, dropped, outside

struct Map
{
    std::vector<cape_map_plane> planes;
    std::vector<cape_map_ring> rings;
    int64_t nVertices = 0;
    std::vector<cape_map_track> tracks;
    std::vector<uint8_t> promotable;
    cape::MaintainLog log{};
};

// round: 0 .. 3 random classes; 4 nothing due; 5 a log that is nearly or quite full; 6, 7 a plane whose rings lie outside the map
Map make(std::mt19937_64& gen, int nMap, int round)
{
    auto pick = [&](int lo, int hi) { return (int)(lo + gen() % (uint64_t)(hi - lo + 1)); };
    Map m;
    m.planes.resize(nMap);
    m.tracks.resize(nMap);
    m.promotable.resize(nMap);
    for (int j = 0; j < nMap; ++j)
    {
        cape_map_plane& M = m.planes[j];
        std::memset(&M, 0, sizeof(M));
        M.ring_first = (uint32_t)m.rings.size();
        M.ring_count = pick(0, 9) ? 1u : (uint32_t)pick(1, 9);
        for (uint32_t k = 0; k < M.ring_count; ++k)
        {
            const uint32_t n = (uint32_t)pick(3, k ? 12 : 40);
            m.rings.push_back(cape_map_ring {(uint32_t)m.nVertices, n});
            m.nVertices += n;
        }
        cape_map_track& T = m.tracks[j];
        std::memset(&T, 0, sizeof(T));
        const bool staged = pick(0, 1) != 0;
        T.flags = (staged ? (uint32_t)CAPE_MAP_TRACK_STAGED : 0u) | (pick(0, 3) ? 0u : (uint32_t)CAPE_MAP_TRACK_MOVING);
        if (round == 4)
        {
            T.successive_matched = pick(-5, 3);
            T.failed_tracking = (uint32_t)pick(0, staged ? 1 : 9);
        }
        else
        {
            T.successive_matched = pick(0, 2) ? pick(-5, 3) : pick(4, 9);
            T.failed_tracking = pick(0, 2) ? (uint32_t)pick(0, 1) : (uint32_t)pick(2, 14);
        }
        T.id = 1000u + (uint64_t)j;
        m.promotable[j] = round == 4 ? 0 : (uint8_t)(pick(0, 3) != 0); // (round 4: a candidate there would be refused, which is not due either)
    }
    m.log.held = cape::MaintainCursor {pick(0, 50), pick(50, 90), pick(900, 1000)};
    m.log.planesCapacity = m.log.ringsCapacity = m.log.verticesCapacity = ~(uint64_t)0;
    if (round == 5)
        m.log.held.planes = CAPE_MAP_RETIRED_MAX_PLANES - pick(0, nMap / 16 + 1);
    if (round >= 6 && nMap > 0)
    {
        cape_map_plane& M = m.planes[pick(0, nMap - 1)];
        if (round % 2)
            M.ring_first = (uint32_t)m.rings.size();
        else
            M.ring_count = pick(0, 1) ? 10u : 0u;
    }
    return m;
}

// ---- the kernel's way: per lane, per wave, per workgroup
struct Kernel
{
    std::vector<cape::MaintainPlanRow> rows;
    cape_map_maintain_result result{};
};

Kernel kernel_way(const Map& m)
{
    const int nMap = (int)m.planes.size();
    Kernel out;
    out.rows.resize(nMap);
    std::vector<cape::MaintainItem> items((size_t)kLanes * kPerLane);
    std::vector<int> my((size_t)kLanes * kWords, 0), incl((size_t)kLanes * kWords, 0);
    // the lanes: four planes each, in order
    for (int tid = 0; tid < kLanes; ++tid)
    {
        cape::MaintainTotals mine{};
        for (int k = 0; k < kPerLane; ++k)
        {
            const int j = kPerLane * tid + k;
            if (j >= nMap)
                continue;
            const cape_map_track& T = m.tracks[j];
            const bool ok = cape::maintain_promote_candidate(T.flags, T.successive_matched) && m.promotable[j] != 0;
            items[(size_t)tid * kPerLane + k] = cape::maintain_plane(m.planes[j], m.rings.data(), m.rings.size(), (uint64_t)m.nVertices, T.flags,
                                                                     T.successive_matched, T.failed_tracking, ok);
            cape::maintain_count(mine, items[(size_t)tid * kPerLane + k]);
        }
        int* w = &my[(size_t)tid * kWords];
        for (int s = 0; s < (int)cape::kMaintainSequences; ++s)
        {
            w[3 * s] = mine.seq[s].planes;
            w[3 * s + 1] = mine.seq[s].rings;
            w[3 * s + 2] = (int)mine.seq[s].vertices;
        }
        w[9] = mine.promoted;
        w[10] = mine.promoteRefused;
        w[11] = mine.dropped;
        w[12] = mine.outside;
    }
    // the waves: an inclusive scan over the 64 lanes (a sum for the counts), lane 63 leaves the wave's totals in the table
    int sums[kWaves][kWords];
    for (int wave = 0; wave < kWaves; ++wave)
        for (int w = 0; w < kWords; ++w)
        {
            int run = 0;
            for (int lane = 0; lane < kWave; ++lane)
            {
                run += my[(size_t)(wave * kWave + lane) * kWords + w];
                incl[(size_t)(wave * kWave + lane) * kWords + w] = run;
            }
            sums[wave][w] = run;
        }
    // the workgroup: every lane adds the waves before its own; the totals make the header
    int total[kWords];
    for (int w = 0; w < kWords; ++w)
    {
        total[w] = 0;
        for (int v = 0; v < kWaves; ++v)
            total[w] += sums[v][w];
    }
    cape::MaintainTotals t{};
    for (int s = 0; s < (int)cape::kMaintainSequences; ++s)
        t.seq[s] = cape::MaintainCursor {total[3 * s], total[3 * s + 1], (int64_t)total[3 * s + 2]};
    t.promoted = total[9];
    t.promoteRefused = total[10];
    t.dropped = total[11];
    t.outside = total[12];
    out.result = cape::maintain_result(t, nMap, (int32_t)m.rings.size(), m.nVertices, (uint64_t)nMap, m.rings.size(), (uint64_t)m.nVertices, m.log);
    const cape::MaintainCursor start[cape::kMaintainSequences] = {cape::MaintainCursor {0, 0, 0}, t.seq[cape::kMaintainSeqLocal], m.log.held};
    for (int tid = 0; tid < kLanes; ++tid)
    {
        const int wave = tid / kWave;
        cape::MaintainCursor at[cape::kMaintainSequences];
        for (int s = 0; s < (int)cape::kMaintainSequences; ++s)
        {
            int before[3] = {0, 0, 0};
            for (int v = 0; v < wave; ++v)
                for (int c = 0; c < 3; ++c)
                    before[c] += sums[v][3 * s + c];
            const int* mine = &my[(size_t)tid * kWords + 3 * s];
            const int* in = &incl[(size_t)tid * kWords + 3 * s];
            at[s].planes = start[s].planes + before[0] + in[0] - mine[0];
            at[s].rings = start[s].rings + before[1] + in[1] - mine[1];
            at[s].vertices = start[s].vertices + (int64_t)(before[2] + in[2] - mine[2]);
        }
        for (int k = 0; k < kPerLane; ++k)
        {
            const int j = kPerLane * tid + k;
            if (j >= nMap)
                continue;
            const cape::MaintainItem& it = items[(size_t)tid * kPerLane + k];
            const uint32_t seq = cape::maintain_sequence(it.cls);
            if (seq == cape::kMaintainSeqNone)
            {
                out.rows[j] = cape::maintain_row(it, cape::MaintainCursor {0, 0, 0});
                continue;
            }
            out.rows[j] = cape::maintain_row(it, at[seq]);
            at[seq].planes += 1;
            at[seq].rings += (int32_t)it.rings;
            at[seq].vertices += (int64_t)it.vertices;
        }
    }
    return out;
}

} // namespace

int main()
{
    std::mt19937_64 gen(20240611);
    const int widths[6] = {0, 1, 255, 256, 257, 1024};
    long maps = 0, differ = 0, flags[4] = {0, 0, 0, 0}, classes[cape::kMaintainClasses] = {0, 0, 0, 0, 0, 0}, outsideFirst = 0, outsideCount = 0;
    for (int nMap : widths)
        for (int round = 0; round < 40; ++round)
        {
            const Map m = make(gen, nMap, round % 8);
            std::vector<cape::MaintainPlanRow> rows((size_t)nMap + 1);
            const cape_map_maintain_result got =
                cape::maintain_plan_serial(m.planes.data(), nMap, m.rings.data(), (int32_t)m.rings.size(), m.nVertices, m.tracks.data(), m.promotable.data(),
                                           (uint64_t)nMap, m.rings.size(), (uint64_t)m.nVertices, m.log, rows.data());
            const Kernel want = kernel_way(m);
            bool same = std::memcmp(&got, &want.result, sizeof(got)) == 0;
            for (int j = 0; j < nMap && same; ++j)
                same = std::memcmp(&rows[j], &want.rows[j], sizeof(cape::MaintainPlanRow)) == 0;
            // what a DONE plan promises the copy kernel: every destination inside its sequence, each exactly once
            if (same && (got.flags & CAPE_MAINTAIN_DONE))
            {
                std::vector<int> mapHit((size_t)got.n_planes, 0), logHit((size_t)got.n_retired, 0);
                for (int j = 0; j < nMap; ++j)
                {
                    const cape::MaintainPlanRow& r = rows[j];
                    if (r.dest == cape::kMaintainToMap && r.plane < (uint32_t)got.n_planes && (uint64_t)r.ringFirst + r.ringCount <= (uint64_t)got.n_rings &&
                        (int64_t)r.vertexFirst + r.vertexCount <= got.n_vertices)
                        ++mapHit[r.plane];
                    else if (r.dest == cape::kMaintainToLog && r.plane >= (uint32_t)m.log.held.planes && r.plane < (uint32_t)got.n_retired &&
                             (uint64_t)r.ringFirst + r.ringCount <= (uint64_t)got.n_retired_rings &&
                             (int64_t)r.vertexFirst + r.vertexCount <= got.n_retired_vertices)
                        ++logHit[r.plane];
                    else if (r.dest != cape::kMaintainToNone)
                        same = false;
                }
                for (int b = 0; b < got.n_planes; ++b)
                    same = same && mapHit[b] == 1;
                for (int b = m.log.held.planes; b < got.n_retired; ++b)
                    same = same && logHit[b] == 1;
            }
            ++maps;
            for (int bit = 0; bit < 4; ++bit)
                flags[bit] += (got.flags >> bit) & 1u;
            for (int j = 0; j < nMap; ++j)
                ++classes[rows[j].cls];
            if (round % 8 >= 6 && nMap > 0)
            {
                ++outsideCount;
                outsideFirst += round % 2;
                same = same && (got.flags & CAPE_MAINTAIN_CAPACITY) && got.n_planes == nMap;
            }
            if (round % 8 == 4)
                same = same && got.flags == CAPE_MAINTAIN_NOTHING;
            if (!same)
            {
                ++differ;
                std::printf("differs: %d planes, round %d: flags %#x / %#x, planes %d / %d, rings %d / %d, vertices %lld / %lld, log %d / %d\n", nMap, round,
                            got.flags, want.result.flags, got.n_planes, want.result.n_planes, got.n_rings, want.result.n_rings, (long long)got.n_vertices,
                            (long long)want.result.n_vertices, got.n_retired, want.result.n_retired);
            }
        }
    std::printf("maps: %ld; DONE %ld, NOTHING %ld, refused for CAPACITY %ld (a ring index outside %ld, a ring count outside %ld), LOG_FULL %ld\n", maps, flags[0],
                flags[1], flags[2], outsideFirst, outsideCount - outsideFirst, flags[3]);
    std::printf("classes: keep-local %ld, promoted %ld, keep-staged %ld, dropped %ld, lost %ld, promote-refused %ld\n", classes[0], classes[1], classes[2],
                classes[3], classes[4], classes[5]);
    std::printf("maps whose serial plan differs from the kernel's way: %ld\n", differ);
    // every class and every refusal cause occurs
    bool all = flags[0] > 0 && flags[1] > 0 && flags[2] > 0 && flags[3] > 0 && outsideFirst > 0 && outsideCount > outsideFirst;
    for (long c : classes)
        all = all && c > 0;
    if (!all)
        std::printf("a class or a refusal cause did not occur\n");
    return differ == 0 && all ? 0 : 1;
}
