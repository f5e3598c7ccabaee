// The plan of cape_map_commit (csrc/cape_map_commit.h: commit_map_plane, commit_union_rings, commit_appends, commit_result and the
// serial scan commit_plan_serial over them) compiled for the HOST and compared with a naive loop -- every decision restated from the
// header's prose, every offset summed from plane 0 again -- on random maps of 0, 1, 255, 256, 257 and 1024 planes, under the address
// and undefined-behaviour sanitizers.  A stand-alone program: tests/host/hip_stub stands in for the HIP runtime header.  Build and run
// from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc
//       -o map_commit_plan.exe tests/host/map_commit_plan.cpp && ./map_commit_plan.exe
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cape_map_commit.h"

namespace {

constexpr int W = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
constexpr uint32_t kHostBits[5] = {CAPE_UNION_HOST_MAP_HOLES, CAPE_UNION_HOST_NEW_HOLE, CAPE_UNION_HOST_CAPACITY, CAPE_UNION_HOST_AMBIGUOUS,
                                   CAPE_UNION_HOST_HOLE_CUT};

struct Frame
{
    std::vector<cape_map_plane> planes;
    std::vector<cape_map_ring> rings;
    int64_t nVertices = 0;
    cape_frame_map_kalman hd{};
    std::vector<cape_map_track_result> tr;
    std::vector<cape_plane_fusion> fusion = std::vector<cape_plane_fusion>(W);
    std::vector<cape_plane_measurement> meas = std::vector<cape_plane_measurement>(W);
    std::vector<cape_plane_union> rows = std::vector<cape_plane_union>(W);
    std::vector<cape_plane_union_rings> ringRows = std::vector<cape_plane_union_rings>(W);
    bool plain = false;
    uint32_t flags = 0;
};

Frame make(std::mt19937_64& gen, int nMap, int round)
{
    auto pick = [&](int lo, int hi) { return (int)(lo + gen() % (uint64_t)(hi - lo + 1)); };
    Frame f;
    f.plain = round % 3 == 1;
    f.flags = round % 2 ? (uint32_t)CAPE_COMMIT_ADD_STAGED : 0u;
    f.planes.resize(nMap);
    f.tr.resize(nMap);
    for (int j = 0; j < nMap; ++j)
    {
        cape_map_plane& M = f.planes[j];
        std::memset(&M, 0, sizeof(M));
        M.ring_first = (uint32_t)f.rings.size();
        M.ring_count = pick(0, 9) ? 1u : (uint32_t)pick(1, 9);
        for (uint32_t k = 0; k < M.ring_count; ++k)
        {
            const uint32_t n = (uint32_t)pick(3, k ? 12 : 40);
            f.rings.push_back(cape_map_ring {(uint32_t)f.nVertices, n});
            f.nVertices += n;
        }
        f.tr[j] = cape_map_track_result {0u, 0, 0u, -1};
    }
    // a few broken planes in the later rounds: rings outside the map
    if (round >= 6 && nMap > 0)
    {
        cape_map_plane& M = f.planes[pick(0, nMap - 1)];
        if (round % 2)
            M.ring_first = (uint32_t)f.rings.size();
        else
            M.ring_count = 10;
    }
    const int nCur = round == 5 ? 0 : pick(0, W);
    f.hd.n_map = nMap;
    f.hd.n_cur = round == 4 ? W + 7 : nCur; // (beyond 128 only with the wide match's overflow flag)
    f.hd.flags = round == 4 ? (uint32_t)CAPE_MATCH_EXACT_OVERFLOW : (round == 3 ? (uint32_t)CAPE_KALMAN_BAD_POSE_COV : 0u);
    uint32_t slabAt = 0;
    for (int i = 0; i < nCur; ++i)
    {
        cape_plane_fusion& F = f.fusion[i];
        cape_plane_measurement& m = f.meas[i];
        cape_plane_union& U = f.rows[i];
        cape_plane_union_rings& R = f.ringRows[i];
        F.map_plane = U.map_plane = -1;
        m.flags = CAPE_MEASURE_KEPT | (pick(0, 3) ? (uint32_t)CAPE_MEASURE_STAGEABLE : (uint32_t)CAPE_MEASURE_RING_TOO_LONG);
        m.vertex_count = pick(0, 40) ? (uint32_t)pick(3, 60) : (uint32_t)pick(0, 2);
        m.vertex_offset = (uint32_t)pick(0, 1000);
        if (nMap > 0 && pick(0, 2))
        {
            const int j = pick(0, nMap - 1);
            if (f.tr[j].kept_plane < 0)
            {
                f.tr[j].kept_plane = pick(0, 30) ? i : i + 1; // (sometimes another plane's, or one past the frame's)
                F.map_plane = pick(0, 30) ? j : (j + 1) % nMap;
                F.flags = (pick(0, 5) ? (uint32_t)CAPE_FUSION_STATE : 0u) | (pick(0, 5) ? (uint32_t)CAPE_FUSION_FRAME : 0u) | (uint32_t)CAPE_FUSION_USED;
                if (round < 2 || pick(0, 9)) // (the first two kinds of frame are refused by nothing)
                    U.map_plane = j;
                const int kind = round < 2 ? 0 : pick(0, 9);
                if (kind <= 6)
                    U.flags = CAPE_UNION_SERVED | (pick(0, 1) ? (uint32_t)CAPE_UNION_HOLES : 0u);
                else if (kind <= 8)
                    U.flags = kHostBits[pick(0, 4)];
                R.ring_count = f.plain ? 0u : (uint32_t)(pick(0, 4) ? 1 : pick(1, 9));
                uint32_t total = 0;
                for (uint32_t k = 0; k < R.ring_count && k < 9u; ++k)
                    total += R.vertex_count[k] = (uint32_t)pick(3, 30);
                U.vertex_count = f.plain ? (uint32_t)pick(3, 30) : R.vertex_count[0];
                if (f.plain)
                    total = U.vertex_count;
                U.vertex_offset = slabAt;
                slabAt += total;
                // broken rows, now and then: the commit hands such a pair to the host
                const int broken = round < 2 ? 0 : pick(0, 40);
                if (broken == 1)
                    R.ring_count = f.plain ? 0u : 10u, U.vertex_count = f.plain ? 2u : U.vertex_count;
                if (broken == 2)
                    U.vertex_count += 1;
                if (broken == 3)
                    U.vertex_offset = CAPE_MAP_UNION_FRAME_VERTICES - 2;
                if (broken == 4 && !f.plain)
                    R.vertex_count[R.ring_count - 1] = 2;
            }
        }
        if (F.map_plane < 0 && pick(0, 6) == 0)
            F.flags = CAPE_FUSION_USED; // (cannot happen: an unmatched plane nobody used; the rule is the flag's alone)
    }
    return f;
}

// ---- the naive loop: the rules as include/cape_hip.h states them, the offsets summed from scratch
struct Naive
{
    std::vector<cape::CommitPlanRow> rows;
    cape_map_commit_result result{};
};

bool naive_union_rings(const Frame& f, int i, std::vector<uint32_t>& counts)
{
    const cape_plane_union& U = f.rows[i];
    counts.clear();
    if (f.plain)
        counts.push_back(U.vertex_count);
    else
    {
        const cape_plane_union_rings& R = f.ringRows[i];
        if (R.ring_count < 1 || R.ring_count > 9)
            return false;
        counts.assign(R.vertex_count, R.vertex_count + R.ring_count);
        if (counts[0] != U.vertex_count)
            return false;
    }
    uint64_t total = 0;
    for (uint32_t n : counts)
    {
        if (n < 3 || n > CAPE_MAP_MAX_RING)
            return false;
        total += n;
    }
    return (uint64_t)U.vertex_offset + total <= CAPE_MAP_UNION_FRAME_VERTICES;
}

Naive naive(const Frame& f, int frame, uint64_t nextId)
{
    Naive out;
    const int nMap = (int)f.planes.size();
    const bool overflow = (f.hd.flags & CAPE_MATCH_EXACT_OVERFLOW) != 0;
    const int nCur = overflow ? 0 : (f.hd.n_cur < 0 ? 0 : (f.hd.n_cur > W ? W : f.hd.n_cur));
    uint32_t refusal = (overflow ? (uint32_t)CAPE_COMMIT_FRAME_OVERFLOW : 0u) | ((f.hd.flags & CAPE_KALMAN_BAD_POSE_COV) ? (uint32_t)CAPE_COMMIT_BAD_POSE_COV : 0u);
    int updated = 0, hostPairs = 0, failPolygon = 0, appended = 0;
    struct Size
    {
        uint32_t rings, vertices;
    };
    std::vector<Size> sizes;
    for (int j = 0; j < nMap; ++j)
    {
        const cape_map_plane& M = f.planes[j];
        const int i = f.tr[j].kept_plane;
        cape::CommitPlanRow row{};
        row.source = cape::kCommitFromMap;
        row.index = (uint32_t)j;
        bool fromMap = true;
        if (i >= 0 && i < nCur && f.fusion[i].map_plane == j && (f.fusion[i].flags & CAPE_FUSION_STATE))
        {
            const cape_plane_union& U = f.rows[i];
            std::vector<uint32_t> counts;
            bool hostBit = false;
            for (uint32_t b : kHostBits)
                hostBit = hostBit || (U.flags & b);
            if (U.map_plane != j)
                refusal |= CAPE_COMMIT_FAIL_POLYGON, ++failPolygon;
            else if (U.flags & CAPE_UNION_SERVED)
            {
                if (naive_union_rings(f, i, counts))
                {
                    fromMap = false;
                    row.source = cape::kCommitFromUnion;
                    row.index = (uint32_t)i;
                    row.ringCount = (uint32_t)counts.size();
                    for (uint32_t n : counts)
                        row.vertexCount += n;
                    row.srcVertex = U.vertex_offset;
                    ++updated;
                }
                else
                    refusal |= CAPE_COMMIT_HOST_PAIR, ++hostPairs;
            }
            else if (hostBit)
                refusal |= CAPE_COMMIT_HOST_PAIR, ++hostPairs;
            else
                refusal |= CAPE_COMMIT_FAIL_POLYGON, ++failPolygon;
        }
        if (fromMap)
        {
            bool ok = M.ring_count >= 1 && M.ring_count <= 9 && (uint64_t)M.ring_first + M.ring_count <= f.rings.size();
            uint32_t total = 0;
            for (uint32_t k = 0; ok && k < M.ring_count; ++k)
            {
                const cape_map_ring r = f.rings[M.ring_first + k];
                ok = r.vertex_count <= CAPE_MAP_MAX_RING && (int64_t)r.vertex_offset + r.vertex_count <= f.nVertices;
                total += r.vertex_count;
            }
            if (!ok)
                refusal |= CAPE_COMMIT_CAPACITY;
            else
                row.ringCount = M.ring_count, row.vertexCount = total;
        }
        out.rows.push_back(row);
        sizes.push_back(Size {row.ringCount, row.vertexCount});
    }
    if (f.flags & CAPE_COMMIT_ADD_STAGED)
        for (int i = 0; i < nCur; ++i)
        {
            const cape_plane_measurement& m = f.meas[i];
            if ((f.fusion[i].flags & CAPE_FUSION_USED) || !(m.flags & CAPE_MEASURE_STAGEABLE) || m.vertex_count < 3 || m.vertex_count > CAPE_MAP_MAX_RING)
                continue;
            cape::CommitPlanRow row{};
            row.source = cape::kCommitFromMeasure;
            row.index = row.srcRow = (uint32_t)i;
            row.ringCount = 1;
            row.vertexCount = m.vertex_count;
            for (int k = 0; k < i; ++k)
                row.srcVertex += f.meas[k].vertex_count;
            out.rows.push_back(row);
            sizes.push_back(Size {1u, m.vertex_count});
            ++appended;
        }
    int64_t rings = 0, vertices = 0;
    for (size_t b = 0; b < out.rows.size(); ++b)
    {
        uint32_t r = 0, v = 0;
        for (size_t k = 0; k < b; ++k) // (from plane 0 again: no running sum to get wrong)
            r += sizes[k].rings, v += sizes[k].vertices;
        out.rows[b].ringFirst = r;
        out.rows[b].vertexFirst = v;
        rings += sizes[b].rings;
        vertices += sizes[b].vertices;
    }
    if ((int)out.rows.size() > CAPE_MAP_MAX_PLANES)
        refusal |= CAPE_COMMIT_CAPACITY;
    const bool done = refusal == 0;
    cape_map_commit_result& R = out.result;
    R.flags = done ? (uint32_t)CAPE_COMMIT_DONE : refusal;
    R.frame = frame;
    R.n_planes = done ? (int32_t)out.rows.size() : nMap;
    R.n_rings = done ? (int32_t)rings : (int32_t)f.rings.size();
    R.n_vertices = done ? vertices : f.nVertices;
    R.n_updated = updated;
    R.n_appended = appended;
    R.n_host_pairs = hostPairs;
    R.n_fail_polygon = failPolygon;
    R.next_id = nextId + (done ? (uint64_t)appended : 0u);
    return out;
}

} // namespace

int main()
{
    std::mt19937_64 gen(20240607);
    const int widths[6] = {0, 1, 255, 256, 257, 1024};
    long frames = 0, done = 0, differ = 0, refusals[6] = {0, 0, 0, 0, 0, 0};
    for (int nMap : widths)
        for (int round = 0; round < 40; ++round)
        {
            const Frame f = make(gen, nMap, round % 8);
            const uint64_t nextId = 1000 + round;
            std::vector<cape::CommitPlanRow> rows((size_t)nMap + cape::kCommitMaxAppended);
            const uint64_t unbounded = ~(uint64_t)0;
            const cape_map_commit_result got =
                cape::commit_plan_serial(f.planes.data(), nMap, f.rings.data(), (int32_t)f.rings.size(), f.nVertices, round, f.hd, f.tr.data(),
                                         f.fusion.data(), f.meas.data(), f.rows.data(), f.plain ? nullptr : f.ringRows.data(), f.flags, nextId, unbounded,
                                         unbounded, unbounded, rows.data());
            const Naive want = naive(f, round, nextId);
            bool same = std::memcmp(&got, &want.result, sizeof(got)) == 0;
            if (same && (got.flags & CAPE_COMMIT_DONE))
                for (int b = 0; b < got.n_planes && same; ++b)
                    same = std::memcmp(&rows[b], &want.rows[b], sizeof(cape::CommitPlanRow)) == 0;
            ++frames;
            done += (got.flags & CAPE_COMMIT_DONE) != 0;
            for (int bit = 0; bit < 6; ++bit)
                refusals[bit] += (got.flags >> bit) & 1u;
            if (!same)
            {
                ++differ;
                std::printf("differs: %d planes, round %d: flags %#x / %#x, planes %d / %d, rings %d / %d, vertices %lld / %lld, counts %d %d %d %d / %d %d %d %d\n",
                            nMap, round, got.flags, want.result.flags, got.n_planes, want.result.n_planes, got.n_rings, want.result.n_rings,
                            (long long)got.n_vertices, (long long)want.result.n_vertices, got.n_updated, got.n_appended, got.n_host_pairs,
                            got.n_fail_polygon, want.result.n_updated, want.result.n_appended, want.result.n_host_pairs, want.result.n_fail_polygon);
            }
        }
    // the capacity rule at its edge: 1024 - k planes and k or k + 1 stageable detections
    for (int k : {1, 37, 128})
        for (int extra = 0; extra < 2; ++extra)
        {
            if (k + extra > W)
                continue;
            Frame f = make(gen, CAPE_MAP_MAX_PLANES - k, 5);
            f.flags = CAPE_COMMIT_ADD_STAGED;
            f.hd.n_cur = k + extra;
            for (int i = 0; i < k + extra; ++i)
            {
                f.fusion[i].map_plane = -1;
                f.meas[i].flags = CAPE_MEASURE_KEPT | CAPE_MEASURE_STAGEABLE;
                f.meas[i].vertex_count = 4;
            }
            std::vector<cape::CommitPlanRow> rows((size_t)CAPE_MAP_MAX_PLANES + cape::kCommitMaxAppended);
            const uint64_t unbounded = ~(uint64_t)0;
            const cape_map_commit_result got =
                cape::commit_plan_serial(f.planes.data(), (int32_t)f.planes.size(), f.rings.data(), (int32_t)f.rings.size(), f.nVertices, 0, f.hd,
                                         f.tr.data(), f.fusion.data(), f.meas.data(), f.rows.data(), nullptr, f.flags, 7, unbounded, unbounded, unbounded,
                                         rows.data());
            const Naive want = naive(f, 0, 7);
            const bool edge = extra ? got.flags == CAPE_COMMIT_CAPACITY && got.n_planes == CAPE_MAP_MAX_PLANES - k
                                    : got.flags == CAPE_COMMIT_DONE && got.n_planes == CAPE_MAP_MAX_PLANES && got.next_id == 7u + (uint64_t)k;
            ++frames;
            if (!edge || std::memcmp(&got, &want.result, sizeof(got)) != 0)
            {
                ++differ;
                std::printf("differs at the capacity edge: k %d, extra %d, flags %#x, planes %d\n", k, extra, got.flags, got.n_planes);
            }
        }
    std::printf("frames: %ld, of them DONE: %ld; refused for FRAME_OVERFLOW %ld, BAD_POSE_COV %ld, HOST_PAIR %ld, FAIL_POLYGON %ld, CAPACITY %ld\n", frames,
                done, refusals[1], refusals[2], refusals[3], refusals[4], refusals[5]);
    std::printf("frames whose plan differs from the naive loop: %ld\n", differ);
    return differ == 0 ? 0 : 1;
}
