// The hand-off of cape_map_step (csrc/cape_map_step.h: step_map_after) compiled for the HOST between the two serial plans it joins:
// commit_plan_serial (cape_map_commit.h) on a map and a frame's appends, its rows applied as the commit's copy kernel applies them,
// then -- on the set, with the counts and only if step_map_after says so, its maintain header still all zero -- maintain_plan_serial
// (cape_map_maintain.h) on the committed map with the capacities and log bounds the step's kernels derive (maintain_log_bounds), its
// rows applied as the maintenance's copy kernel applies them, then step_map_after again with both headers: where the map lies, and
// what it holds.  Compared with a naive loop that appends and then partitions a plain list of planes.  Maps of 0, 1, 255, 256, 257,
// 1020 and 1024 planes with up to four appended planes, so that the committed count crosses 256 and reaches 1024 (and, from 1024,
// is refused).  Every outcome of the step's table must occur: the program asserts it.  Under the address and undefined-behaviour
// sanitizers.  A stand-alone program: tests/host/hip_stub stands in for the HIP runtime header.  Build and run from the repository
// root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc
//       -o map_step_plan.exe tests/host/map_step_plan.cpp && ./map_step_plan.exe
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cape_map_step.h"

namespace {

// one buffer set of the map: planes, rings, vertices (one double each: a vertex's identity), tracks
struct Set
{
    std::vector<cape_map_plane> planes;
    std::vector<cape_map_ring> rings;
    std::vector<double> vertices;
    std::vector<cape_map_track> tracks;
    void room(size_t p, size_t r, size_t v)
    {
        planes.assign(p, cape_map_plane{});
        rings.assign(r, cape_map_ring{});
        vertices.assign(v, -1.0);
        tracks.assign(p, cape_map_track{});
    }
};

// a plane of the naive route: its identity (kept in cape_map_plane::d), its rings, its track
struct Entry
{
    double id;
    std::vector<std::vector<double>> rings;
    cape_map_track track;
};

bool same_track(const cape_map_track& a, const cape_map_track& b)
{
    return a.flags == b.flags && a.successive_matched == b.successive_matched && a.failed_tracking == b.failed_tracking && a.id == b.id;
}

// the first `planes` planes of a set as a list, or false if rings and vertices are not laid out plane after plane, back to back, or
// the counts do not agree with it
bool entries_of(const Set& s, int32_t planes, int32_t rings, int64_t vertices, std::vector<Entry>& out)
{
    uint32_t ring = 0, vertex = 0;
    out.clear();
    for (int32_t j = 0; j < planes; ++j)
    {
        const cape_map_plane& P = s.planes[j];
        if (P.ring_first != ring)
            return false;
        Entry e{P.d, {}, s.tracks[j]};
        for (uint32_t k = 0; k < P.ring_count; ++k, ++ring)
        {
            const cape_map_ring r = s.rings[ring];
            if (r.vertex_offset != vertex)
                return false;
            e.rings.emplace_back(s.vertices.begin() + vertex, s.vertices.begin() + vertex + r.vertex_count);
            vertex += r.vertex_count;
        }
        out.push_back(e);
    }
    return (int32_t)ring == rings && (int64_t)vertex == vertices;
}

bool same_list(const std::vector<Entry>& a, const std::vector<Entry>& b)
{
    if (a.size() != b.size())
        return false;
    for (size_t j = 0; j < a.size(); ++j)
        if (a[j].id != b[j].id || a[j].rings != b[j].rings || !same_track(a[j].track, b[j].track))
            return false;
    return true;
}

struct Case
{
    Set front;
    int32_t nRings = 0;
    int64_t nVertices = 0;
    // the frame: its header, one track result per map plane (no pair: the commit's served pairs are map_commit_plan.cpp's), its kept
    // planes' fusion rows and measurement rows, the world rings back to back
    cape_frame_map_kalman hd{};
    std::vector<cape_map_track_result> results;
    std::vector<cape_plane_fusion> fusion;
    std::vector<cape_plane_measurement> measurements;
    std::vector<double> world;
    uint32_t commitFlags = 0;
    uint64_t nextId = 0;
    cape::MaintainCursor held{};
    std::vector<uint8_t> promotable; // per identity: old planes by index, appended ones are never candidates
};

// round: 0 .. 2 random classes; 3 nothing due; 4 the log nearly or quite full; 5 no CAPE_COMMIT_ADD_STAGED; 6 a frame the header refuses
Case make(std::mt19937_64& gen, int nMap, int round)
{
    auto pick = [&](int lo, int hi) { return (int)(lo + gen() % (uint64_t)(hi - lo + 1)); };
    Case c;
    double next = 1.0;
    c.front.room((size_t)nMap, (size_t)nMap * 9, (size_t)nMap * 84 + 64);
    c.promotable.resize((size_t)nMap + 8, 0);
    for (int j = 0; j < nMap; ++j)
    {
        cape_map_plane& M = c.front.planes[j];
        M.d = (double)j;
        M.ring_first = (uint32_t)c.nRings;
        M.ring_count = pick(0, 9) ? 1u : (uint32_t)pick(2, 9);
        for (uint32_t k = 0; k < M.ring_count; ++k)
        {
            const uint32_t n = (uint32_t)pick(3, k ? 8 : 20);
            c.front.rings[c.nRings++] = cape_map_ring {(uint32_t)c.nVertices, n};
            for (uint32_t v = 0; v < n; ++v)
                c.front.vertices[c.nVertices++] = next++;
        }
        cape_map_track& T = c.front.tracks[j];
        const bool staged = pick(0, 1) != 0;
        T.flags = staged ? (uint32_t)CAPE_MAP_TRACK_STAGED : 0u;
        if (round == 3 || round == 4)
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
        c.promotable[j] = (uint8_t)(pick(0, 3) != 0);
    }
    if (round == 4 && nMap > 0) // one local plane is lost: the log decides
    {
        cape_map_track& T = c.front.tracks[pick(0, nMap - 1)];
        T.flags = 0;
        T.failed_tracking = 11;
    }
    c.results.assign((size_t)std::max(nMap, 1), cape_map_track_result{});
    for (auto& r : c.results)
        r.kept_plane = -1;
    const bool four = nMap == 1020; // exactly four appends: the committed map reaches 1 024 planes
    const int nCur = four ? pick(4, 6) : pick(1, 6);
    c.hd.n_cur = nCur;
    c.hd.flags = round == 6 ? (uint32_t)CAPE_KALMAN_BAD_POSE_COV : 0u;
    c.fusion.assign((size_t)nCur, cape_plane_fusion{});
    c.measurements.assign((size_t)nCur, cape_plane_measurement{});
    int appends = 0;
    for (int i = 0; i < nCur; ++i)
    {
        c.fusion[i].map_plane = -1;
        cape_plane_measurement& m = c.measurements[i];
        m.vertex_count = (uint32_t)pick(3, 12);
        m.vertex_offset = 0;
        const bool stage = four ? i < 4 : appends < 4 && pick(0, 2) != 0;
        m.flags = stage ? (uint32_t)CAPE_MEASURE_STAGEABLE : 0u;
        c.fusion[i].flags = four || pick(0, 4) ? 0u : (uint32_t)CAPE_FUSION_USED;
        appends += stage && !(c.fusion[i].flags & CAPE_FUSION_USED);
        for (uint32_t v = 0; v < m.vertex_count; ++v)
            c.world.push_back(next++);
    }
    c.commitFlags = round == 5 ? 0u : (uint32_t)CAPE_COMMIT_ADD_STAGED;
    c.nextId = 5000;
    c.held = cape::MaintainCursor {pick(0, 50), pick(50, 90), pick(900, 1000)};
    if (round == 4)
        c.held.planes = CAPE_MAP_RETIRED_MAX_PLANES - pick(0, 1);
    return c;
}

constexpr double kAppendedId = 1.0e6; // + kept plane: the identity of an appended plane

// ---- the naive route: a list, appended to and then partitioned
struct Outcome
{
    bool committed = false, maintained = false, refusedMaintain = false;
    std::vector<Entry> map, log; // the log: this call's lost planes
};

Outcome naive(const Case& c, int nMap)
{
    Outcome o;
    std::vector<Entry> list;
    { // (the front set is laid out back to back by construction)
        bool ok = entries_of(c.front, nMap, c.nRings, c.nVertices, list);
        if (!ok)
            std::printf("the generated map is not laid out back to back\n");
    }
    o.map = list;
    if (c.hd.flags & (CAPE_KALMAN_BAD_POSE_COV | CAPE_MATCH_EXACT_OVERFLOW))
        return o;
    size_t world = 0;
    uint64_t id = c.nextId;
    for (int i = 0; i < c.hd.n_cur; ++i)
    {
        const cape_plane_measurement& m = c.measurements[i];
        if ((c.commitFlags & CAPE_COMMIT_ADD_STAGED) && !(c.fusion[i].flags & CAPE_FUSION_USED) && (m.flags & CAPE_MEASURE_STAGEABLE))
        {
            Entry e{kAppendedId + i, {std::vector<double>(c.world.begin() + world, c.world.begin() + world + m.vertex_count)}, cape_map_track{}};
            e.track.flags = CAPE_MAP_TRACK_STAGED;
            e.track.id = id++;
            list.push_back(e);
        }
        world += m.vertex_count;
    }
    if (list.size() > (size_t)CAPE_MAP_MAX_PLANES)
        return o;
    o.committed = true;
    o.map = list;
    // the maintenance of the committed list
    std::vector<Entry> local, staged, lost;
    bool due = false;
    for (const Entry& e : list)
    {
        const cape_map_track& T = e.track;
        const bool ok = e.id < kAppendedId && c.promotable[(size_t)e.id] != 0;
        const uint32_t cls = cape::maintain_class(T.flags, T.successive_matched, T.failed_tracking, ok);
        Entry out = e;
        if (cls == cape::kMaintainPromoted)
        {
            out.track.flags &= ~(uint32_t)CAPE_MAP_TRACK_STAGED;
            out.track.failed_tracking = 0;
        }
        due = due || cls == cape::kMaintainPromoted || cls == cape::kMaintainDropped || cls == cape::kMaintainLost;
        if (cls == cape::kMaintainKeepLocal || cls == cape::kMaintainPromoted)
            local.push_back(out);
        else if (cls == cape::kMaintainKeepStaged || cls == cape::kMaintainPromoteRefused)
            staged.push_back(out);
        else if (cls == cape::kMaintainLost)
            lost.push_back(out);
    }
    if (!lost.empty() && (size_t)c.held.planes + lost.size() > (size_t)CAPE_MAP_RETIRED_MAX_PLANES)
    {
        o.refusedMaintain = true;
        return o;
    }
    if (!due)
        return o;
    o.maintained = true;
    o.map = local;
    o.map.insert(o.map.end(), staged.begin(), staged.end());
    o.log = lost;
    return o;
}

// ---- the step's route: the two serial plans with the hand-off between them, their rows applied as the copy kernels apply them
void copy_rings(const Set& from, const cape_map_plane& M, Set& to, uint32_t ringFirst, uint32_t vertexFirst)
{
    uint32_t at = 0;
    for (uint32_t k = 0; k < M.ring_count; ++k)
    {
        const cape_map_ring r = from.rings[M.ring_first + k];
        for (uint32_t v = 0; v < r.vertex_count; ++v)
            to.vertices.at((size_t)vertexFirst + at + v) = from.vertices[r.vertex_offset + v];
        to.rings.at(ringFirst + k) = cape_map_ring {vertexFirst + at, r.vertex_count};
        at += r.vertex_count;
    }
}

struct Stepped
{
    cape_map_commit_result commit{};
    cape_map_maintain_result maintain{};
    cape::StepMapState after{};
    Set sets[3];
    Set log; // indexed from what the log holds: room for held + this call's
};

Stepped stepped(const Case& c, int nMap)
{
    Stepped s;
    s.sets[cape::kStepSetFront] = c.front;
    // the bounds the host knows: 128 appended planes, their rings, the frame's world rings
    const size_t planesCap = std::min<size_t>(CAPE_MAP_MAX_PLANES, (size_t)nMap + cape::kCommitMaxAppended), ringsCap = planesCap * cape::kCommitMaxRings,
                 verticesCap = (size_t)c.nVertices + c.world.size();
    s.sets[cape::kStepSetBack].room(planesCap, ringsCap, verticesCap);
    s.sets[cape::kStepSetThird].room(planesCap, ringsCap, verticesCap);
    std::vector<cape::CommitPlanRow> rows((size_t)nMap + cape::kCommitMaxAppended);
    std::vector<cape_plane_union> noUnion(1);
    s.commit = cape::commit_plan_serial(c.front.planes.data(), nMap, c.front.rings.data(), c.nRings, c.nVertices, 3, c.hd, c.results.data(), c.fusion.data(),
                                        c.measurements.data(), noUnion.data(), nullptr, c.commitFlags, c.nextId, planesCap, ringsCap, verticesCap, rows.data());
    if (s.commit.flags & CAPE_COMMIT_DONE)
    {
        Set& back = s.sets[cape::kStepSetBack];
        uint64_t id = c.nextId;
        for (int32_t b = 0; b < s.commit.n_planes; ++b)
        {
            const cape::CommitPlanRow& r = rows[b];
            cape_map_plane& P = back.planes.at(b);
            if (r.source == cape::kCommitFromMap)
            {
                P = c.front.planes[r.index];
                copy_rings(c.front, c.front.planes[r.index], back, r.ringFirst, r.vertexFirst);
                back.tracks.at(b) = c.front.tracks[r.index];
            }
            else
            {
                P = cape_map_plane{};
                P.d = kAppendedId + r.srcRow;
                for (uint32_t v = 0; v < r.vertexCount; ++v)
                    back.vertices.at((size_t)r.vertexFirst + v) = c.world.at(r.srcVertex + v);
                back.rings.at(r.ringFirst) = cape_map_ring {r.vertexFirst, r.vertexCount};
                back.tracks.at(b) = cape_map_track{};
                back.tracks.at(b).flags = CAPE_MAP_TRACK_STAGED;
                back.tracks.at(b).id = id++;
            }
            P.ring_first = r.ringFirst;
            P.ring_count = r.ringCount;
        }
    }
    // the hand-off: the state after the commit alone is the maintenance's source, or it does not run
    const cape::StepMapState from = cape::step_map_after(s.commit, cape_map_maintain_result{});
    if (from.set == cape::kStepSetBack)
    {
        const Set& src = s.sets[from.set];
        const cape::MaintainLog log = cape::maintain_log_bounds(c.held, (uint64_t)from.planes, (uint64_t)from.rings, (uint64_t)from.vertices);
        s.log.room((size_t)log.planesCapacity, (size_t)log.ringsCapacity, (size_t)log.verticesCapacity);
        std::vector<uint8_t> promotable((size_t)from.planes);
        for (int32_t j = 0; j < from.planes; ++j)
            promotable[j] = src.planes[j].d < kAppendedId ? c.promotable[(size_t)src.planes[j].d] : 0;
        std::vector<cape::MaintainPlanRow> plan((size_t)from.planes + 1);
        s.maintain = cape::maintain_plan_serial(src.planes.data(), from.planes, src.rings.data(), from.rings, from.vertices, src.tracks.data(), promotable.data(),
                                                (uint64_t)from.planes, (uint64_t)from.rings, (uint64_t)from.vertices, log, plan.data());
        if (s.maintain.flags & CAPE_MAINTAIN_DONE)
            for (int32_t j = 0; j < from.planes; ++j)
            {
                const cape::MaintainPlanRow& r = plan[j];
                if (r.dest == cape::kMaintainToNone)
                    continue;
                Set& to = r.dest == cape::kMaintainToLog ? s.log : s.sets[cape::kStepSetThird];
                copy_rings(src, src.planes[j], to, r.ringFirst, r.vertexFirst);
                cape_map_plane& P = to.planes.at(r.plane);
                P = src.planes[j];
                P.ring_first = r.ringFirst;
                P.ring_count = r.ringCount;
                cape_map_track T = src.tracks[j];
                if (r.edit == cape::kMaintainEditPromote)
                {
                    T.flags &= ~(uint32_t)CAPE_MAP_TRACK_STAGED;
                    T.failed_tracking = 0;
                }
                to.tracks.at(r.plane) = T;
            }
    }
    s.after = cape::step_map_after(s.commit, s.maintain);
    return s;
}

// the planes the call logged, from the log's arrays (they start where the log stood)
bool logged(const Stepped& s, const cape::MaintainCursor& held, std::vector<Entry>& out)
{
    out.clear();
    if (!(s.maintain.flags & CAPE_MAINTAIN_DONE))
        return true;
    uint32_t ring = (uint32_t)held.rings, vertex = (uint32_t)held.vertices;
    for (int32_t j = held.planes; j < s.maintain.n_retired; ++j)
    {
        const cape_map_plane& P = s.log.planes.at(j);
        if (P.ring_first != ring)
            return false;
        Entry e{P.d, {}, s.log.tracks.at(j)};
        for (uint32_t k = 0; k < P.ring_count; ++k, ++ring)
        {
            const cape_map_ring r = s.log.rings.at(ring);
            if (r.vertex_offset != vertex)
                return false;
            e.rings.emplace_back(s.log.vertices.begin() + vertex, s.log.vertices.begin() + vertex + r.vertex_count);
            vertex += r.vertex_count;
        }
        out.push_back(e);
    }
    return (int32_t)ring == s.maintain.n_retired_rings && (int64_t)vertex == s.maintain.n_retired_vertices;
}

} // namespace

int main()
{
    std::mt19937_64 gen(20250314);
    const int widths[7] = {0, 1, 255, 256, 257, 1020, 1024};
    long cases = 0, differ = 0, refused = 0, doneNothing = 0, doneDone = 0, doneRefused = 0, across256 = 0, at1024 = 0;
    for (int nMap : widths)
        for (int round = 0; round < 42; ++round)
        {
            const Case c = make(gen, nMap, round % 7);
            const Outcome want = naive(c, nMap);
            const Stepped got = stepped(c, nMap);
            const bool committed = (got.commit.flags & CAPE_COMMIT_DONE) != 0, maintained = (got.maintain.flags & CAPE_MAINTAIN_DONE) != 0;
            const bool refusedMaintain = (got.maintain.flags & (CAPE_MAINTAIN_CAPACITY | CAPE_MAINTAIN_LOG_FULL)) != 0;
            bool same = committed == want.committed && maintained == want.maintained && refusedMaintain == want.refusedMaintain;
            // where the map lies: the front set behind a refused commit, the back set unless the maintenance is DONE, else the third
            same = same && got.after.set == (!committed ? cape::kStepSetFront : maintained ? cape::kStepSetThird : cape::kStepSetBack);
            if (!committed)
            {
                const cape_map_maintain_result zero{};
                same = same && std::memcmp(&got.maintain, &zero, sizeof(zero)) == 0 && got.commit.next_id == c.nextId;
            }
            std::vector<Entry> map, log;
            same = same && entries_of(got.sets[got.after.set], got.after.planes, got.after.rings, got.after.vertices, map) && same_list(map, want.map);
            same = same && logged(got, c.held, log) && same_list(log, want.log);
            if (committed)
                same = same && (refusedMaintain || maintained || got.maintain.flags == CAPE_MAINTAIN_NOTHING);
            ++cases;
            refused += !committed;
            doneNothing += committed && got.maintain.flags == CAPE_MAINTAIN_NOTHING;
            doneDone += committed && maintained;
            doneRefused += committed && refusedMaintain;
            across256 += committed && nMap <= 255 && got.commit.n_planes >= 256;
            at1024 += committed && nMap < 1024 && got.commit.n_planes == 1024;
            if (!same)
            {
                ++differ;
                std::printf("differs: %d planes, round %d: commit %#x (%d planes), maintain %#x (%d planes), set %u; naive: committed %d, maintained %d, %zu planes\n",
                            nMap, round, got.commit.flags, got.commit.n_planes, got.maintain.flags, got.maintain.n_planes, got.after.set, (int)want.committed,
                            (int)want.maintained, want.map.size());
            }
        }
    std::printf("cases: %ld; commit refused %ld, DONE + NOTHING %ld, DONE + DONE %ld, DONE + a refused maintenance %ld\n", cases, refused, doneNothing, doneDone,
                doneRefused);
    std::printf("committed counts that cross 256: %ld, that reach 1024 from below: %ld\n", across256, at1024);
    std::printf("cases whose step differs from the naive loop: %ld\n", differ);
    const bool all = refused > 0 && doneNothing > 0 && doneDone > 0 && doneRefused > 0 && across256 > 0 && at1024 > 0;
    if (!all)
        std::printf("an outcome of the table did not occur\n");
    return differ == 0 && all ? 0 : 1;
}
