// The kept planes of a frame over its whole record chain (cape_frame_header::next_record), shared by the wide matchers: the
// consecutive-frame one (cape_match_wide.hip) and the map one (cape_match_map.hip).  Both files compile their own copy (anonymous
// namespace; no device symbol crosses a file).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"

namespace cape {

namespace {

// what a chain walk reads: the batch's records followed by the spill pool's, and the polygon rows of both, indexed by the RECORD index
struct RecordChains
{
    const cape_frame_record* records;
    const cape_polygon* polygons; // records x CAPE_MAX_PLANES
    int maxBatch, nRecords;       // a link of a chain lies in [maxBatch, nRecords)
};

// The kept planes of a frame (output plane whose polygon Primitive_Detection keeps: valid_planes' rule) over its record chain, in
// record order, one wavefront per frame: table[k] = (record, segment in it) and segs[k] = the position in the frame's concatenated
// segment list of kept plane k < min(count, CAPE_MATCH_WIDE_MAX_PLANES); returns the count.  hostOnly: an output plane of the chain
// has no device polygon (CAPE_POLY_OVERFLOW).  A link outside the spill pool ends the chain, and a chain is followed through at most
// as many links as the pool has records.
__device__ __forceinline__ int walk_chain(const RecordChains& c, int frame, int lane, uint2* table, int* segs, bool& hostOnly)
{
    int kept = 0, segBase = 0, rec = frame;
    bool overflow = false;
    for (int hop = 0; hop <= c.nRecords - c.maxBatch; ++hop)
    {
        const cape_frame_record& R = c.records[rec];
        const cape_polygon* pol = c.polygons + (size_t)rec * CAPE_MAX_PLANES;
        int nSeg = R.header.n_plane_segments;
        nSeg = nSeg < 0 ? 0 : (nSeg > CAPE_MAX_PLANES ? CAPE_MAX_PLANES : nSeg);
        const bool isOut = lane < nSeg && R.segments[lane].is_output != 0;
        const unsigned flags = isOut ? pol[lane].flags : 0u;
        const bool ok = isOut && (flags & CAPE_POLY_VALID) != 0 && pol[lane].vertex_count >= 3;
        overflow = overflow || __ballot(isOut && (flags & CAPE_POLY_OVERFLOW) != 0) != 0ull;
        const unsigned long long m = __ballot(ok);
        const int rank = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && rank < CAPE_MATCH_WIDE_MAX_PLANES)
        {
            table[rank] = make_uint2((unsigned)rec, (unsigned)lane);
            segs[rank] = segBase + lane;
        }
        kept += __popcll(m);
        segBase += nSeg;
        const int next = R.header.next_record;
        if (next < c.maxBatch || next >= c.nRecords)
            break;
        rec = next;
    }
    hostOnly = overflow;
    return kept;
}

} // namespace

} // namespace cape
