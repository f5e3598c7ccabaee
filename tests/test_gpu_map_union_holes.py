"""cape_map_union_holes: the polygon half of the map update on the device for map planes that have interior rings and unions that
create some -- against its host twins cape_host_polygon_union (one pair through the debug entry) and cape_host_map_union_holes (fed
the device's own fusion and measurement rows), bit for bit, and against the whole host update.

As for cape_map_union, a frame that outgrows the 2 048-vertex slab is compared with the twin, which applies the same rule; the update
knows no slab.  Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest

from map_union_hole_cases import CAPACITY, HOLE_CUT, TABLES, holed_star_pairs, square_hole, tilted_frames
from test_gpu_map_kalman import _tracks, room  # noqa: F401  (the eight room frames after the four calls)
from test_gpu_map_union import _bits, _measurement_rows, _sans_nodes
from test_map_union_host import star_pairs

pytestmark = pytest.mark.gpu

W = 128
FLAG_NAMES = ("SERVED", "UNCHANGED", "DISJOINT", "MAP_HOLES", "NEW_HOLE", "CAPACITY", "AMBIGUOUS", "HOLES", "HOLE_CUT")


@pytest.fixture(scope="module")
def ex1():
    from cape_amd import Extractor, synth

    ex = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)
    yield ex
    ex.close()


def _same_polygon(a, b):
    return (a is None and b is None) or (a is not None and b is not None and len(a) == len(b)
                                         and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)))


def _one_pair(ca, ex, name, rings_a, b, frames, counts):
    """the debug entry against its twin: the row without n_nodes and the rings row byte for byte, every ring bit for bit, in order"""
    row, rr, poly = ex.debug_polygon_union(rings_a, b, frames)
    trow, trr, tpoly = ca.host_polygon_union(rings_a, b, frames)
    for bit in range(9):
        counts[bit] += bool(row["flags"] & (1 << bit))
    assert _sans_nodes(row).tobytes() == trow.tobytes(), f"{name}: {row} != {trow}"
    assert rr.tobytes() == trr.tobytes(), f"{name}: {rr} != {trr}"
    assert _same_polygon(poly, tpoly), f"{name}: rings"
    return row, rr, poly


# ---- 1. the debug entry against its twin on the tables ---------------------------------------------------------------------------
def test_debug_entry_equals_the_twin_on_the_tables(ex1, host_binaries):
    import cape_amd as ca

    counts = [0] * 9
    print()
    for name, rings_a, b, outcome in TABLES:
        row, rr, poly = _one_pair(ca, ex1, name, rings_a, b, None, counts)
        print(f"{name:48s} flags {int(row['flags']):#05x} rings {rr['vertex_count'][: rr['ring_count']].tolist()} new/kept/covered "
              f"{int(rr['holes_new'])}/{int(rr['holes_kept'])}/{int(rr['holes_covered'])} n_nodes {int(row['n_nodes'])}")
        if outcome == CAPACITY:
            assert row["flags"] == ca.UNION_HOST_CAPACITY, name
        elif outcome == HOLE_CUT:
            assert row["flags"] == ca.UNION_HOST_HOLE_CUT, name
        else:
            assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == outcome, name
        _one_pair(ca, ex1, name + " (tilted)", rings_a, b, tilted_frames(), counts)
    print(f"the tables, canonical and tilted frames: pairs per flag bit {dict(zip(FLAG_NAMES, counts))}")
    assert counts[3] == counts[4] == counts[6] == 0


# ---- 2. the star sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 24])
def test_debug_entry_equals_the_twin_on_star_sets_with_a_hole(ex1, host_binaries, n):
    import cape_amd as ca

    counts = [0] * 9
    kept = covered = 0
    for k, (rings_a, b) in enumerate(holed_star_pairs(n)):
        row, rr, _ = _one_pair(ca, ex1, f"star pair {k}", rings_a, b, None, counts)
        kept += bool(row["flags"] & ca.UNION_SERVED and rr["holes_kept"])
        covered += bool(row["flags"] & ca.UNION_SERVED and rr["holes_covered"])
    print(f"\n{n}-vertex stars with a hole: {kept} kept and served, {covered} covered and served, {counts[8]} partly covered; pairs per flag bit "
          f"{dict(zip(FLAG_NAMES, counts))}")
    assert counts[8] <= 20 and counts[5] == 0 and counts[6] == 0 and kept >= 20 and covered >= 20


@pytest.mark.parametrize("n", [8, 24])
def test_plain_star_sets_are_served_with_their_new_holes(ex1, host_binaries, n):
    import cape_amd as ca

    counts = [0] * 9
    for k, (a, b) in enumerate(star_pairs(n)):
        _one_pair(ca, ex1, f"star pair {k}", [a], b, None, counts)
    print(f"\n{n}-vertex stars: pairs per flag bit {dict(zip(FLAG_NAMES, counts))}")
    assert counts[0] == 200 and counts[7] == {8: 1, 24: 9}[n]


# ---- 3. order independence -------------------------------------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_the_pairs_before_it(ex1):
    """Every pair of the tables through the one handle in table order and again in reverse: a row, rings row or ring that differs read
    something an earlier pair left in the carve (the intersection's arrays borrow the cut lists, the nodes and the walked face; the
    interior rings and their lengths are written on demand)."""
    cases = [(name, rings_a, b, frames) for name, rings_a, b, _ in TABLES for frames in (None, tilted_frames())]
    forward = [ex1.debug_polygon_union(a, b, frames) for _, a, b, frames in cases]
    backward = [ex1.debug_polygon_union(a, b, frames) for _, a, b, frames in reversed(cases)][::-1]
    differ = [name + (" (tilted)" if frames is not None else "") for (name, _, _, frames), x, y in zip(cases, forward, backward)
              if x[0].tobytes() != y[0].tobytes() or x[1].tobytes() != y[1].tobytes() or not _same_polygon(x[2], y[2])]
    print(f"\n{len(cases)} pairs in table order and in reverse: {len(differ)} differ {differ}")
    assert not differ


# ---- 4. the frames kernel --------------------------------------------------------------------------------------------------------
def _grown(plane, factor=1.5):
    """the map plane with its ring grown about its vertex mean: a map plane that reaches beyond the detection it came from, so that a
    hole in its rim -- _holed(where=(0, 0.75)): at 0.75 * 1.5 = 1.125 times the distance of the detection's farthest vertex -- lies
    outside that detection and is kept"""
    nrm, d, x, y, c, ring, holes = plane
    mean = ring.mean(axis=0)
    return nrm, d, x, y, c, mean + factor * (ring - mean), holes


def _holed(ca, arrays, where=(0.0, 0.8), second_every=1):
    """The map with two square holes per plane, each with the largest side of 40, 20, 10, 5 that lies inside the ring (chosen here on
    the CPU; a place outside the ring, or too close to it, gets none).  The first sits at the ring's vertex mean.  A detection of the
    same plane covers the middle of its map plane in every frame of the streams used here (measured: 11 of 11 room pairs, with sides up
    to 1 000 too, where the rest are partly covered), so a second one sits four fifths of the way from the vertex mean to the vertex
    farthest from it, where a camera that has moved leaves some of them alone: 5 kept, 15 covered, 1 partly covered on the room
    frames.  second_every: only every so many planes get the second one (a frame's slab holds 2 048 vertices)."""
    P, R, V = arrays
    planes, holed = [], 0
    for j in range(len(P)):
        r = R[P[j]["ring_first"]]
        outer = V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]].copy()
        mean = outer.mean(axis=0)
        far = outer[np.argmax(np.linalg.norm(outer - mean, axis=1))]
        holes = []
        for centre in (mean + t * (far - mean) for t in (where if j % second_every == 0 else where[:1])):
            holes += [h for h in (square_hole([centre], side) for side in (40.0, 20.0, 10.0, 5.0)) if _inside(h, outer)][:1]
        holed += bool(holes)
        planes.append((P[j]["normal"], float(P[j]["d"]), P[j]["x_axis"], P[j]["y_axis"], P[j]["center"], outer, holes))
    return ca.pack_map(planes), holed


def _inside(hole, ring):
    """every vertex of the hole strictly inside the ring (crossing number), and no edge of the ring meeting an edge of the hole"""
    a, b = ring, np.roll(ring, -1, axis=0)
    for px, py in hole:
        with np.errstate(divide="ignore", invalid="ignore"):
            cross = ((a[:, 1] > py) != (b[:, 1] > py)) & (px < (b[:, 0] - a[:, 0]) * (py - a[:, 1]) / (b[:, 1] - a[:, 1]) + a[:, 0])
        if not cross.sum() & 1:
            return False

    def side(o, p, q):
        return (p[..., 0] - o[..., 0]) * (q[..., 1] - o[..., 1]) - (p[..., 1] - o[..., 1]) * (q[..., 0] - o[..., 0])

    for c, d in zip(hole, np.roll(hole, -1, axis=0)):
        if np.any((side(a, b, c) * side(a, b, d) <= 0) & (side(c, d, a) * side(c, d, b) <= 0)):
            return False
    return True


def _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, meas):
    """every frame of the last map_union_holes against cape_host_map_union_holes on the device's own rows"""
    out = ex.map_union_polygons(n)
    for f in range(n):
        rows, ring_rows, polys = out[f]
        n_cur = len(meas[f])
        mrows, worlds = _measurement_rows(ca, meas[f])
        trows, trings, tpolys = ca.host_map_union_holes(arrays, match[f], fusion[f, :n_cur], mrows, worlds)
        assert not rows[n_cur:].view(np.uint8).any() and not ring_rows[n_cur:].view(np.uint8).any(), f"frame {f}: rows beyond n_cur"
        for i in range(n_cur):
            assert _sans_nodes(rows[i]).tobytes() == trows[i].tobytes(), f"frame {f}, kept plane {i}: {rows[i]} != {trows[i]}"
            assert ring_rows[i].tobytes() == trings[i].tobytes(), f"frame {f}, kept plane {i}: {ring_rows[i]} != {trings[i]}"
            assert _same_polygon(polys[i], tpolys[i]), f"frame {f}, kept plane {i}: rings"
    return out


def test_room_frames_against_a_holed_map_equal_the_twin_and_the_update(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    try:
        arrays, holed = _holed(ca, room.arrays)
        ex.upload_map(arrays)
        ex.upload_tracks(room.tracks)
        ex.match_map_wide(n, room.W2C, None, room.flags, st)
        ex.map_kalman(n, st)
        _, match, _, _ = ex.map_matches_wide(n)
        _, fusion, _ = ex.map_kalman_rows(n)
        ex.map_union_holes(n, st)
        out = _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, room.meas)
        counts = [0] * 9
        served = with_holes = 0
        for f in range(n):
            rows, ring_rows, polys = out[f]
            n_cur = len(room.meas[f])
            for bit in range(9):
                counts[bit] += int(np.count_nonzero(rows[:n_cur][rows[:n_cur]["map_plane"] >= 0]["flags"] & (1 << bit)))
            # the served polygons lie back to back in kept-plane order
            at = 0
            for r, q in zip(rows[:n_cur], ring_rows[:n_cur]):
                if r["flags"] & ca.UNION_SERVED:
                    assert r["vertex_offset"] == at
                    at += int(q["vertex_count"].sum())
            # the whole update: the same rings, ring for ring, with the vertex counts of the update's new polygon
            det, _ = room.det[f]
            (P, R, V), Tr, _, _ = ca.host_map_update(arrays, room.tracks, match[f], det, room.T[f], room.S[f])
            for i in range(n_cur):
                j = int(rows[i]["map_plane"])
                if j < 0 or not rows[i]["flags"] & ca.UNION_SERVED:
                    continue
                want = [int(R[P[j]["ring_first"] + k]["vertex_count"]) for k in range(int(P[j]["ring_count"]))]
                assert not Tr[j]["result"] & ca.MAP_RESULT_OVERFLOW, f"frame {f}, map plane {j}"
                assert [len(r) for r in polys[i]] == want, f"frame {f}, map plane {j}: {[len(r) for r in polys[i]]} vertices, the update has {want}"
                served += 1
                with_holes += bool(rows[i]["flags"] & ca.UNION_HOLES)
        print(f"\nroom frames against a map of {len(arrays[0])} planes, {holed} of them with a hole: pairs per flag bit {dict(zip(FLAG_NAMES, counts))}; "
              f"{served} served pairs have the update's ring lengths, {with_holes} of them with interior rings")
        assert holed >= 1 and with_holes >= 1 and counts[8] >= 1 and counts[3] == counts[4] == counts[6] == 0
    
    finally:  # (the fixture is shared: the tests after this one see its own map again whatever happened here)
        room.restore()


# ---- 5. the chained frame --------------------------------------------------------------------------------------------------------
def test_a_chained_frame_against_a_holed_map_equals_the_twin():
    import cape_amd as ca
    from test_gpu_map_match import _w2c
    from test_gpu_map_measure import _pose_covariances
    from test_gpu_match_map_wide import _chained_input, _extract
    from test_map_update_host import _pose

    frames, Wd, Ht, intr = _chained_input()
    ex, st = _extract(frames, Wd, Ht, intr)
    n = len(frames)
    rng = np.random.default_rng(33)
    T, S = np.stack([_pose(rng) for _ in range(n)]), _pose_covariances(rng, n)
    W2C = np.stack([_w2c(T[f][:3, :3], T[f][:3, 3]) for f in range(n)])
    ex.map_measure(n, T, S, st)
    map_meas = [m for m in ex.map_measurements(n)[1] if m["flags"] & ca.MEASURE_STAGEABLE]
    tracks = _tracks(map_meas)
    meas = ex.map_measurements(n)
    # Two maps.  The planes as measured, with the two holes of the room test: each plane meets its own detection, which covers both
    # holes, and every pair with i >= 64 is served.  The planes grown about their vertex mean, the second hole in the rim the
    # detection does not reach: most pairs there are partly covered holes, and at least one pair with i >= 64 keeps a hole, so that
    # interior rings are written into the slab for a row of the upper half.
    figures = []
    for label, planes, where in (("as measured", [m["plane"] for m in map_meas], (0.0, 0.8)),
                                 ("grown", [_grown(m["plane"]) for m in map_meas], (0.0, 0.75))):
        arrays, holed = _holed(ca, ca.pack_map(planes), where=where)
        ex.upload_map(arrays)
        ex.upload_tracks(tracks)
        ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
        ex.map_kalman(n, st)
        ex.map_union_holes(n, st)
        _, fusion, _ = ex.map_kalman_rows(n)
        _, match, _, _ = ex.map_matches_wide(n)
        out = _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, meas)
        rows, ring_rows, _ = out[1]
        high = [i for i in range(64, len(meas[1])) if rows[i]["map_plane"] >= 0 and meas[1][i]["segment"] >= 64]
        served = [i for i in high if rows[i]["flags"] & ca.UNION_SERVED]
        with_holes = [i for i in range(len(meas[1])) if rows[i]["flags"] & ca.UNION_HOLES]
        high_holes = [i for i in served if rows[i]["flags"] & ca.UNION_HOLES and ring_rows[i]["holes_kept"]]
        print(f"\nchained frame against the map {label}, {holed} holed planes: {len(meas[1])} kept planes, "
              f"{int((rows['map_plane'][:len(meas[1])] >= 0).sum())} pairs, {len(high)} with i >= 64 and a ring in the spill record, {len(served)} of "
              f"them served (flags {sorted({int(rows[i]['flags']) for i in high})}), {len(with_holes)} pairs of the frame served with interior "
              f"rings, {len(high_holes)} of them with i >= 64 and a kept hole")
        assert len(high) >= 1 and len(served) >= 1 and holed >= 1
        figures.append((len(high), len(served), len(high_holes)))
    assert figures[0][1] == figures[0][0], "as measured, every pair with i >= 64 is served"
    assert figures[1][2] >= 1, "grown, a pair with i >= 64 keeps a hole"
    ex.close()


# ---- 6. the plain call after the holes call ----------------------------------------------------------------------------------------
def test_a_plain_union_after_the_holes_call_returns_its_own_rows(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    ex.map_union(n, st)
    plain = ex.map_union_rows(n)
    with pytest.raises(ca.CapeError, match=r"cape_copy_map_union_rings failed \(-4\)"):
        ex.map_union_ring_rows(1)
    ex.map_union_holes(n, st)
    holes_rows = ex.map_union_rows(n)[0]
    rings = ex.map_union_ring_rows(n)
    ptr = C.c_void_p()
    assert ex.L.cape_device_map_union_rings(ex.h, C.byref(ptr)) == 0 and ptr.value
    # what the plain call serves the holes call serves with the same row, one ring, wherever the slab has it; what the plain call
    # hands over for a new hole is served with interior rings
    served = (plain[0]["flags"] & ca.UNION_SERVED) != 0
    a, b = holes_rows[served].copy(), plain[0][served].copy()
    a["vertex_offset"] = b["vertex_offset"] = 0
    assert a.tobytes() == b.tobytes()
    assert np.all(rings["ring_count"][served] == 1)
    now = (holes_rows["flags"] & ca.UNION_SERVED) != 0
    assert np.all(rings["ring_count"][now] >= 1) and not rings["ring_count"][~now].any()
    assert not np.any(holes_rows["flags"] & (ca.UNION_HOST_NEW_HOLE | ca.UNION_HOST_MAP_HOLES))
    assert np.all(now[(plain[0]["flags"] & ca.UNION_HOST_NEW_HOLE) != 0] | ((holes_rows["flags"] & ca.UNION_HOST_CAPACITY) != 0)[(plain[0]["flags"] & ca.UNION_HOST_NEW_HOLE) != 0])
    ex.map_union(n, st)
    again = ex.map_union_rows(n)
    assert again[0].tobytes() == plain[0].tobytes()
    for f in range(n):
        used = int(plain[0][f]["vertex_count"].sum())
        assert np.array_equal(_bits(again[1][f, :used]), _bits(plain[1][f, :used]))
    with pytest.raises(ca.CapeError, match=r"cape_copy_map_union_rings failed \(-4\)"):
        ex.map_union_ring_rows(1)
    assert ex.L.cape_device_map_union_rings(ex.h, C.byref(ptr)) == -4
