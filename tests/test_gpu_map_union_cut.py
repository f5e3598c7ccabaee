"""cape_map_union_cut: the polygon half of the map update on the device where the detection covers a part of a hole of the map plane --
the pieces of (hole minus detection) from a second arrangement inside the pair -- against its host twins cape_host_polygon_union_cut
(one pair through the debug entry) and cape_host_map_union_cut (fed the device's own fusion and measurement rows), bit for bit, against
cape_map_union_holes on every pair that call serves, and against the whole host update.

Every test prints its figures before it asserts (`pytest -s`)."""
import numpy as np
import pytest

from map_union_cut_cases import CUT_HOLES, DEVICE_CAPACITY, PIECES
from map_union_hole_cases import CAPACITY, TABLES, holed_star_pairs, tilted_frames
from test_gpu_map_kalman import _tracks, room  # noqa: F401  (the eight room frames after the four calls)
from test_gpu_map_union import _bits, _measurement_rows, _sans_nodes
from test_gpu_map_union_holes import _grown, _holed, _same_polygon

pytestmark = pytest.mark.gpu

FLAG_NAMES = ("SERVED", "UNCHANGED", "DISJOINT", "MAP_HOLES", "NEW_HOLE", "CAPACITY", "AMBIGUOUS", "HOLES", "HOLE_CUT", "HOLE_PIECES")


@pytest.fixture(scope="module")
def ex1():
    from cape_amd import Extractor, synth

    ex = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)
    yield ex
    ex.close()


def _one_pair(ca, ex, name, rings_a, b, frames, counts, device_capacity=False):
    """the debug entry against its twin: the row without n_nodes and the rings row byte for byte, every ring bit for bit, in order.
    device_capacity: a row named for a capacity of the second arrangement, which the twin -- the host class -- does not have."""
    row, rr, poly = ex.debug_polygon_union_cut(rings_a, b, frames)
    trow, trr, tpoly = ca.host_polygon_union_cut(rings_a, b, frames)
    for bit in range(len(FLAG_NAMES)):
        counts[bit] += bool(row["flags"] & (1 << bit))
    if device_capacity:
        assert row["flags"] == ca.UNION_HOST_CAPACITY and trow["flags"] & ca.UNION_SERVED and trow["flags"] & ca.UNION_HOLE_PIECES, name
        assert poly is None and row["vertex_count"] == 0 and row["area"] == 0 and not rr.tobytes().strip(b"\0"), name
        return row, rr, poly
    assert _sans_nodes(row).tobytes() == trow.tobytes(), f"{name}: {row} != {trow}"
    assert rr.tobytes() == trr.tobytes(), f"{name}: {rr} != {trr}"
    assert _same_polygon(poly, tpoly), f"{name}: rings"
    if row["flags"] & ca.UNION_SERVED:
        assert 3 <= row["n_nodes"] <= ca.MAP_UNION_MAX_NODES, name  # the first arrangement's
    return row, rr, poly


# ---- 1. the debug entry against its twin on the table ----------------------------------------------------------------------------
def test_debug_entry_equals_the_twin_on_the_table(ex1, host_binaries):
    import cape_amd as ca

    counts = [0] * len(FLAG_NAMES)
    canonical = 0
    print()
    for name, rings_a, b, outcome in CUT_HOLES:
        handed = name in DEVICE_CAPACITY
        row, rr, poly = _one_pair(ca, ex1, name, rings_a, b, None, counts, handed)
        print(f"{name:58s} flags {int(row['flags']):#05x} rings {rr['vertex_count'][: rr['ring_count']].tolist()} new/kept/covered "
              f"{int(rr['holes_new'])}/{int(rr['holes_kept'])}/{int(rr['holes_covered'])} n_nodes {int(row['n_nodes'])}")
        if outcome == CAPACITY or handed:
            assert row["flags"] == ca.UNION_HOST_CAPACITY, name
        else:
            assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == outcome, name
            assert bool(row["flags"] & ca.UNION_HOLE_PIECES) == (name in PIECES), name
        canonical += bool(row["flags"] & ca.UNION_HOLE_PIECES)
        # (in the tilted frames the projected coordinates decide the two sliver rows anew: the twin, bit for bit, is the whole check)
        _one_pair(ca, ex1, name + " (tilted)", rings_a, b, tilted_frames(), counts, handed)
    print(f"the table, canonical and tilted frames: pairs per flag bit {dict(zip(FLAG_NAMES, counts))}")
    assert counts[3] == counts[4] == counts[6] == counts[8] == 0 and canonical == len(PIECES) - len(DEVICE_CAPACITY) and counts[9] > canonical


def test_the_tables_of_the_holes_mode_keep_their_rows(ex1, host_binaries):
    """every pair of the holes mode's tables through both debug entries: where the holes entry serves or refuses for a capacity, the cut
    entry gives the same row, rings row and rings; its partly covered pairs (one row in the canonical frame, four more in the tilted
    frames, where the projected coordinates decide the touching and the exactly-covered holes anew: 5, as measured for the holes mode)
    are served with their pieces, as the twin has them"""
    import cape_amd as ca

    counts = [0] * len(FLAG_NAMES)
    cut = 0
    for name, rings_a, b, _ in TABLES:
        for frames in (None, tilted_frames()):
            old = ex1.debug_polygon_union(rings_a, b, frames)
            new = _one_pair(ca, ex1, name, rings_a, b, frames, counts)
            if old[0]["flags"] == ca.UNION_HOST_HOLE_CUT:
                assert new[0]["flags"] & ca.UNION_HOLE_PIECES, name
                cut += 1
            else:
                assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes() and _same_polygon(old[2], new[2]), name
    print(f"\nthe holes mode's tables, both frames: {cut} partly covered pairs now served; pairs per flag bit {dict(zip(FLAG_NAMES, counts))}")
    assert cut == 5 and counts[8] == 0


def test_a_pair_does_not_depend_on_the_pairs_before_it(ex1):
    """Every pair of the table through the one handle in table order and again in reverse: a row, rings row or ring that differs read
    something an earlier pair left in the carve (the second arrangement reuses the cut lists, the nodes, the adjacency and the walked
    face after the intersection, and keeps its sorted cuts in the intersection's heights)."""
    cases = [(name, rings_a, b, frames) for name, rings_a, b, _ in CUT_HOLES for frames in (None, tilted_frames())]
    forward = [ex1.debug_polygon_union_cut(a, b, frames) for _, a, b, frames in cases]
    backward = [ex1.debug_polygon_union_cut(a, b, frames) for _, a, b, frames in reversed(cases)][::-1]
    differ = [name + (" (tilted)" if frames is not None else "") for (name, _, _, frames), x, y in zip(cases, forward, backward)
              if x[0].tobytes() != y[0].tobytes() or x[1].tobytes() != y[1].tobytes() or not _same_polygon(x[2], y[2])]
    print(f"\n{len(cases)} pairs in table order and in reverse: {len(differ)} differ {differ}")
    assert not differ


# ---- 2. the star sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 24])
def test_debug_entry_equals_the_twin_on_star_sets_with_a_hole(ex1, host_binaries, n):
    import cape_amd as ca

    counts = [0] * len(FLAG_NAMES)
    was_cut = now = 0
    for k, (rings_a, b) in enumerate(holed_star_pairs(n)):
        row, rr, _ = _one_pair(ca, ex1, f"star pair {k}", rings_a, b, None, counts)
        old, _, _ = ex1.debug_polygon_union(rings_a, b)
        handed = bool(old["flags"] & ca.UNION_HOST_HOLE_CUT)
        assert handed == bool(row["flags"] & ca.UNION_HOLE_PIECES or row["flags"] == ca.UNION_HOST_CAPACITY), f"star pair {k}"
        was_cut += handed
        now += bool(row["flags"] & ca.UNION_HOLE_PIECES)
    print(f"\n{n}-vertex stars with a hole: {was_cut} partly covered, {now} of them served with pieces; pairs per flag bit "
          f"{dict(zip(FLAG_NAMES, counts))}")
    assert (was_cut, now) == {8: (11, 11), 24: (17, 17)}[n] and counts[5] == counts[6] == counts[8] == 0


# ---- 3. the frames kernel ---------------------------------------------------------------------------------------------------------
def _frames_against_the_twin(ca, ex, n, arrays, match, fusion, meas):
    """every frame of the last map_union_cut against cape_host_map_union_cut on the device's own rows"""
    out = ex.map_union_polygons(n)
    for f in range(n):
        rows, ring_rows, polys = out[f]
        n_cur = len(meas[f])
        mrows, worlds = _measurement_rows(ca, meas[f])
        trows, trings, tpolys = ca.host_map_union_cut(arrays, match[f], fusion[f, :n_cur], mrows, worlds)
        assert not rows[n_cur:].view(np.uint8).any() and not ring_rows[n_cur:].view(np.uint8).any(), f"frame {f}: rows beyond n_cur"
        for i in range(n_cur):
            assert _sans_nodes(rows[i]).tobytes() == trows[i].tobytes(), f"frame {f}, kept plane {i}: {rows[i]} != {trows[i]}"
            assert ring_rows[i].tobytes() == trings[i].tobytes(), f"frame {f}, kept plane {i}: {ring_rows[i]} != {trings[i]}"
            assert _same_polygon(polys[i], tpolys[i]), f"frame {f}, kept plane {i}: rings"
    return out


def _same_frames(a, b, keep=None):
    """two results of map_union_polygons agree on every row: rows, rings rows, vertices.  With `keep`, on the rows it selects, and up to
    the place in the frame's slab: a pair served now that was handed over before moves every polygon behind it."""
    for f, ((rows, rings, polys), (rows2, rings2, polys2)) in enumerate(zip(a, b)):
        for i in range(len(rows)):
            if keep is None or keep(rows[i]):
                r, r2 = rows[i].copy(), rows2[i].copy()
                if keep is not None:
                    r["vertex_offset"] = r2["vertex_offset"] = 0
                assert r.tobytes() == r2.tobytes() and rings[i].tobytes() == rings2[i].tobytes(), f"frame {f}, kept plane {i}"
                assert _same_polygon(polys[i], polys2[i]), f"frame {f}, kept plane {i}: rings"


def test_room_frames_against_a_holed_map(room):  # noqa: F811
    """map_union_holes, then map_union_cut, then map_union_holes again on one batch"""
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
        before = ex.map_union_polygons(n)
        ex.map_union_cut(n, st)
        out = _frames_against_the_twin(ca, ex, n, arrays, match, fusion, room.meas)
        # every row the holes call did not hand over for a partly covered hole is the same row
        _same_frames(before, out, keep=lambda r: r["flags"] != ca.UNION_HOST_HOLE_CUT)
        was_cut = pieces = 0
        for f in range(n):
            rows, ring_rows, polys = out[f]
            n_cur = len(room.meas[f])
            det, _ = room.det[f]
            (P, R, V), Tr, _, _ = ca.host_map_update(arrays, room.tracks, match[f], det, room.T[f], room.S[f])
            assert not np.any(rows["flags"] & ca.UNION_HOST_HOLE_CUT)
            for i in range(n_cur):
                if before[f][0][i]["flags"] != ca.UNION_HOST_HOLE_CUT:
                    assert not rows[i]["flags"] & ca.UNION_HOLE_PIECES
                    continue
                was_cut += 1
                assert rows[i]["flags"] & ca.UNION_SERVED and rows[i]["flags"] & ca.UNION_HOLE_PIECES, f"frame {f}, kept plane {i}: {rows[i]['flags']:#x}"
                pieces += 1
                # the whole update: the same polygon, every vertex of every ring
                j = int(rows[i]["map_plane"])
                want = [V[R[P[j]["ring_first"] + k]["vertex_offset"]:][: R[P[j]["ring_first"] + k]["vertex_count"]] for k in range(int(P[j]["ring_count"]))]
                assert not Tr[j]["result"] & ca.MAP_RESULT_OVERFLOW and [len(r) for r in polys[i]] == [len(r) for r in want], f"frame {f}, map plane {j}"
                worst = max(float(np.max(np.abs(a - b))) for a, b in zip(polys[i], want))
                print(f"\nframe {f}, kept plane {i}, map plane {j}: rings {[len(r) for r in want]}, largest absolute vertex difference from the "
                      f"whole update {worst:.3g} mm")
                assert _same_polygon(polys[i], want), f"frame {f}, map plane {j}: the update's polygon differs in a bit (by at most {worst:.3g} mm)"
        print(f"\nroom frames against a map of {len(arrays[0])} planes, {holed} of them with a hole: {was_cut} pairs were HOST_HOLE_CUT, {pieces} of "
              f"them are served with HOLE_PIECES and equal the update")
        assert was_cut == pieces == 1
        ex.map_union_holes(n, st)
        _same_frames(before, ex.map_union_polygons(n))
    finally:  # (the fixture is shared: the tests after this one see its own map again whatever happened here)
        room.restore()


# ---- 4. the chained frame --------------------------------------------------------------------------------------------------------
def test_a_chained_frame_against_the_grown_map_equals_the_twin():
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
    # the planes grown about their vertex mean, the second hole in the rim the detection does not reach whole: most pairs are partly
    # covered holes (test_gpu_map_union_holes.py)
    arrays, holed = _holed(ca, ca.pack_map([_grown(m["plane"]) for m in map_meas]), where=(0.0, 0.75))
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    _, fusion, _ = ex.map_kalman_rows(n)
    _, match, _, _ = ex.map_matches_wide(n)
    ex.map_union_holes(n, st)
    before = ex.map_union_polygons(n)
    ex.map_union_cut(n, st)
    out = _frames_against_the_twin(ca, ex, n, arrays, match, fusion, meas)
    _same_frames(before, out, keep=lambda r: r["flags"] != ca.UNION_HOST_HOLE_CUT)
    rows, ring_rows, polys = out[1]
    n_cur = len(meas[1])
    high = [i for i in range(64, n_cur) if rows[i]["map_plane"] >= 0 and meas[1][i]["segment"] >= 64]
    was_cut = [i for i in high if before[1][0][i]["flags"] == ca.UNION_HOST_HOLE_CUT]
    pieces = [i for i in high if rows[i]["flags"] & ca.UNION_SERVED and rows[i]["flags"] & ca.UNION_HOLE_PIECES]
    flags = sorted({int(rows[i]["flags"]) for i in was_cut})
    print(f"\nchained frame against the grown map, {holed} holed planes: {n_cur} kept planes, {len(high)} pairs with i >= 64 and a ring in the spill "
          f"record, {len(was_cut)} of them were HOST_HOLE_CUT, {len(pieces)} are served with HOLE_PIECES (their flags now: {[hex(v) for v in flags]}); "
          f"the frame's slab holds {int(ring_rows['vertex_count'].sum())} vertices")
    assert len(high) == 52 and len(was_cut) == 51 and len(pieces) >= 1
    assert not np.any(rows["flags"] & ca.UNION_HOST_HOLE_CUT)
    for i in was_cut:
        assert rows[i]["flags"] == ca.UNION_HOST_CAPACITY or rows[i]["flags"] & ca.UNION_HOLE_PIECES, f"kept plane {i}: {rows[i]['flags']:#x}"
    # the served polygons lie back to back in the frame's slab in kept-plane order, the pieces of the upper half among them
    at = 0
    for r, q in zip(rows[:n_cur], ring_rows[:n_cur]):
        if r["flags"] & ca.UNION_SERVED:
            assert r["vertex_offset"] == at
            at += int(q["vertex_count"].sum())
    assert at <= ca.MAP_UNION_FRAME_VERTICES
    ex.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------
def test_a_plain_union_after_the_cut_call_makes_the_rings_table_stale(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    ex.map_union_cut(n, st)
    rows = ex.map_union_rows(n)[0]
    rings = ex.map_union_ring_rows(n)
    now = (rows["flags"] & ca.UNION_SERVED) != 0
    assert now.any() and np.all(rings["ring_count"][now] >= 1) and not rings["ring_count"][~now].any()
    ex.map_union_holes(n, st)  # (no map plane of the fixture's own map has a hole: the two calls agree on every row)
    assert ex.map_union_rows(n)[0].tobytes() == rows.tobytes() and ex.map_union_ring_rows(n).tobytes() == rings.tobytes()
    ex.map_union_cut(n, st)
    ex.map_union(n, st)
    with pytest.raises(ca.CapeError, match=r"cape_copy_map_union_rings failed \(-4\)"):
        ex.map_union_ring_rows(1)
    ex.map_union_cut(n, st)
    assert ex.map_union_ring_rows(n).tobytes() == rings.tobytes()
    with pytest.raises(ca.CapeError, match=r"cape_map_union_cut failed \(-4\)"):
        ex.map_union_cut(n + 1, st)  # more frames than the Kalman call covered


def test_a_frame_the_wide_match_flags_writes_zeros():
    """[room, a wall of more boundary candidates than the device hull takes, room]: the wide match flags the middle frame
    CAPE_MATCH_EXACT_OVERFLOW, and the cut call reports nothing for it -- rows and rings rows of zeros -- while its neighbours have pairs"""
    import cape_amd as ca
    from cape_amd import synth
    from test_gpu_map_match import _w2c
    from test_gpu_map_measure import _pose_covariances
    from test_gpu_match_map_wide import _extract
    from test_gpu_match_wide import _perforated_wall
    from test_map_update_host import _pose

    Wd, Ht = 1280, 960
    intr = {k: v * 2.0 for k, v in synth.DEFAULT_INTRINSICS.items()}
    rooms = [synth.room(seed=1, frame=f, width=Wd, height=Ht, intr=intr) for f in (0, 3)]
    ex, st = _extract(np.stack([rooms[0], _perforated_wall(Wd, Ht, intr), rooms[1]]), Wd, Ht, intr)
    n = 3
    rng = np.random.default_rng(5)
    T, S = np.stack([_pose(rng) for _ in range(n)]), _pose_covariances(rng, n)
    W2C = np.stack([_w2c(T[f][:3, :3], T[f][:3, 3]) for f in range(n)])
    ex.map_measure(n, T, S, st)
    map_meas = [m for m in ex.map_measurements(n)[0] if m["flags"] & ca.MEASURE_STAGEABLE]
    assert len(map_meas) >= 2
    arrays, holed = _holed(ca, ca.pack_map([_grown(m["plane"]) for m in map_meas]), where=(0.0, 0.75))
    ex.upload_map(arrays)
    ex.upload_tracks(_tracks(map_meas))
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    fr = ex.map_matches_wide(n)[0]
    out = ex.map_union_polygons(n)
    meas = ex.map_measurements(n)
    pairs = [int((out[f][0][: len(meas[f])]["map_plane"] >= 0).sum()) for f in (0, 2)]
    print(f"\nmatch flags per frame {[int(v) for v in fr['flags']]}, {holed} holed map planes, pairs of frames 0 and 2 {pairs}, flags of frame 0 "
          f"{sorted({hex(int(v)) for v in out[0][0]['flags'][: len(meas[0])][out[0][0]['map_plane'][: len(meas[0])] >= 0]})}")
    assert [int(v) for v in fr["flags"]] == [0, ca.MATCH_EXACT_OVERFLOW, 0]
    assert not out[1][0].view(np.uint8).any() and not out[1][1].view(np.uint8).any() and all(p is None for p in out[1][2])
    assert (out[0][0]["flags"] & ca.UNION_SERVED).any()
    ex.close()
