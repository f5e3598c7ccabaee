"""cape_map_union: the polygon half of the map update on the device -- per matched pair Polygon::project, merge_union and simplify for a
map plane without holes whose union creates no hole -- against its host twins cape_host_ring_union (one pair through the debug entry)
and cape_host_map_union (fed the device's own fusion and measurement rows), bit for bit, and against the whole host update.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_map_kalman import _tracks, room  # noqa: F401  (the eight room frames after the four calls)
from test_map_union_host import ALL_PAIRS, CAPACITY, DEVICE_CAPACITY, HAND_BUILT, LONG_NODES, LONG_PAIRS, SERVED, classify, star_pairs

pytestmark = pytest.mark.gpu

W = 128


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _sans_nodes(rows):
    """the rows without the diagnostic the twin cannot know"""
    r = np.atleast_1d(rows).copy()  # (np.array(<structured scalar>, copy=True) still shares the scalar's memory)
    r["n_nodes"] = 0
    return r


def _device_only(ca, flags):
    return bool(flags & (ca.UNION_HOST_CAPACITY | ca.UNION_HOST_AMBIGUOUS))


def _measurement_rows(ca, meas_f):
    """a frame's measurement dicts (Extractor.map_measurements) as the rows and world rings the twin takes"""
    rows = np.zeros(len(meas_f), ca.PLANE_MEASUREMENT_DTYPE)
    rings = []
    for r, m in zip(rows, meas_f):
        _, _, x, y, c, ring, _ = m["plane"]
        r["normal"], r["d"], r["covariance"], r["flags"] = m["normal"], m["d"], m["covariance"], m["flags"]
        r["x_axis"], r["y_axis"], r["center"], r["vertex_count"] = x, y, c, len(ring)
        rings.append(ring)
    return rows, rings


def _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, meas):
    """every frame of the last map_union against cape_host_map_union on the device's own rows; returns (rows, rings) per frame"""
    out = ex.map_unions(n)
    for f in range(n):
        rows, rings = out[f]
        n_cur = len(meas[f])
        mrows, worlds = _measurement_rows(ca, meas[f])
        trows, trings = ca.host_map_union(arrays, match[f], fusion[f, :n_cur], mrows, worlds)
        assert not rows[n_cur:].view(np.uint8).any(), f"frame {f}: rows beyond n_cur"
        for i in range(n_cur):
            assert _sans_nodes(rows[i]).tobytes() == trows[i].tobytes(), f"frame {f}, kept plane {i}: {rows[i]} != {trows[i]}"
            if rows[i]["flags"] & ca.UNION_SERVED:
                assert np.array_equal(_bits(rings[i]), _bits(trings[i])), f"frame {f}, kept plane {i}: ring"
                assert 3 <= rows[i]["n_nodes"] <= ca.MAP_UNION_MAX_NODES
            else:
                assert rings[i] is None
    return out


# ---- 1. the debug entry against its twin -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ex1():
    from cape_amd import Extractor, synth

    ex = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)
    yield ex
    ex.close()


def _one_pair(ca, ex, name, a, b, frames, counts, allow_device_only=False):
    row, ring = ex.debug_ring_union(a, b, frames)
    trow, tring = ca.host_ring_union(a, b, frames)
    for bit in range(7):
        counts[bit] += bool(row["flags"] & (1 << bit))
    if _device_only(ca, int(row["flags"])) and not _device_only(ca, int(trow["flags"])):
        assert allow_device_only, f"{name}: the device hands the pair to the host ({row['flags']:#x}), the twin serves it ({trow['flags']:#x})"
        assert row["vertex_count"] == 0 and row["area"] == 0
        return row
    assert _sans_nodes(row).tobytes() == trow.tobytes(), f"{name}: {row} != {trow}"
    assert np.array_equal(_bits(ring), _bits(tring)), f"{name}: ring"
    return row


def _tilted_frames(rng):
    from test_map_update_host import _rot

    F = []
    for _ in range(3):
        R = _rot(rng, 0.05)
        F += [R[:, 0], R[:, 1], rng.uniform(-20, 20, 3)]
    return np.concatenate(F)


def test_debug_entry_equals_the_twin_on_hand_built_pairs(ex1, host_binaries):
    import cape_amd as ca

    counts = [0] * 7
    for name, a, b, cls, count in HAND_BUILT:
        row = _one_pair(ca, ex1, name, a, b, None, counts, allow_device_only=(name == "crossed combs"))
        assert classify(ca, int(row["flags"])) == (CAPACITY if name in DEVICE_CAPACITY else cls), name
        if count is not None:
            assert row["vertex_count"] == count, name
        if cls == CAPACITY or name in DEVICE_CAPACITY:
            assert row["flags"] == ca.UNION_HOST_CAPACITY, name
    rng = np.random.default_rng(5)
    for name, a, b, cls, _ in HAND_BUILT:
        _one_pair(ca, ex1, name + " (tilted)", a, b, _tilted_frames(rng), counts, allow_device_only=(name == "crossed combs"))
    print(f"\nhand-built pairs, canonical and tilted frames: pairs per flag bit {counts}")


def test_debug_entry_equals_the_twin_on_long_pairs(ex1, host_binaries):
    """Operands of more than 64 vertices (LONG_PAIRS of tests/test_map_union_host.py, and the two 128-gons): every lane loop of the wave
    runs more than one 64-wide chunk.  Rows and rings are the twin's bit for bit in canonical and in tilted frames; in canonical frames
    the class and the vertex count are the table's and n_nodes of a served pair is the one-lane port's
    (tests/host/map_union_algebra.cpp).  Only the pairs of DEVICE_CAPACITY may be the device's alone, as CAPE_UNION_HOST_CAPACITY and
    nothing else -- in canonical frames they must be; HOST_AMBIGUOUS nowhere."""
    import cape_amd as ca

    pairs = [c for c in HAND_BUILT if c[0] == "two 128-gons"] + LONG_PAIRS
    counts = [0] * 7
    rng = np.random.default_rng(9)
    print()
    for name, a, b, cls, count in pairs:
        alone = name in DEVICE_CAPACITY
        for where, frames in (("canonical", None), ("tilted", _tilted_frames(rng))):
            row, _ = ex1.debug_ring_union(a, b, frames)
            trow, _ = ca.host_ring_union(a, b, frames)
            device_only = _device_only(ca, int(row["flags"])) and not _device_only(ca, int(trow["flags"]))
            print(f"{name:26s} {where:9s} flags {int(row['flags']):#04x} (twin {int(trow['flags']):#04x})  vertices {int(row['vertex_count']):3d}  "
                  f"n_nodes {int(row['n_nodes']):3d}" + (f" (port {LONG_NODES[name]:3d})" if frames is None else "")
                  + ("  the device's alone" if device_only else ""))
            row = _one_pair(ca, ex1, f"{name} ({where})", a, b, frames, counts, allow_device_only=alone)
            assert not row["flags"] & ca.UNION_HOST_AMBIGUOUS, f"{name} ({where})"
            if device_only:
                assert row["flags"] == ca.UNION_HOST_CAPACITY and row["vertex_count"] == 0 and row["area"] == 0, f"{name} ({where})"
            if row["flags"] & ca.UNION_SERVED:
                assert row["n_nodes"] > 64 or name.startswith("pinched"), f"{name} ({where}): node_of never left its first chunk"
            if frames is not None:  # (each operand has a frame of its own: the rings shift against each other, the table does not hold)
                continue
            assert device_only == alone, name
            if alone:
                assert classify(ca, int(trow["flags"])) == cls, f"{name}: the twin"
                continue
            assert classify(ca, int(row["flags"])) == cls, name
            if count is not None:
                assert row["vertex_count"] == count, name
            if cls == SERVED:
                assert row["n_nodes"] == LONG_NODES[name], name
    print(f"long pairs, canonical and tilted frames: pairs per flag bit {counts}")


def test_a_pair_does_not_depend_on_the_pairs_before_it(ex1):
    """Every pair of the tables through the one handle in table order and again in reverse: a row or ring that differs read something
    an earlier pair left in the carve (the sorted cuts alias the walked rings; keep, seen and deg are written on demand)."""
    rng = np.random.default_rng(10)
    cases = [(name, a, b, frames) for name, a, b, _, _ in ALL_PAIRS for frames in (None, _tilted_frames(rng))]
    forward = [ex1.debug_ring_union(a, b, frames) for _, a, b, frames in cases]
    backward = [ex1.debug_ring_union(a, b, frames) for _, a, b, frames in reversed(cases)][::-1]
    differ = [name + (" (tilted)" if frames is not None else "") for (name, _, _, frames), (r0, v0), (r1, v1) in zip(cases, forward, backward)
              if r0.tobytes() != r1.tobytes() or not np.array_equal(_bits(v0), _bits(v1))]
    print(f"\n{len(cases)} pairs in table order and in reverse: {len(differ)} differ {differ}")
    assert not differ


@pytest.mark.parametrize("n", [8, 24])
def test_debug_entry_equals_the_twin_on_star_sets(ex1, host_binaries, n):
    import cape_amd as ca

    counts, nodes = [0] * 7, 0
    rng = np.random.default_rng(7)
    for k, (a, b) in enumerate(star_pairs(n)):
        row = _one_pair(ca, ex1, f"star pair {k}", a, b, None, counts)
        assert not _device_only(ca, int(row["flags"])), f"star pair {k}: {row['flags']:#x}"
        nodes = max(nodes, int(row["n_nodes"]))
        _one_pair(ca, ex1, f"star pair {k} (tilted)", a, b, _tilted_frames(rng), [0] * 7)
    print(f"\n{n}-vertex stars: pairs per flag bit {counts}, largest n_nodes {nodes}")
    assert counts[4] <= 10 and counts[5] == 0 and counts[6] == 0  # at most 5 % make a hole; none is the device's alone


# ---- 2. eight room frames ------------------------------------------------------------------------------------------------------
def _union(room):  # noqa: F811
    room.ex.map_union(room.n, room.st)
    return room.ex.map_unions(room.n)


def test_room_frames_equal_the_twin(room):  # noqa: F811
    import cape_amd as ca

    room.ex.map_union(room.n, room.st)
    _, match, _ = room.matches
    out = _compare_frames_with_twin(ca, room.ex, room.n, room.arrays, match, room.rows, room.meas)
    counts = [0] * 7
    updated = (room.results["result"] & ca.MAP_RESULT_UPDATED) != 0
    for f in range(room.n):
        rows, _ = out[f]
        n_cur = len(room.meas[f])
        pairs = rows[:n_cur][rows[:n_cur]["map_plane"] >= 0]
        assert len(pairs) == int(updated[f].sum()), f"frame {f}: the pairs are the UPDATED ones"
        assert sorted(pairs["map_plane"].tolist()) == np.flatnonzero(updated[f]).tolist()
        for bit in range(7):
            counts[bit] += int(np.count_nonzero(pairs["flags"] & (1 << bit)))
        if len(pairs):
            assert np.any(pairs["flags"] & ca.UNION_SERVED), f"frame {f}: no served pair"
        if f == room.source:
            assert np.all(pairs["flags"] & ca.UNION_SERVED), f"frame {f}: the map's own frame"
        # the served rings lie back to back in kept-plane order
        at = 0
        for r in rows[:n_cur]:
            if r["flags"] & ca.UNION_SERVED:
                assert r["vertex_offset"] == at
                at += int(r["vertex_count"])
    print(f"\nroom frames: {int(updated.sum())} pairs over {room.n} frames, pairs per flag bit (SERVED, UNCHANGED, DISJOINT, MAP_HOLES, "
          f"NEW_HOLE, CAPACITY, AMBIGUOUS) {counts}")
    assert counts[6] == 0


# ---- 3. the chained frame ------------------------------------------------------------------------------------------------------
def test_a_chained_frame_is_merged_through_the_kept_plane_table():
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
    arrays, tracks = ca.pack_map([m["plane"] for m in map_meas]), _tracks(map_meas)
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    ex.map_union(n, st)
    _, fusion, _ = ex.map_kalman_rows(n)
    _, match, _, _ = ex.map_matches_wide(n)
    meas = ex.map_measurements(n)
    out = _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, meas)
    rows, _ = out[1]
    high = [i for i in range(64, len(meas[1])) if rows[i]["map_plane"] >= 0 and meas[1][i]["segment"] >= 64]
    served = [i for i in high if rows[i]["flags"] & ca.UNION_SERVED]
    print(f"\nchained frame: {len(meas[1])} kept planes, {int((rows['map_plane'][:len(meas[1])] >= 0).sum())} pairs, {len(high)} with i >= 64 "
          f"and a ring in the spill record, {len(served)} of them served")
    assert len(high) >= 1 and len(served) >= 1
    ex.close()


# ---- 4. what the device leaves to the host, per pair ---------------------------------------------------------------------------
def test_map_holes_and_long_rings_are_the_hosts_pair_by_pair(room):  # noqa: F811
    import cape_amd as ca

    base = _union(room)
    P, R, V = room.arrays
    _, match, _ = room.matches
    hit = [j for j in range(len(P)) if (match[:, j] >= 0).any()]
    assert len(hit) >= 2
    j_hole, j_long = hit[0], hit[1]
    planes = []
    for j in range(len(P)):
        r = R[P[j]["ring_first"]]
        outer = V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]].copy()
        holes = []
        if j == j_hole:  # a hole too small to change a match: a 1e-3 mm triangle at the middle of the first edge's inward side
            c = outer.mean(axis=0)
            holes = [c + 1e-3 * np.array([[0, 0], [1, 0], [0, 1.0]])]
        if j == j_long:  # the same outline with 129 vertices: points on its first edge
            t = np.linspace(0, 1, 129 - len(outer) + 2)[1:-1, None]
            outer = np.concatenate([outer[:1], outer[0] + t * (outer[1] - outer[0]), outer[1:]])
            assert len(outer) == 129
        planes.append((P[j]["normal"], float(P[j]["d"]), P[j]["x_axis"], P[j]["y_axis"], P[j]["center"], outer, holes))
    arrays = ca.pack_map(planes)
    ex, n, st = room.ex, room.n, room.st
    ex.upload_map(arrays)
    ex.upload_tracks(room.tracks)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    assert np.array_equal(ex.map_matches_wide(n)[1], match), "the edits changed a match"
    ex.map_union(n, st)
    got = ex.map_unions(n)
    touched = 0
    for f in range(n):
        rows, rings = got[f]
        brows, brings = base[f]
        special = np.isin(brows["map_plane"], [j_hole, j_long]) & (brows["map_plane"] >= 0) & (np.arange(W) < len(room.meas[f]))
        if not special.any():
            assert rows.tobytes() == brows.tobytes(), f"frame {f}: an untouched frame changed"
            assert all((a is None and b is None) or np.array_equal(_bits(a), _bits(b)) for a, b in zip(rings, brings))
            continue
        touched += 1
        for i in range(W):
            if special[i]:
                want = ca.UNION_HOST_MAP_HOLES if brows[i]["map_plane"] == j_hole else ca.UNION_HOST_CAPACITY
                assert rows[i]["flags"] == want and rows[i]["vertex_count"] == 0 and rows[i]["area"] == 0 and rings[i] is None
                assert rows[i]["map_plane"] == brows[i]["map_plane"]
            else:  # the other pairs of the frame: the same ring, further up in the slab
                a, b = np.atleast_1d(rows[i]).copy(), np.atleast_1d(brows[i]).copy()
                a["vertex_offset"] = b["vertex_offset"] = 0
                assert a.tobytes() == b.tobytes(), f"frame {f}, kept plane {i}"
                assert (rings[i] is None and brings[i] is None) or np.array_equal(_bits(rings[i]), _bits(brings[i]))
    print(f"\nmap plane {j_hole} given a hole, map plane {j_long} a ring of 129 vertices: {touched} frames hold a pair of theirs")
    assert touched >= 1
    room.restore()


def test_a_map_ring_of_128_vertices_is_served_by_the_frames_kernel(room):  # noqa: F811
    """CAPE_MAP_UNION_MAX_RING exactly: one matched map plane whose pairs are all served gets the same outline with 128 vertices.  Its
    pairs stay served with the vertex counts they had (simplify drops the added points), every frame is the twin's on the edited map,
    and the other pairs do not move but for their place in the slab.

    The added points lie on a shallow arc, not on the edge itself as in the 129-vertex test above: points interpolated on an edge are
    collinear only up to rounding, and against the plane's own detection, whose edge is that very line, they give an arrangement
    whose neighbours lie some 1e-14 rad apart.  The host class walks its faces by those angles (some of its walks do not close: it
    skips those faces) and still returns the outline; the device hands such a pair to the host, as its guard band of 1e-10 rad demands
    (CAPE_UNION_HOST_CAPACITY for the walk that does not close; measured on the device with this very map plane).  On the arc the
    closest directions are 1e-5 rad apart."""
    import cape_amd as ca

    base = _union(room)
    P, R, V = room.arrays
    _, match, _ = room.matches

    def pairs_of(j, got):
        return [(f, i) for f in range(room.n) for i in range(len(room.meas[f])) if got[f][0][i]["map_plane"] == j]

    j_long = next(j for j in range(len(P)) if pairs_of(j, base) and all(base[f][0][i]["flags"] & ca.UNION_SERVED for f, i in pairs_of(j, base)))
    planes = []
    for j in range(len(P)):
        r = R[P[j]["ring_first"]]
        outer = V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]].copy()
        if j == j_long:  # the same outline with 128 vertices: points along its first edge, on an arc that bulges outwards by 0.01 mm
            t = np.linspace(0, 1, W - len(outer) + 2)[1:-1, None]
            x, y = outer[:, 0], outer[:, 1]
            turn = np.sign(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))
            d = outer[1] - outer[0]
            out = turn * np.array([d[1], -d[0]]) / np.hypot(*d)
            outer = np.concatenate([outer[:1], outer[0] + t * d + 0.04 * t * (1 - t) * out, outer[1:]])
            assert len(outer) == W == ca.MAP_UNION_MAX_RING
        planes.append((P[j]["normal"], float(P[j]["d"]), P[j]["x_axis"], P[j]["y_axis"], P[j]["center"], outer, []))
    arrays = ca.pack_map(planes)
    ex, n, st = room.ex, room.n, room.st
    ex.upload_map(arrays)
    ex.upload_tracks(room.tracks)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    assert np.array_equal(ex.map_matches_wide(n)[1], match), "the edit changed a match"
    _, fusion, _ = ex.map_kalman_rows(n)
    ex.map_union(n, st)
    got = _compare_frames_with_twin(ca, ex, n, arrays, match, fusion, room.meas)
    long_pairs = pairs_of(j_long, got)
    print(f"\nmap plane {j_long} given a ring of {W} vertices: its pairs (frame, kept plane, flags, vertices, n_nodes; vertices before) "
          f"{[(f, i, int(got[f][0][i]['flags']), int(got[f][0][i]['vertex_count']), int(got[f][0][i]['n_nodes']), int(base[f][0][i]['vertex_count'])) for f, i in long_pairs]}")
    assert long_pairs == pairs_of(j_long, base) and len(long_pairs) >= 1
    for f in range(n):
        rows, rings = got[f]
        brows, brings = base[f]
        for i in range(W):
            if (f, i) in long_pairs:
                assert rows[i]["flags"] & ca.UNION_SERVED and rows[i]["flags"] == brows[i]["flags"], f"frame {f}, kept plane {i}"
                assert rows[i]["vertex_count"] == brows[i]["vertex_count"], f"frame {f}, kept plane {i}"
                assert rows[i]["n_nodes"] >= W, f"frame {f}, kept plane {i}: every vertex of the long ring is a node"
            else:  # the other pairs: the same row and ring, wherever the slab has them
                a, b = np.atleast_1d(rows[i]).copy(), np.atleast_1d(brows[i]).copy()
                a["vertex_offset"] = b["vertex_offset"] = 0
                assert a.tobytes() == b.tobytes(), f"frame {f}, kept plane {i}"
                assert (rings[i] is None and brings[i] is None) or np.array_equal(_bits(rings[i]), _bits(brings[i]))
    room.restore()


# ---- 5. against the whole host update --------------------------------------------------------------------------------------------
def test_against_the_whole_host_update(room):  # noqa: F811
    """The device's rings come from the device's fusion frames and world rings, the update's from the host's own covariances (pow):
    the vertex counts must agree, the largest absolute vertex difference is printed (no bound is fixed for it)."""
    import cape_amd as ca

    out = _union(room)
    _, match, _ = room.matches
    worst, served = 0.0, 0
    for f in range(room.n):
        det, _ = room.det[f]
        (P, R, V), Tr, _, _ = ca.host_map_update(room.arrays, room.tracks, match[f], det, room.T[f], room.S[f])
        rows, rings = out[f]
        for i in range(len(room.meas[f])):
            j = int(rows[i]["map_plane"])
            if j < 0 or not rows[i]["flags"] & ca.UNION_SERVED:
                continue
            r = R[P[j]["ring_first"]]
            outer = V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]]
            assert P[j]["ring_count"] == 1 and not Tr[j]["result"] & ca.MAP_RESULT_OVERFLOW, f"frame {f}, map plane {j}"
            assert len(outer) == rows[i]["vertex_count"], f"frame {f}, map plane {j}: {rows[i]['vertex_count']} vertices, the update has {len(outer)}"
            worst = max(worst, float(np.max(np.abs(outer - rings[i]))))
            served += 1
    print(f"\nagainst cape_host_map_update: {served} served pairs, largest absolute vertex difference {worst:.3g} mm")
    assert served >= len(room.arrays[0])


# ---- 6. bookkeeping ------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    CAP = r"failed \(-4\)"

    def state():
        rows, ver = ex.measurement_rows(n)
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in (*ex.map_matches_wide(n), rows, ver, *ex.map_kalman_rows(n))]

    room.restore()
    before = state()
    # CAPE_ERR_CAPACITY: the Kalman results were replaced since the last union (room.restore ran cape_map_kalman)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    rows_p = C.c_void_p()
    assert ex.L.cape_device_map_union(ex.h, C.byref(rows_p), None) == -4
    ex.map_union(n, st)
    first = ex.map_union_rows(n)
    ex.map_union(n, st)
    second = ex.map_union_rows(n)
    after = state()
    assert first[0].tobytes() == second[0].tobytes()
    for f in range(n):  # (the slab beyond a frame's rings is not written)
        used = int(first[0][f]["vertex_count"].sum())
        assert np.array_equal(_bits(first[1][f, :used]), _bits(second[1][f, :used]))
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "map_union wrote into a match, measurement or fusion buffer (the map and the tracks: below)"
    # (the map and the tracks cannot be read back: a match and a Kalman call after the unions, without another upload, still see the
    #  same state)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    for a, b in zip(ex.map_matches_wide(n), (None,) + room.matches[1:2] + (None,) + room.matches[2:3]):
        assert b is None or np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), \
            "map_union wrote into the map"
    for a, b in zip(ex.map_kalman_rows(n), (room.frames, room.rows, room.results)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "map_union wrote into the map or the tracks"
    ex.map_union(n, st)
    assert ex.L.cape_device_map_union(ex.h, C.byref(rows_p), None) == 0 and rows_p.value
    # fewer frames may be copied, more may not
    ex.map_union(4, st)
    assert ex.map_union_rows(4)[0].tobytes() == first[0][:4].tobytes()
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(5)
    # more frames than the Kalman call covered
    ex.map_kalman(4, st)
    with pytest.raises(ca.CapeError, match="cape_map_union " + CAP):
        ex.map_union(5, st)
    ex.map_union(4, st)
    # every call that invalidates the Kalman results invalidates these
    ex.map_measure(n, room.T, room.S, st)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    with pytest.raises(ca.CapeError, match="cape_map_union " + CAP):
        ex.map_union(1, st)
    room.restore()
    ex.map_union(n, st)
    ex.upload_map(room.arrays)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    with pytest.raises(ca.CapeError, match="cape_map_union " + CAP):
        ex.map_union(n, st)  # no Kalman call on the new map
    # an empty map succeeds: no pair anywhere
    ex.upload_map(ca.pack_map([]))
    ex.upload_tracks(np.zeros(0, ca.MAP_TRACK_DTYPE))
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union(n, st)
    rows, _ = ex.map_union_rows(n)
    for f in range(n):
        k = len(room.meas[f])
        assert np.all(rows[f, :k]["map_plane"] == -1) and not rows[f, :k]["flags"].any() and not rows[f, k:].view(np.uint8).any()
    room.restore()
    ex.map_union(n, st)
    assert ex.map_union_rows(n)[0].tobytes() == first[0].tobytes()
