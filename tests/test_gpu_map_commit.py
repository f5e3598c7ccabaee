"""cape_map_commit, cape_map_info and cape_map_download: a frame's update written into the device map and read back -- against the host
twin cape_host_map_commit fed the device's own rows, byte for byte (the commit has no arithmetic: planes, rings, vertices, tracks and
the result header are compared with tobytes()), and, over a loop of eight commits, against the pure host route.

Every test prints its figures before it asserts (`pytest -s`)."""
import numpy as np
import pytest

import capacity_cases as K
from test_gpu_map_kalman import _tracks, room  # noqa: F401  (the eight room frames after the four calls)
from test_gpu_map_union import _measurement_rows
from test_gpu_map_union_holes import _holed

pytestmark = pytest.mark.gpu

W = 128
CAP = r"failed \(-4\)"


def _same_map(got, want, what):
    (P, R, V), Tr = got
    (P2, R2, V2), Tr2 = want
    for name, a, b in (("planes", P, P2), ("rings", R, R2), ("vertices", V, V2), ("tracks", Tr, Tr2)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what}: {name}"


def _twin_inputs(ca, ex, n, f, meas_f, with_rings=True):
    """frame f of the device's own results as cape_host_map_commit takes them"""
    frames, rows, results = ex.map_kalman_rows(n)
    mrows, worlds = _measurement_rows(ca, meas_f)
    for r, m in zip(mrows, meas_f):
        r["staged_normal"] = m["staged_normal"]
    urows, ver = ex.map_union_rows(n)
    rrows = ex.map_union_ring_rows(n)[f] if with_rings else None
    return frames[f], results[f], rows[f], mrows, worlds, urows[f], rrows, ver[f]


def _commit_both(ca, ex, st, n, f, meas_f, flags, next_id, with_rings=True, what=""):
    """the commit of frame f on the device and through the twin on the downloaded map: header, map and tracks byte for byte -- the old
    map's where the frame is refused.  Returns (result, next_id, the map and tracks after, those before)."""
    before = ex.download_map()
    inputs = _twin_inputs(ca, ex, n, f, meas_f, with_rings)
    new, Tr, want, want_id = ca.host_map_commit(before[0], before[1], *inputs, flags, next_id, frame=f)
    result, nid = ex.map_commit(f, flags, next_id, st)
    after = ex.download_map()
    print(f"{what}frame {f}: flags {int(result['flags']):#x}, {int(result['n_planes'])} planes, {int(result['n_rings'])} rings, "
          f"{int(result['n_vertices'])} vertices, updated {int(result['n_updated'])}, appended {int(result['n_appended'])}, host pairs "
          f"{int(result['n_host_pairs'])}, fail polygon {int(result['n_fail_polygon'])}, next id {int(result['next_id'])}")
    assert result.tobytes() == want.tobytes(), f"{what}frame {f}: header {result} != {want}"
    assert nid == want_id
    assert ex.map_info() == (int(result["n_planes"]), int(result["n_rings"]), int(result["n_vertices"]))
    if result["flags"] & ca.COMMIT_DONE:
        _same_map(after, (new, Tr), f"{what}frame {f}")
    else:
        _same_map(after, before, f"{what}frame {f} (refused)")
    return result, nid, after, before


def _signed(ring):
    x, y = ring[:, 0], ring[:, 1]
    return 0.5 * float(np.sum(np.roll(x, 1) * y - x * np.roll(y, 1)))


def _rings_of(arrays, j):
    P, R, V = arrays
    return [V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]] for r in R[P[j]["ring_first"]: P[j]["ring_first"] + P[j]["ring_count"]]]


def _rebuilt(ca, arrays, flip=lambda j, k: False, oriented=False):
    """the map plane by plane: every ring reversed where `flip` says, or as the host class holds it (outer ring clockwise, holes
    counter-clockwise)"""
    P = arrays[0]
    planes = []
    for j in range(len(P)):
        rings = []
        for k, ring in enumerate(_rings_of(arrays, j)):
            turn = ((_signed(ring) > 0) if k == 0 else (_signed(ring) < 0)) if oriented else flip(j, k)
            rings.append(ring[::-1].copy() if turn else ring.copy())
        planes.append((P[j]["normal"], float(P[j]["d"]), P[j]["x_axis"], P[j]["y_axis"], P[j]["center"], rings[0], rings[1:]))
    return ca.pack_map(planes)


# ---- 1. upload, then download ---------------------------------------------------------------------------------------------------
def test_the_download_is_the_reoriented_upload(room):  # noqa: F811
    import cape_amd as ca

    ex = room.ex
    holed, count = _holed(ca, room.arrays)
    assert count >= 2
    mixed = _rebuilt(ca, holed, flip=lambda j, k: (j + k) % 2 == 0)  # every other ring the other way round
    ex.upload_map(mixed)
    want = _rebuilt(ca, mixed, oriented=True)
    assert want[2].tobytes() != mixed[2].tobytes()
    got, tracks = ex.download_map()
    print(f"\nmap of {len(want[0])} planes, {len(want[1])} rings, {len(want[2])} vertices: uploaded with mixed orientations, downloaded")
    _same_map((got, tracks), (want, np.zeros(len(want[0]), ca.MAP_TRACK_DTYPE)), "before upload_tracks")
    assert ex.map_info() == (len(want[0]), len(want[1]), len(want[2]))
    sent = room.tracks.copy()
    sent["result"] = np.arange(len(sent)) + 7
    sent["id"] = (np.arange(len(sent), dtype=np.uint64) << np.uint64(33)) + np.uint64(5)
    ex.upload_tracks(sent)
    _same_map(ex.download_map(), (want, sent), "after upload_tracks")
    ex.upload_map(want)  # a new map discards the tracks
    _same_map(ex.download_map(), (want, np.zeros(len(want[0]), ca.MAP_TRACK_DTYPE)), "after another upload_map")
    # arrays that are too small
    n, r, v = ex.map_info()
    P, R, V = np.zeros(n, ca.MAP_PLANE_DTYPE), np.zeros(r, ca.MAP_RING_DTYPE), np.zeros((v, 2))
    for caps in ((n - 1, r, v), (n, r - 1, v), (n, r, v - 1)):
        assert ex.L.cape_map_download(ex.h, P.ctypes.data, caps[0], R.ctypes.data, caps[1], V.ctypes.data, caps[2], None) == ca.CAPE_ERR_CAPACITY
    assert ex.L.cape_map_download(ex.h, P.ctypes.data, n, R.ctypes.data, r, V.ctypes.data, v, None) == 0
    ex.upload_map(ca.pack_map([]))
    assert ex.map_info() == (0, 0, 0) and len(ex.download_map()[1]) == 0
    room.restore()


# ---- 2. each room frame ---------------------------------------------------------------------------------------------------------
def test_each_room_frame_commits_like_the_twin(room):  # noqa: F811
    """restore, cape_map_union_cut, commit(f, ADD_STAGED) per frame.  Every frame is DONE with the fixture's own seed (room stream, seed
    11): none had to be chosen for it."""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    print()
    appended = updated = 0
    for f in range(n):
        room.restore()
        ex.map_union_cut(n, st)
        result, nid, after, before = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, 1000 + f)
        assert result["flags"] == ca.COMMIT_DONE, f"frame {f} is refused"
        assert nid == 1000 + f + result["n_appended"] and result["n_updated"] == room.frames[f]["n_updated"]
        assert after[1]["id"][len(before[0][0]):].tolist() == list(range(1000 + f, nid))
        appended += int(result["n_appended"])
        updated += int(result["n_updated"])
    print(f"eight room frames, each against the map of {len(room.arrays[0])} planes: {updated} planes updated, {appended} appended")
    assert updated >= len(room.arrays[0]) and appended >= 1
    room.restore()


def test_the_frame_is_the_union_rows_where_the_map_polygon_kept_its_own(room):  # noqa: F811
    """Polygon::project returns the map polygon itself where its frame is the target within 1e-12 (isApprox): the union row then carries
    the map polygon's OWN frame, not the fusion row's, and so must the committed plane.  Every map plane that a pair of the frame
    updates is re-expressed here in its fusion frame, a component of each axis and of the centre one ulp off."""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    f = room.source
    P, R, V = (a.copy() for a in room.arrays)
    moved = []
    for j in range(len(P)):
        i = int(room.results[f, j]["kept_plane"])
        if i < 0 or not room.rows[f, i]["flags"] & ca.FUSION_FRAME:
            continue
        F = room.rows[f, i]
        r = R[P[j]["ring_first"]]
        at = slice(int(r["vertex_offset"]), int(r["vertex_offset"]) + int(r["vertex_count"]))
        points = P[j]["center"] + V[at, :1] * P[j]["x_axis"] + V[at, 1:] * P[j]["y_axis"]
        V[at] = np.stack([(points - F["center"]) @ F["x_axis"], (points - F["center"]) @ F["y_axis"]], 1)
        x_axis, y_axis, centre = F["x_axis"].copy(), F["y_axis"].copy(), F["center"].copy()
        for v, k in ((centre, int(np.argmax(np.abs(centre)))), (x_axis, int(np.argmin(np.abs(x_axis)))), (y_axis, int(np.argmin(np.abs(y_axis))))):
            v[k] = np.nextafter(v[k], np.inf)  # (the axes' smallest components: their norms stay 1 within DBL_EPSILON)
        P[j]["x_axis"], P[j]["y_axis"], P[j]["center"] = x_axis, y_axis, centre
        moved.append(j)
    assert moved
    ex.upload_map((P, R, V))
    ex.upload_tracks(room.tracks)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    urows, _ = ex.map_union_rows(n)
    _, fusion, _ = ex.map_kalman_rows(n)
    own = [i for i in range(len(room.meas[f])) if urows[f, i]["flags"] & ca.UNION_SERVED and urows[f, i]["center"].tobytes() != fusion[f, i]["center"].tobytes()]
    print(f"\nmap planes {moved} re-expressed in their fusion frames, one ulp off: {len(own)} served pairs of frame {f} keep the map polygon's own frame")
    assert len(own) >= 1
    result, _, after, _ = _commit_both(ca, ex, st, n, f, room.meas[f], 0, 0)
    assert result["flags"] == ca.COMMIT_DONE
    for i in own:
        plane = after[0][0][int(urows[f, i]["map_plane"])]
        for k in ("x_axis", "y_axis", "center"):
            assert plane[k].tobytes() == urows[f, i][k].tobytes() != fusion[f, i][k].tobytes(), k
    room.restore()


# ---- 3. a holed map through the plain union -------------------------------------------------------------------------------------
def test_a_holed_map_through_the_plain_union_is_refused(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    arrays, holed = _holed(ca, room.arrays)
    ex.upload_map(arrays)
    ex.upload_tracks(room.tracks)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union(n, st)
    f = room.source
    urows, _ = ex.map_union_rows(n)
    _, fusion, _ = ex.map_kalman_rows(n)
    host_bits = ca.UNION_HOST | ca.UNION_HOST_HOLE_CUT
    flagged = int(np.count_nonzero((urows[f]["flags"] & host_bits) != 0))
    assert np.any(urows[f]["flags"] & ca.UNION_HOST_MAP_HOLES)
    state = [a.tobytes() for a in (*ex.map_kalman_rows(n), *ex.map_union_rows(n))]
    print()
    result, nid, _, _ = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, 50, with_rings=False)
    assert result["flags"] == ca.COMMIT_HOST_PAIR and nid == 50
    assert result["n_host_pairs"] == flagged >= 1
    assert all(fusion[f][i]["flags"] & ca.FUSION_STATE for i in np.flatnonzero(urows[f]["flags"] & host_bits))
    # the results are still there, and still the same
    assert [a.tobytes() for a in (*ex.map_kalman_rows(n), *ex.map_union_rows(n))] == state
    # the same frame through the cut mode commits
    ex.map_union_cut(n, st)
    result, _, _, _ = _commit_both(ca, ex, st, n, f, room.meas[f], 0, 50)
    assert result["flags"] == ca.COMMIT_DONE and result["n_updated"] >= 1
    room.restore()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------
def test_a_loop_of_eight_commits_without_an_upload(room):  # noqa: F811
    """For f = 0 .. 7 on the same batch: wide match, Kalman, union_cut, commit(f), no upload in between (the measurements stay valid).
    After every step the download is the twin's on the device's rows.  After the last step the map is compared with the pure host
    route (cape_host_match_map + cape_host_map_update per frame): the counts, ids, counters and result bits must agree; the largest
    parameter and vertex differences are printed (the covariances pass through two different pows; no bound is fixed for them)."""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    next_id = 1000
    print()
    for f in range(n):
        if f:
            ex.match_map_wide(n, room.W2C, None, room.flags, st)
            ex.map_kalman(n, st)
        ex.map_union_cut(n, st)
        result, next_id, device, _ = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, next_id, what="loop, ")
        assert result["flags"] == ca.COMMIT_DONE, f"step {f} is refused"
    (P, R, V), Tr = device
    A, Th, host_id = _rebuilt(ca, room.arrays, oriented=True), room.tracks.copy(), 1000
    for f in range(n):
        det, _ = room.det[f]
        match, _ = ca.host_match_map(A, [d[:7] for d in det], room.W2C[f], None, room.flags)
        A, Th, _, host_id = ca.host_map_update(A, Th, match, det, room.T[f], room.S[f], ca.MAP_ADD_STAGED, host_id)
    HP, HR, HV = A
    print(f"after eight commits: device {len(P)} planes, {len(R)} rings, {len(V)} vertices, next id {next_id}; host route {len(HP)} planes, "
          f"{len(HR)} rings, {len(HV)} vertices, next id {host_id}")
    same_shape = (len(P), len(R), len(V)) == (len(HP), len(HR), len(HV))
    if same_shape:
        params = max(float(np.max(np.abs(P[k] - HP[k]))) for k in ("normal", "d", "x_axis", "y_axis", "center"))
        print(f"largest parameter difference {params:.3g}, largest covariance difference (relative) "
              f"{float(np.max(np.abs(Tr['covariance'] - Th['covariance']) / np.maximum(np.abs(Th['covariance']), 1e-300).max())):.3g}, "
              f"largest vertex difference {float(np.max(np.abs(V - HV))) if len(V) else 0.0:.3g} mm")
    assert same_shape and next_id == host_id
    assert np.array_equal(R["vertex_count"], HR["vertex_count"]) and np.array_equal(P["ring_count"], HP["ring_count"])
    for k in ("id", "successive_matched", "failed_tracking", "result", "flags"):
        assert np.array_equal(Tr[k], Th[k]), k
    room.restore()


# ---- 5. widths ------------------------------------------------------------------------------------------------------------------
def _wall_copies(ca, room, size, rng, far=False):  # noqa: F811
    """a map of `size` planes: the room's own, then copies of them a little off (profiles/map_kalman_rate.py's 1 024-plane map) -- or,
    `far`, ten metres off, where no detection matches any"""
    base = [(P["normal"], float(P["d"]), P["x_axis"], P["y_axis"], P["center"], _rings_of(room.arrays, j)[0], []) for j, P in enumerate(room.arrays[0])]
    planes, covs = ([] if far else list(base[:size])), ([] if far else [t["covariance"] for t in room.tracks[:size]])
    while len(planes) < size:
        at = int(rng.integers(len(base)))
        nw, d, x, y, c, ring, h = base[at]
        planes.append((nw, d + (10000.0 if far else float(rng.uniform(-120, 120))), x, y, c, ring * rng.uniform(0.7, 1.3) + rng.uniform(-200, 200, 2), h))
        covs.append(room.tracks[at]["covariance"])
    tracks = np.zeros(size, ca.MAP_TRACK_DTYPE)
    for j in range(size):
        tracks[j]["covariance"] = covs[j]
        tracks[j]["flags"] = ca.MAP_TRACK_STAGED if j % 2 else 0
        tracks[j]["successive_matched"], tracks[j]["failed_tracking"], tracks[j]["id"] = j % 5, j % 3, 5000 + j
    return ca.pack_map(planes), tracks


def _pipeline(room, arrays, tracks):  # noqa: F811
    ex, n, st = room.ex, room.n, room.st
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)


# the plan kernel decides four map planes per lane (3 / 4 / 5), 256 per wave (255 / 256 / 257, 511 / 513, 767 / 769) and 1 024 per
# workgroup; cape_map_kalman visits the map 64 planes at a time (63 / 64 / 65)
WIDTHS = [3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 767, 769, 1023, 1024]


@pytest.mark.parametrize("size", WIDTHS)
def test_map_widths(room, size):  # noqa: F811
    import cape_amd as ca

    rng = np.random.default_rng(size)
    arrays, tracks = _wall_copies(ca, room, size, rng)
    _pipeline(room, arrays, tracks)
    f = room.source
    flags = ca.COMMIT_ADD_STAGED if size + W <= ca.MAP_MAX_PLANES else 0
    print()
    result, nid, after, _ = _commit_both(ca, room.ex, room.st, room.n, f, room.meas[f], flags, 9000, what=f"{size} planes, ")
    assert result["flags"] == ca.COMMIT_DONE and result["n_updated"] >= 1
    assert after[1]["id"][:size].tolist() == list(range(5000, 5000 + size))
    # ... and the frame that leaves the most planes to append, where there is room for them
    g = max(range(room.n), key=lambda h: sum(bool(m["flags"] & ca.MEASURE_STAGEABLE) for m in room.meas[h]))
    if flags and g != f:
        _pipeline(room, arrays, tracks)
        result, nid, after, _ = _commit_both(ca, room.ex, room.st, room.n, g, room.meas[g], flags, 9000, what=f"{size} planes, ")
        assert result["n_appended"] >= 1
        if result["flags"] & ca.COMMIT_DONE:  # (a copy's pair may be the host's: the twin agreed on the refusal above)
            assert nid == 9000 + result["n_appended"] and after[1]["id"].tolist() == list(range(5000, 5000 + size)) + list(range(9000, nid))
        else:
            assert size > len(room.arrays[0]), "the room's own map serves every pair of this frame"
    if size == WIDTHS[-1]:
        room.restore()


def test_the_capacity_edge(room):  # noqa: F811
    """1024 - k planes that match nothing and the k stageable kept planes of a frame: DONE at exactly 1 024 planes; one map plane more
    and the frame is refused with CAPE_COMMIT_CAPACITY, the map unchanged"""
    import cape_amd as ca

    f = max(range(room.n), key=lambda g: sum(bool(m["flags"] & ca.MEASURE_STAGEABLE) for m in room.meas[g]))
    k = sum(bool(m["flags"] & ca.MEASURE_STAGEABLE) for m in room.meas[f])
    assert k >= 2
    print()
    for size, want in ((ca.MAP_MAX_PLANES - k, ca.COMMIT_DONE), (ca.MAP_MAX_PLANES - k + 1, ca.COMMIT_CAPACITY)):
        arrays, tracks = _wall_copies(ca, room, size, np.random.default_rng(3), far=True)
        _pipeline(room, arrays, tracks)
        result, nid, after, _ = _commit_both(ca, room.ex, room.st, room.n, f, room.meas[f], ca.COMMIT_ADD_STAGED, 70, what=f"{size} planes + {k}, ")
        assert result["flags"] == want and result["n_appended"] == k and result["n_updated"] == 0
        assert (len(after[0][0]), nid) == ((ca.MAP_MAX_PLANES, 70 + k) if want == ca.COMMIT_DONE else (size, 70))
    room.restore()


# ---- 6. a chained frame ---------------------------------------------------------------------------------------------------------
def test_a_chained_frame_appends_the_planes_of_its_second_record():
    """the wall behind the lattice with 65 panes (tests/capacity_cases.py): 65 kept planes over two records, appended to an empty map
    in kept-plane order through the kept-plane table"""
    import cape_amd as ca
    from test_gpu_map_measure import _pose_covariances
    from test_gpu_match_wide import _extract

    depth, intr, _ = K.lattice_with(65, 1280, 960, 4, 5)
    ex, st = _extract(np.stack([depth]), 1280, 960, intr)
    assert len(ex.results(1).chain(0)) == 2
    ex.map_measure(1, None, _pose_covariances(np.random.default_rng(4), 1), st)
    meas = ex.map_measurements(1)
    stageable = [m for m in meas[0] if m["flags"] & ca.MEASURE_STAGEABLE]
    assert len(meas[0]) == 65 and len(stageable) == 65 and meas[0][-1]["segment"] >= 64
    ex.upload_map(ca.pack_map([]))
    ex.upload_tracks(np.zeros(0, ca.MAP_TRACK_DTYPE))
    ex.match_map_wide(1, None, None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(1, st)
    ex.map_union_cut(1, st)
    print()
    result, nid, after, _ = _commit_both(ca, ex, st, 1, 0, meas[0], ca.COMMIT_ADD_STAGED, 300, what="lattice of 65 panes, ")
    assert result["flags"] == ca.COMMIT_DONE and result["n_appended"] == 65 and nid == 365
    (P, R, V), Tr = after
    assert Tr["id"].tolist() == list(range(300, 365)) and np.all(Tr["flags"] == ca.MAP_TRACK_STAGED) and np.all(Tr["result"] == ca.MAP_RESULT_APPENDED)
    for j, m in enumerate(meas[0]):  # kept-plane order, the spill record's planes last
        ring = m["plane"][5]
        assert V[R[j]["vertex_offset"]: R[j]["vertex_offset"] + R[j]["vertex_count"]].tobytes() == np.ascontiguousarray(ring).tobytes(), j
        assert P[j]["normal"].tobytes() == np.ascontiguousarray(m["staged_normal"]).tobytes() and Tr[j]["covariance"].tobytes() == m["covariance"].tobytes()
    # the committed map is a map: the frame matches it plane for plane, and a second frame commits into it
    ex.match_map_wide(1, None, None, ca.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(1, st)
    ex.map_union_cut(1, st)
    result, nid, _, _ = _commit_both(ca, ex, st, 1, 0, meas[0], ca.COMMIT_ADD_STAGED, nid, what="lattice of 65 panes again, ")
    if result["flags"] & ca.COMMIT_DONE:
        assert result["n_planes"] == 65 + result["n_appended"] and result["n_updated"] + result["n_appended"] >= 1
    ex.close()


# ---- 7. bookkeeping -------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    # no union result is current
    with pytest.raises(ca.CapeError, match="cape_map_commit " + CAP):
        ex.map_commit(0, 0, 0, st)
    ex.map_union_cut(4, st)
    with pytest.raises(ca.CapeError, match="cape_map_commit " + CAP):
        ex.map_commit(4, 0, 0, st)  # beyond what the union covered
    with pytest.raises(ca.CapeError, match=r"cape_map_commit failed \(-1\)"):
        ex.map_commit(0, 2, 0, st)
    ex.map_union_cut(n, st)

    def buffers():
        rows, ver = ex.measurement_rows(n)
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in (*ex.map_matches_wide(n), rows, ver, *ex.map_kalman_rows(n), *ex.map_union_rows(n),
                                                                          ex.map_union_ring_rows(n))]

    print()
    f = room.source
    result, nid, committed, _ = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, 10, what="bookkeeping, ")
    assert result["flags"] == ca.COMMIT_DONE
    # after DONE: the Kalman and union results are gone until a new wide match; a second commit has no union
    with pytest.raises(ca.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(n, st)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    with pytest.raises(ca.CapeError, match="cape_map_commit " + CAP):
        ex.map_commit(f, 0, nid, st)
    # the measurement rows are still valid, and the tracks are the committed ones: wide match + Kalman without upload_tracks
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    frames, rows, results = ex.map_kalman_rows(n)
    _, match, _, _ = ex.map_matches_wide(n)
    for g in range(n):
        frame, trows, tres = ca.host_map_kalman(committed[0], committed[1], match[g], room.meas[g])
        k = len(room.meas[g])
        assert frames[g].tobytes() == frame.tobytes() and rows[g, :k].tobytes() == trows.tobytes() and results[g].tobytes() == tres.tobytes(), g
    # a refused commit (the map made full) leaves every result buffer as it was
    arrays, tracks = _wall_copies(ca, room, ca.MAP_MAX_PLANES, np.random.default_rng(8), far=True)
    _pipeline(room, arrays, tracks)
    full = buffers()
    result, _, _, _ = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, 10, what="bookkeeping, the full map, ")
    assert result["flags"] == ca.COMMIT_CAPACITY
    assert all(np.array_equal(a, b) for a, b in zip(full, buffers())), "a refused commit wrote into a result buffer"
    ex.map_kalman_rows(n), ex.map_union_rows(n)  # (still current)
    room.restore()
