"""cape_map_measure: the measurement half of the map update on the device -- per kept plane the world plane, its covariance and
the polygon in world space -- against its host twin cape_host_map_update(CAPE_MAP_ADD_STAGED) on an empty map, which appends every
plane it can measure.  What does not pass through pow(s, 3 / 2) -- the decisions, the world plane, the polygon frame, every ring
vertex -- is compared bit for bit; the two covariances with _rel < 1e-12, the measure and figure of tests/test_map_update_host.py.

Every test prints its figures before it asserts (`pytest -s`): the largest _rel and how many covariances differ from the twin's in any bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUND = 1e-12


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _c2w(R, o):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, o
    return T


def _normalize3(n):
    """map_tracking's normalize3 in numpy scalars"""
    z = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    return n / z if z > 0 else n.copy()


def _pose_covariances(rng, n):
    """a pose covariance of a few mm^2 per frame"""
    from test_map_update_host import _spd

    return np.stack([_spd(rng, 3, 1.0) for _ in range(n)])


def _detected(ex, n):
    """per frame: (kept planes with the segment's point-cloud covariance as the 8th item, their segment positions)"""
    res = ex.results(n, with_boundary=False)
    out = []
    for f, (det, segs) in enumerate(ex.kept_planes(n)):
        S = res.segments(f)
        out.append(([d + (S[s]["cov"].reshape(3, 3).copy(),) for d, s in zip(det, segs)], segs))
    return out


def _twin(det, T, S):
    """cape_host_map_update on an empty map with CAPE_MAP_ADD_STAGED, in chunks of at most 64 planes: per detected plane the
    appended (plane row, track row, ring), or None where the twin appends nothing"""
    import cape_amd

    out = []
    for at in range(0, len(det), 64):
        chunk = det[at: at + 64]
        (P, R, V), Tr, used, _ = cape_amd.host_map_update(cape_amd.pack_map([]), np.zeros(0, cape_amd.MAP_TRACK_DTYPE), [], chunk, T, S,
                                                          cape_amd.MAP_ADD_STAGED)
        assert not used.any() and np.all(Tr["result"] == cape_amd.MAP_RESULT_APPENDED) and np.all(P["ring_count"] == 1)
        out.append([(P[k], Tr[k], V[R[P[k]["ring_first"]]["vertex_offset"]:][: R[P[k]["ring_first"]]["vertex_count"]]) for k in range(len(P))])
    return out


def _compare_frame(meas, det, segs, T, S, stats):
    """the measurements of one frame against the twin; returns the number of stageable planes compared"""
    import cape_amd
    from test_map_update_host import _rel

    KEPT, OK, LONG = cape_amd.MEASURE_KEPT, cape_amd.MEASURE_STAGEABLE, cape_amd.MEASURE_RING_TOO_LONG
    assert [m["segment"] for m in meas] == segs, "the kept planes are those of kept_planes, in order"
    twin = _twin(det, T, S)
    compared = 0
    for at, appended in zip(range(0, len(det), 64), twin):
        chunk = meas[at: at + 64]
        assert all(m["flags"] in (KEPT | OK, KEPT | LONG) for m in chunk), [hex(m["flags"]) for m in chunk]
        assert all((m["flags"] & LONG != 0) == (len(m["plane"][5]) > cape_amd.MAP_MAX_RING) for m in chunk)
        stageable = [m for m in chunk if m["flags"] & OK]
        assert len(stageable) == len(appended), "the twin appends exactly the stageable planes"
        for m, (P, Tr, ring) in zip(stageable, appended):
            normal, d, x, y, c, wring, holes = m["plane"]
            assert holes == [] and d == m["d"]
            for name, mine, theirs in (("staged_normal", m["staged_normal"], P["normal"]), ("d", m["d"], P["d"]), ("x_axis", x, P["x_axis"]),
                                       ("y_axis", y, P["y_axis"]), ("center", c, P["center"]), ("ring", wring, ring)):
                assert np.array_equal(_bits(mine), _bits(theirs)), f"segment {m['segment']}: {name} differs from the twin"
            assert np.array_equal(_bits(normal), _bits(m["staged_normal"]))
            assert np.array_equal(_bits(_normalize3(m["normal"])), _bits(m["staged_normal"]))
            rel = _rel(m["covariance"], Tr["covariance"])
            stats["rel"] = max(stats["rel"], rel)
            stats["bits"] += int(not np.array_equal(_bits(m["covariance"]), _bits(Tr["covariance"])))
            stats["n"] += 1
            assert rel < BOUND, f"segment {m['segment']}: covariance {rel:.3g} from the twin"
            compared += 1
    return compared


# ---- 1. the algebra through debug_eval -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(host_binaries):
    import cape_amd

    L = cape_amd._host_library()
    vp = C.c_void_p
    L.cape_host_covariance_valid.argtypes = [vp, C.c_int]
    L.cape_host_plane_covariance.argtypes = [vp, C.c_double, vp, vp]
    L.cape_host_world_plane_covariance.argtypes = [vp, C.c_double, vp, vp, vp, vp]
    return L


def test_covariance_algebra_equals_the_host_twin(host):
    import cape_amd
    from test_map_update_host import _c, _p, _pose, _rel, _spd, _unit

    rng = np.random.default_rng(3)
    rows9, rows10, ref9, ref10 = [], [], [], []
    for _ in range(200):
        n, d = _unit(rng), rng.uniform(300, 4000) * rng.choice([-1, 1])
        pcc = _c(_spd(rng, 3, rng.uniform(0.1, 30)))
        out = np.zeros(16)
        ok9 = host.cape_host_plane_covariance(_p(n), d, _p(pcc), _p(out))
        T, pose = _c(_pose(rng)), _c(_spd(rng, 3, 1e-3))
        w = np.zeros(16)
        ok10 = host.cape_host_world_plane_covariance(_p(n), d, _p(T), _p(out), _p(pose), _p(w))
        rows9.append(np.concatenate([n, [d], pcc.ravel()]))
        rows10.append(np.concatenate([n, [d], T.ravel(), out, pose.ravel()]))
        ref9.append((ok9, out))
        ref10.append((ok10, w))
    for op, rows, ref in (("plane_cov", rows9, ref9), ("world_plane_cov", rows10, ref10)):
        got = cape_amd.debug_eval(op, np.stack(rows))
        assert got.shape == (200, 17)
        assert [int(g[0]) for g in got] == [ok for ok, _ in ref] and all(ok == 1 for ok, _ in ref), op
        rels = [_rel(g[1:].reshape(4, 4), r.reshape(4, 4)) for g, (_, r) in zip(got, ref)]
        differ = sum(int(not np.array_equal(_bits(g[1:]), _bits(r))) for g, (_, r) in zip(got, ref))
        print(f"\n{op}: largest _rel {max(rels):.3g} over 200 cases, {differ} matrices differ in a bit")
        assert max(rels) < BOUND, op
    # d = 0 and a normal of norm 1 + 1e-9: not a plane, like the host
    n, pcc = _unit(rng), _c(_spd(rng, 3, 1.0))
    bad = np.stack([np.concatenate([n, [0.0], pcc.ravel()]), np.concatenate([n * (1 + 1e-9), [1000.0], pcc.ravel()])])
    out = np.zeros(16)
    assert host.cape_host_plane_covariance(_p(_c(bad[0, :3])), 0.0, _p(pcc), _p(out)) == 0
    assert host.cape_host_plane_covariance(_p(_c(bad[1, :3])), 1000.0, _p(pcc), _p(out)) == 0
    got = cape_amd.debug_eval("plane_cov", bad)
    assert np.all(got == 0.0)


def test_covariance_validity_decides_like_the_host_twin(host):
    import cape_amd
    from test_map_update_host import _c, _p, _spd

    rng = np.random.default_rng(7)
    cases = []
    for n in (3, 4):
        for _ in range(20):
            cases.append((n, _spd(rng, n, rng.uniform(1e-3, 30))))
        A = _spd(rng, n, 1.0)
        nan, asym, indef = A.copy(), A.copy(), A.copy()
        nan[1, 1] = np.nan
        asym[0, 1] += 1e-3
        indef[n - 1, n - 1] = -5.0
        v = rng.normal(size=(n, 1))
        semi = np.zeros((n, n))
        semi[0, 0] = 2.0  # a zero pivot after the first, zeros below it
        semi2 = semi.copy()
        semi2[n - 1, n - 1] = 1e-300  # ... and a valid pivot after a zero one
        cases += [(n, nan), (n, asym), (n, indef), (n, -A), (n, np.zeros((n, n))), (n, semi), (n, semi2), (n, v @ v.T),
                  (n, np.diag([0.0] + [1.0] * (n - 1)))]
    rows = np.zeros((len(cases), 17))
    for k, (n, M) in enumerate(cases):
        rows[k, 0] = n
        rows[k, 1: 1 + n * n] = M.ravel()
    got = cape_amd.debug_eval("cov_valid", rows)
    want = [host.cape_host_covariance_valid(_p(_c(M)), n) for n, M in cases]
    assert [int(g) for g in got] == want
    assert 0 < sum(want) < len(want)


# ---- 2. eight room frames --------------------------------------------------------------------------------------------------
class _Room:
    pass


@pytest.fixture(scope="module")
def room():
    from test_gpu_map_match import _stream

    r = _Room()
    r.n = 8
    r.ex, r.st, r.c2w = _stream("room", 11, 20, 5, r.n)
    r.T = np.stack([_c2w(*r.c2w[f]) for f in range(r.n)])
    r.S = _pose_covariances(np.random.default_rng(21), r.n)
    r.ex.map_measure(r.n, r.T, r.S, r.st)
    r.rows, r.ver = r.ex.measurement_rows(r.n)
    r.meas = r.ex.map_measurements(r.n)
    r.det = _detected(r.ex, r.n)
    yield r
    r.ex.close()


def test_room_frames_equal_the_twin(room):
    import cape_amd

    stats = dict(rel=0.0, bits=0, n=0)
    pol, ver = room.ex.polygons(room.n)
    total = 0
    for f in range(room.n):
        det, segs = room.det[f]
        assert all(m["flags"] == cape_amd.MEASURE_KEPT | cape_amd.MEASURE_STAGEABLE for m in room.meas[f])
        total += _compare_frame(room.meas[f], det, segs, room.T[f], room.S[f], stats)
        # the world covariance is not the 0.01 I of a vanishing input: the comparison above is not vacuous
        assert all(np.max(np.abs(m["covariance"] - 0.01 * np.eye(4))) > 1e-4 for m in room.meas[f])
    print(f"\nroom frames: largest _rel {stats['rel']:.3g} over {stats['n']} kept planes, {stats['bits']} covariances differ in a bit")
    # rows of segments that are not kept are all zero, and the kept rows are exactly the kept planes
    kept = (room.rows["flags"] & cape_amd.MEASURE_KEPT) != 0
    assert int(kept.sum()) == total == sum(len(m) for m in room.meas) > 8
    assert not room.rows[~kept].view(np.uint8).any()
    assert np.array_equal(kept, (pol["flags"] & cape_amd.POLY_VALID != 0) & (pol["vertex_count"] >= 3))
    # the world rings are not copies of the camera rings
    moved = sum(int(not np.array_equal(_bits(m["plane"][5]), _bits(d[5]))) for f in range(room.n) for m, d in zip(room.meas[f], room.det[f][0]))
    assert moved > 0


# ---- 3. a chained frame ------------------------------------------------------------------------------------------------------
def test_a_chained_frame_is_measured_over_its_spill_record():
    import cape_amd
    from test_gpu_match_map_wide import _chained_input, _extract
    from test_map_update_host import _pose

    frames, Wd, Ht, intr = _chained_input()
    ex, st = _extract(frames, Wd, Ht, intr)
    n = len(frames)
    rng = np.random.default_rng(33)
    T, S = np.stack([_pose(rng) for _ in range(n)]), _pose_covariances(rng, n)
    ex.map_measure(n, T, S, st)
    meas, det = ex.map_measurements(n), _detected(ex, n)
    used, _, _ = ex.spill_info()
    assert used >= 1 and len(det[1][0]) > 64 and max(det[1][1]) >= 64, "frame 1 continues in a spill record"
    stats = dict(rel=0.0, bits=0, n=0)
    for f in range(n):
        _compare_frame(meas[f], det[f][0], det[f][1], T[f], S[f], stats)
    in_spill = sum(1 for m in meas[1] if m["segment"] >= 64)
    print(f"\nchained frame: largest _rel {stats['rel']:.3g} over {stats['n']} kept planes ({in_spill} of a spill record), "
          f"{stats['bits']} covariances differ in a bit")
    assert in_spill > 0 and stats["n"] > 64
    # the spill record's rows and world rings come through cape_copy_spill_measurements, indexed like its polygons
    res = ex.results(n, with_boundary=False)
    k = int(res.records["header"]["next_record"][1]) - ex.max_batch
    srows, sver = ex.spill_measurement_rows(k, 1)
    spol, _ = ex.spill_polygons(k, 1)
    kept = (srows[0]["flags"] & cape_amd.MEASURE_KEPT) != 0
    assert int(kept.sum()) == in_spill and not srows[0][~kept].view(np.uint8).any()
    tail = [m for m in meas[1] if m["segment"] >= 64]
    for m, i in zip(tail, np.flatnonzero(kept)):
        assert m["segment"] == 64 + i
        p = spol[0][i]
        assert np.array_equal(_bits(m["plane"][5]), _bits(sver[0][p["vertex_offset"]: p["vertex_offset"] + p["vertex_count"]]))
        assert np.array_equal(_bits(m["covariance"]), _bits(srows[0][i]["covariance"]))
    ex.close()


# ---- 4. failures follow the twin ---------------------------------------------------------------------------------------------
def test_failures_follow_the_twin(room):
    import cape_amd

    FAILS = cape_amd.MEASURE_FAIL_PLANE_COV | cape_amd.MEASURE_FAIL_WORLD_COV | cape_amd.MEASURE_FAIL_POLYGON
    T, S = room.T.copy(), room.S.copy()
    T[2, 1, 3] = np.nan    # a NaN translation
    S[5, 0, 1] += 1e-3     # an asymmetric pose covariance
    room.ex.map_measure(room.n, T, S, room.st)
    rows, ver = room.ex.measurement_rows(room.n)
    meas = room.ex.map_measurements(room.n)
    others = [f for f in range(room.n) if f not in (2, 5)]
    assert np.array_equal(rows[others].view(np.uint8), room.rows[others].view(np.uint8)) and np.array_equal(_bits(ver[others]), _bits(room.ver[others]))
    assert len(meas[2]) == len(room.meas[2]) > 0 and len(meas[5]) == len(room.meas[5]) > 0
    for m in meas[2]:
        assert m["flags"] & cape_amd.MEASURE_KEPT and m["flags"] & FAILS and not m["flags"] & cape_amd.MEASURE_STAGEABLE
        assert m["flags"] == cape_amd.MEASURE_KEPT | cape_amd.MEASURE_FAIL_WORLD_COV  # the first failing step, named
        assert not m["covariance"].any() and not m["normal"].any() and not m["plane"][5].any()
    assert _twin(room.det[2][0], T[2], S[2]) == [[]]  # the twin appends none
    for m in meas[5]:
        assert m["flags"] == cape_amd.MEASURE_KEPT | cape_amd.MEASURE_BAD_POSE_COV
        assert not m["covariance"].any() and not m["plane"][5].any()
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        _twin(room.det[5][0], T[5], S[5])
    room.ex.map_measure(room.n, room.T, room.S, room.st)  # (the fixture's state)


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------
def test_measurements_become_a_map_the_matcher_finds_again(room):
    import cape_amd
    from test_gpu_map_match import _w2c
    from test_gpu_match_map_wide import _compare_with_twin

    W2C = np.stack([_w2c(*room.c2w[f]) for f in range(room.n)])
    flags = cape_amd.MATCH_ALLOW_INDEX0
    kept = room.ex.kept_planes(room.n)
    # frame 0, and -- this stream's frame 0 shows no plane, so its map is the empty one -- the first frame with several planes
    several = next(f for f in range(room.n) if len(room.meas[f]) > 1)
    for f in sorted({0, several}):
        planes = [m["plane"] for m in room.meas[f] if m["flags"] & cape_amd.MEASURE_STAGEABLE]
        assert len(planes) == len(room.meas[f])
        room.ex.upload_map(cape_amd.pack_map(planes))
        room.ex.match_map_wide(room.n, W2C, None, flags | cape_amd.MATCH_MAP_AREAS, room.st)
        frames, match, seg_cur, map_of, inter = _compare_with_twin(room.ex, room.n, kept, planes, W2C, flags)
        assert list(match[f]) == list(range(len(planes))), f"in frame {f} every map plane takes the plane it came from"
        assert f != several or np.count_nonzero(inter[f] > 0) >= len(planes) > 1


# ---- 6. bookkeeping ------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):
    import torch

    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu
    from test_gpu_map_match import _w2c

    ex, n, st = room.ex, room.n, room.st
    # two calls give byte-equal results; the polygons and a preceding match_map_wide are left alone
    planes = [m["plane"] for m in next(m for m in room.meas if len(m) > 1)]
    ex.upload_map(cape_amd.pack_map(planes))
    W2C = np.stack([_w2c(*room.c2w[f]) for f in range(n)])
    ex.match_map_wide(n, W2C, None, cape_amd.MATCH_ALLOW_INDEX0 | cape_amd.MATCH_MAP_AREAS, st)
    before = ex.map_matches_wide(n, areas=True)
    pol0, ver0 = ex.polygons(n)
    ex.map_measure(n, room.T, room.S, st)
    rows, ver = ex.measurement_rows(n)
    assert np.array_equal(rows.view(np.uint8), room.rows.view(np.uint8)) and np.array_equal(_bits(ver), _bits(room.ver))
    pol1, ver1 = ex.polygons(n)
    assert np.array_equal(pol0.view(np.uint8), pol1.view(np.uint8)) and np.array_equal(_bits(ver0), _bits(ver1))
    after = ex.map_matches_wide(n, areas=True)
    assert int((before[1] >= 0).sum()) > 0
    assert all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(before, after))
    # fewer frames than the call covered may be copied, more may not
    ex.map_measure(4, room.T[:4], room.S[:4], st)
    assert np.array_equal(ex.measurement_rows(4)[0].view(np.uint8), room.rows[:4].view(np.uint8))
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_measurements failed \(-4\)"):
        ex.measurement_rows(5)
    ex.map_measure(n, room.T, room.S, st)  # (the fixture's state)
    # CAPE_ERR_CAPACITY: before build_polygons, for more frames than it covered, and from the copy calls after a new extract
    dev = torch.cat([synth_gpu.stream("room", 11, 1, start=20 + 5 * i, device="cuda", chunk=1) for i in range(4)]).contiguous()
    ex2 = Extractor(640, 480, cylinders=False, max_batch=4, **synth.DEFAULT_INTRINSICS)
    ex2.extract_device(dev.data_ptr(), 4, st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_measure failed \(-4\)"):
        ex2.map_measure(4, room.T[:4], room.S[:4], st)
    ex2.build_polygons(3, st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_measure failed \(-4\)"):
        ex2.map_measure(4, room.T[:4], room.S[:4], st)
    ex2.map_measure(3, room.T[:3], room.S[:3], st)
    assert np.count_nonzero(room.rows[:3]["flags"]) > 0, "the frames compared show planes"
    assert np.array_equal(ex2.measurement_rows(3)[0].view(np.uint8), room.rows[:3].view(np.uint8))
    ex2.extract_device(dev.data_ptr(), 4, st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_measurements failed \(-4\)"):
        ex2.measurement_rows(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_spill_measurements failed \(-4\)"):
        ex2.spill_measurement_rows(0, 0)
    rows_p, ver_p = C.c_void_p(), C.c_void_p()
    assert ex2.L.cape_device_map_measurements(ex2.h, C.byref(rows_p), C.byref(ver_p)) == -4
    ex2.close()
