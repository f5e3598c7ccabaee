"""cape_match_map: MapPlane::find_matches against a persistent map on the device (Feature_Map::get_matches,
feature_map.hpp:638-697).  Checked bit for bit against the host twin cape_host_match_map on synthetic streams with their true
poses, against physics on the room box, on maps with holes and long rings (every capacity tier), and for the argument checks."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _stream(scene, seed, start, stride, n):
    import torch
    from cape_amd import Extractor, synth, synth_gpu

    intr = synth.TUM_FR1_INTRINSICS if scene == "tumlike" else synth.DEFAULT_INTRINSICS
    frames = [start + stride * i for i in range(n)]
    dev = torch.cat([synth_gpu.stream(scene, seed, 1, start=f, device="cuda", chunk=1) for f in frames]).contiguous()
    poses = synth_gpu._poses(scene, seed, 0, start + stride * n)
    cam_to_world = [poses[f] for f in frames]
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    return ex, st, cam_to_world


def _w2c(R, o):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ o
    return T


def _kept(ex, n):
    """per frame: the kept planes as host_match_map takes them, and their segment indices"""
    from cape_amd.dist import kept_segments

    res = ex.results(n)
    pol, ver = ex.polygons(n)
    out = []
    for f in range(n):
        segs = res.segments(f)
        kept = []
        for i in kept_segments(res, pol, f):
            s, p = segs[i], pol[f, i]
            ring = ver[f, p["vertex_offset"]: p["vertex_offset"] + p["vertex_count"]].copy()
            kept.append((i, (s["out_normal"].copy(), float(s["d"]), p["x_axis"].copy(), p["y_axis"].copy(), p["center"].copy(), ring,
                             float(p["area"]))))
        out.append(kept)
    return out


def _lift(det, R, o, ring=None, holes=()):
    """a detected plane (camera) as a map plane (world): p_w = o + R p_c"""
    n, d, x, y, c, r, _ = det
    nw, cw = _unit(R @ n), o + R @ c
    return (nw, float(-(nw @ cw)), _unit(R @ x), _unit(R @ y), cw, r if ring is None else ring, list(holes))


def _map_from(kept, cam_to_world, frames, rng, size=100):
    planes = []
    for f in frames:
        R, o = cam_to_world[f]
        planes += [_lift(k, R, o) for _, k in kept[f]]
    base = list(planes)
    while len(planes) < size and base:
        n, d, x, y, c, ring, holes = base[int(rng.integers(len(base)))]
        # perturbed copy: the outline scaled / shifted, the plane moved along its normal
        shift = rng.uniform(-200, 200, 2)
        planes.append((n, d + float(rng.uniform(-120, 120)), x, y, c, ring * rng.uniform(0.7, 1.3) + shift, holes))
    order = rng.permutation(len(planes))
    return [planes[k] for k in order]


def _oracle_decisions(kept_f, planes, T, skip_f, flags):
    """polygon_oracle_py.find_matches on the visited map planes (hole-free maps), expanded back to the map's indices.

    Not for a map polygon that is a frame's own polygon carried to world and back: two rings equal up to a few ulps (5e-13 mm)
    have edges that nearly coincide, and the oracle's ring intersection returns 0 for them where the host class -- and the
    geometry -- give the full area.  The callers compare frames whose map polygons are other frames' or shifted copies."""
    import cape_amd
    import polygon_oracle_py as P

    P.build()
    def cw(ring):
        # the oracle takes clockwise rings (what Boost's correct leaves); a hull may come out the other way round, which the host
        # class's ring constructor and cape_map_upload re-orient
        x, y = ring[:, 0], ring[:, 1]
        return (ring[::-1] if np.sum(np.roll(x, 1) * y - x * np.roll(y, 1)) > 0 else ring).copy()

    visited = [j for j in range(len(planes)) if skip_f is None or not (int(skip_f[j >> 5]) >> (j & 31)) & 1]
    mp = [(planes[j][0], planes[j][1], P.Polygon(cw(planes[j][5]), planes[j][2], planes[j][3], planes[j][4])) for j in visited]
    dp = [(nn, d, P.Polygon(cw(ring), x, y, c, area=area)) for nn, d, x, y, c, ring, area in kept_f]
    om, oi = P.find_matches(mp, dp, T, advanced=bool(flags & cape_amd.MATCH_ADVANCED), allow_index0=bool(flags & cape_amd.MATCH_ALLOW_INDEX0))
    out = [-1] * len(planes)
    for k, j in enumerate(visited):
        out[j] = om[k]
    return out


def _compare_with_twin(ex, n, kept, planes, T, skip, flags, oracle=False, sources=()):
    import cape_amd

    arrays = cape_amd.pack_map(planes)
    frames, match, inter = ex.map_matches(n, areas=True)
    served = 0
    for f in range(n):
        g = frames[f]
        assert g["n_map"] == len(planes)
        if g["flags"] & cape_amd.MATCH_EXACT_OVERFLOW:
            continue
        served += 1
        segs = [s for s, _ in kept[f]]
        assert g["n_cur"] == len(segs) and list(g["seg_cur"][: len(segs)]) == segs and all(g["seg_cur"][len(segs):] == -1)
        m, mo, ia = cape_amd.host_match_map(arrays, [k for _, k in kept[f]], T[f], None if skip is None else skip[f], flags, areas=True)
        assert list(match[f]) == list(m), f"frame {f}"
        assert list(g["map_of"][: len(segs)]) == list(mo) and all(g["map_of"][len(segs):] == -1)
        assert g["n_matched"] == sum(1 for v in m if v >= 0)
        assert np.array_equal(_bits(inter[f][:, : len(segs)]), _bits(ia)), f"frame {f}: areas differ from the host class"
        assert np.all(inter[f][:, len(segs):] == -1.0)
        if oracle and f not in sources:
            assert list(match[f]) == _oracle_decisions([k for _, k in kept[f]], planes, T[f], None if skip is None else skip[f], flags), f"frame {f}"
    return served


@pytest.mark.parametrize("scene,stride", [("room", 5), ("tumlike", 3), ("tunnel", 4)])
def test_map_matches_equal_the_host_twin_bit_for_bit(scene, stride):
    import cape_amd

    n = 64
    ex, st, c2w = _stream(scene, 11, 20, stride, n)
    kept = _kept(ex, n)
    rng = np.random.default_rng(5)
    sources = (0, 9, 23)
    planes = _map_from(kept, c2w, sources, rng)
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    words = (len(planes) + 31) // 32
    matched = 0
    for flags, use_skip in ((0, False), (1, True), (2, False), (3, True)):
        skip = rng.integers(0, 2**32, (n, words), dtype=np.uint64).astype(np.uint32) & np.uint32(0x5A5A5A5A) if use_skip else None
        ex.match_map(n, T, skip, flags | cape_amd.MATCH_MAP_AREAS, st)
        assert _compare_with_twin(ex, n, kept, planes, T, skip, flags, oracle=True, sources=sources) >= n - 4
        matched += int(ex.map_matches(n)[0]["n_matched"].sum())
    assert matched > n  # the true poses find the planes the map was built from
    ex.close()


def test_analytic_room_faces():
    """The map = the six faces of the room box as world rectangles.  Through the true poses every kept plane whose world-lifted
    plane passes the gates of a face is matched to it; a pose 300 mm off along every face normal matches strictly fewer."""
    import cape_amd

    n = 32
    ex, st, c2w = _stream("room", 3, 10, 7, n)
    kept = _kept(ex, n)
    lo, hi = np.array([-2000.0, -1500.0, -1500.0]), np.array([2000.0, 1500.0, 3500.0])
    faces = []
    for ax in range(3):
        u, v = [k for k in range(3) if k != ax]
        for side, val in ((+1, lo[ax]), (-1, hi[ax])):
            nrm = np.zeros(3)
            nrm[ax] = side
            x, y = np.zeros(3), np.zeros(3)
            x[u], y[v] = 1.0, 1.0
            c = (lo + hi) / 2
            c[ax] = val
            hu, hv = (hi[u] - lo[u]) / 2, (hi[v] - lo[v]) / 2
            ring = np.array([[-hu, -hv], [-hu, hv], [hu, hv], [hu, -hv]])
            faces.append((nrm, float(-(nrm @ c)), x, y, c, ring, []))
    ex.upload_map(faces)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    ex.match_map(n, T, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    frames, match = ex.map_matches(n)
    expected = 0
    min_cos = abs(math.cos(math.radians(20)))
    for f in range(n):
        if frames[f]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW:
            continue
        R, o = c2w[f]
        for i, (_, k) in enumerate(kept[f]):
            nw, dw = _lift(k, R, o)[:2]
            gated = [j for j, fc in enumerate(faces) if abs(dw - fc[1]) < 100 and abs(nw @ fc[0]) > min_cos]
            if gated:
                assert frames[f]["map_of"][i] in gated, f"frame {f} plane {i}"
                expected += 1
    assert expected > n
    good = int(frames["n_matched"].sum())
    T_off = T.copy()
    T_off[:, :3, 3] += T_off[:, :3, :3] @ np.array([300.0, 300.0, 300.0])
    ex.match_map(n, T_off, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    assert int(ex.map_matches(n)[0]["n_matched"].sum()) < good
    ex.close()


def _circle(c, r, k, phase=0.0):
    a = phase + np.linspace(0, 2 * math.pi, k, endpoint=False)
    return np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)


def test_holes_and_long_rings_every_tier():
    import cape_amd

    n = 8
    ex, st, c2w = _stream("room", 4, 30, 5, n)
    kept = _kept(ex, n)
    planes = []
    for f in range(n):
        R, o = c2w[f]
        for _, k in kept[f]:
            ring = k[5]
            ctr, r = ring.mean(0), 0.6 * float(np.sqrt(k[6] / math.pi))
            for size in (20, 100, 400):  # tiers 0, 1 and the long ones
                holes = [_circle(ctr + [r * 0.3, 0], r * 0.15, 4), _circle(ctr - [r * 0.3, 0], r * 0.2, 6)]
                planes.append(_lift(k, R, o, _circle(ctr, r, size, 0.1 * f), holes))
                if len(planes) >= 240:
                    break
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS | cape_amd.MATCH_ALLOW_INDEX0, st)
    assert _compare_with_twin(ex, n, kept, planes, T, None, cape_amd.MATCH_ALLOW_INDEX0) >= n - 2
    frames, match, inter = ex.map_matches(n, areas=True)
    assert np.count_nonzero(inter > 0) > 20 and int(frames["n_matched"].sum()) > 0
    # a ring of 513 vertices is refused at upload (the caller simplifies first)
    bad = [(planes[0][0], planes[0][1], planes[0][2], planes[0][3], planes[0][4], _circle((0, 0), 500, 513), [])]
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.upload_map(bad)
    ex.close()


def test_persistence_empty_map_and_argument_checks():
    import torch
    import cape_amd
    from cape_amd import synth_gpu

    n = 16
    ex, st, c2w = _stream("room", 8, 0, 11, n)
    kept = _kept(ex, n)
    planes = _map_from(kept, c2w, [0, 5], np.random.default_rng(2), size=40)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    ex.upload_map(planes)
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    # a second batch on the same upload ...
    dev2 = torch.cat([synth_gpu.stream("room", 8, 1, start=200 + 3 * f, device="cuda", chunk=1) for f in range(n)]).contiguous()
    ex.extract_device(dev2.data_ptr(), n, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # the polygons of the new batch are not built yet
        ex.match_map(n, T, None, 0, st)
    ex.build_polygons(n, st)
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    second = ex.map_matches(n, areas=True)
    # ... equals a fresh upload before it
    ex.upload_map(planes)
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    again = ex.map_matches(n, areas=True)
    assert np.array_equal(second[1], again[1]) and np.array_equal(_bits(second[2]), _bits(again[2]))
    assert np.array_equal(second[0], again[0])
    # an empty map: nothing matched
    ex.upload_map([])
    ex.match_map(n, T, None, 0, st)
    frames, match = ex.map_matches(n)
    assert match.shape == (n, 0) and np.all(frames["map_of"] == -1) and np.all(frames["n_matched"] == 0)
    # argument checks
    good = planes[0]
    for bad in ([(good[0], good[1], good[2], good[3], good[4], good[5][:2], [])],             # ring of 2 vertices
                [(good[0], good[1], good[2] * 1.001, good[3], good[4], good[5], [])]):      # axis not unit
        with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
            ex.upload_map(bad)
    P, R, V = cape_amd.pack_map([good])
    R["vertex_offset"] = len(V)  # outside the vertex array
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.upload_map(P, R, V)
    P2 = P.copy()
    P2["ring_count"] = 0
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.upload_map(P2, cape_amd.pack_map([good])[1], V)
    ex.upload_map([good])
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_map(n, T, None, 1 << 7, st)
    ex.match_map(n - 2, T[: n - 2], None, 0, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # more frames than the last call covered
        ex.map_matches(n - 1)
    ex.close()


def _checker_frames(W, H, tile):
    from test_gpu_parity import _checkerboard_of_facets

    return _checkerboard_of_facets(W, H, tile=tile)


def test_more_than_16_kept_planes_are_served():
    """The consecutive matcher stops at 16 kept planes; this path serves every kept plane of the frame's first record (up to 64):
    a checkerboard of facets, its own planes as the map (identity pose), matched bit for bit like the host twin and like the oracle,
    kept-plane indices beyond 15 included."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth

    W, H = 640, 480
    big, intr = _checker_frames(W, H, 80)
    frames = np.stack([big, synth.room(seed=2, frame=5, width=W, height=H, intr=intr)])
    dev = torch.from_numpy(frames).cuda()
    ex = Extractor(W, H, cylinders=False, max_batch=2, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), 2, st)
    ex.build_polygons(2, st)
    kept = _kept(ex, 2)
    assert 16 < len(kept[0]) <= 64, len(kept[0])
    eye = (np.eye(3), np.zeros(3))
    planes = [(nn, d, x, y, c, ring + [7.0, 5.0], h)  # (shifted: see _oracle_decisions)
              for nn, d, x, y, c, ring, h in _map_from(kept, [eye, eye], [0], np.random.default_rng(4), size=120)]
    ex.upload_map(planes)
    T = np.stack([np.eye(4)] * 2)
    for flags in (cape_amd.MATCH_ALLOW_INDEX0, 0):
        ex.match_map(2, T, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        assert _compare_with_twin(ex, 2, kept, planes, T, None, flags, oracle=True) == 2
        fr, match = ex.map_matches(2)
        assert fr[0]["n_cur"] == len(kept[0]) and not (fr[0]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW)
        assert int(match[0].max()) >= 16, "kept planes beyond the first 16 are matched"
    ex.close()


def test_a_spilled_frame_is_flagged_and_left_to_the_host_twin():
    """A frame of 116 plane segments continues in a spill record: the device flags it CAPE_MATCH_EXACT_OVERFLOW and reports no match;
    the host twin then answers for it from the kept planes of the whole record chain."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth

    W, H = 1280, 960
    big, intr = _checker_frames(W, H, 100)
    frames = np.stack([synth.room(seed=1, frame=0, width=W, height=H, intr=intr), big])
    dev = torch.from_numpy(frames).cuda()
    ex = Extractor(W, H, cylinders=False, max_batch=2, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), 2, st)
    ex.build_polygons(2, st)
    res = ex.results(2)
    pol, ver = ex.polygons(2)
    spol, sver = ex.spill_polygons(0, ex.spill_info()[0])
    chain = res.chain(1)
    assert len(chain) == 2
    kept = []
    for part, (rec, _) in enumerate(chain):
        k = int(res.records["header"]["next_record"][1]) - ex.max_batch if part else None
        prow, vslab = (pol[1], ver[1]) if part == 0 else (spol[k], sver[k])
        for i in range(min(64, int(rec["header"]["n_plane_segments"]))):
            sg, p = rec["segments"][i], prow[i]
            if sg["is_output"] and (p["flags"] & cape_amd.POLY_VALID) and p["vertex_count"] >= 3:
                ring = vslab[p["vertex_offset"]: p["vertex_offset"] + p["vertex_count"]].copy()
                kept.append((sg["out_normal"].copy(), float(sg["d"]), p["x_axis"].copy(), p["y_axis"].copy(), p["center"].copy(), ring,
                             float(p["area"])))
    assert len(kept) > 64
    eye = (np.eye(3), np.zeros(3))
    planes = [_lift(k, *eye, ring=k[5] + [7.0, 5.0]) for k in kept[::3]]  # (shifted: see _oracle_decisions)
    ex.upload_map(planes)
    ex.match_map(2, None, None, cape_amd.MATCH_MAP_AREAS, st)
    fr, match, inter = ex.map_matches(2, areas=True)
    assert not (fr[0]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW)
    assert fr[1]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW
    assert np.all(match[1] == -1) and np.all(fr[1]["map_of"] == -1) and fr[1]["n_matched"] == 0 and np.all(inter[1] == -1.0)
    m, mo = cape_amd.host_match_map(cape_amd.pack_map(planes), kept, None, None, 0)
    assert sum(1 for v in m if v >= 0) >= len(planes) - 2, "the twin gives the frame's answer: its own planes are found"
    assert list(m) == _oracle_decisions(kept, planes, np.eye(4), None, 0)
    ex.close()
