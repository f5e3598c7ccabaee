"""cape_match_map_shards: the persistent-map matcher fed by gathered shards in device memory instead of the handle's records.  Every
expected value is bit for bit: a packed shard equals the record path (cape_match_map) on the frames it was packed from, ragged shards
on a handle that never extracted equal the host route (cape_host_shard_frame + cape_host_match_map), a chained frame of more than 64
kept planes is flagged beside a served one, dropped rings / planes flag exactly the frames that hold them, and shards whose header or
indices do not fit the layout are refused without being read.  The receive buffer of a gather is assembled by hand: rank after rank, byte for byte
what ncclAllGather delivers."""
import numpy as np
import pytest

from test_gpu_map_match import _bits, _checker_frames, _kept, _lift, _map_from, _stream, _w2c

pytestmark = pytest.mark.gpu

EYE = (np.eye(3), np.zeros(3))


def _skip_words(rng, n, n_map):
    return rng.integers(0, 2**32, (n, (n_map + 31) // 32), dtype=np.uint64).astype(np.uint32) & np.uint32(0x5A5A5A5A)


def _assert_same(a, b, rows=None):
    """two (frames, match, inter_area) results are equal in every field and bit"""
    rows = slice(None) if rows is None else rows
    assert np.array_equal(a[0][rows], b[0][rows])
    assert np.array_equal(a[1][rows], b[1][rows])
    assert np.array_equal(_bits(a[2][rows]), _bits(b[2][rows]))


def _assert_flagged(res, s, flags):
    """a flagged slot reports nothing"""
    frames, match, inter = res
    assert frames[s]["flags"] == flags, (s, frames[s]["flags"])
    assert np.all(match[s] == -1) and np.all(frames[s]["map_of"] == -1) and frames[s]["n_matched"] == 0 and np.all(inter[s] == -1.0)


def _assert_equals_host_route(res, s, buf, layout, k, arrays, T, skip, flags):
    """slot s against cape_host_shard_frame + cape_host_match_map on the shard's bytes; returns seg_cur of the slot"""
    import cape_amd

    frames, match, inter = res
    det, segs = cape_amd.host_shard_frame(buf, layout, k)
    g = frames[s]
    n = len(det)
    assert g["n_cur"] == n and list(g["seg_cur"][:n]) == list(segs) and np.all(g["seg_cur"][n:] == -1)
    m, mo, ia = cape_amd.host_match_map(arrays, [d[:7] for d in det], T, skip, flags, areas=True)
    assert list(match[s]) == list(m), f"slot {s}"
    assert list(g["map_of"][:n]) == list(mo) and np.all(g["map_of"][n:] == -1)
    assert g["n_matched"] == sum(1 for v in m if v >= 0)
    assert np.array_equal(_bits(inter[s][:, :n]), _bits(ia)), f"slot {s}: areas differ from the host class"
    assert np.all(inter[s][:, n:] == -1.0)
    return list(segs)


# ---- 1. one shard equals the record path -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,stride", [("room", 5), ("tumlike", 3), ("tunnel", 4)])
def test_one_shard_equals_the_record_path(scene, stride):
    import cape_amd

    n = 24
    ex, st, c2w = _stream(scene, 11, 20, stride, n)
    kept = _kept(ex, n)
    rng = np.random.default_rng(5)
    planes = _map_from(kept, c2w, (0, 9, 23), rng)
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    layout = ex.gather_configure(n, planes_per_frame=64, polygons=True, vertices_per_frame=ex.boundary_capacity)  # nothing can be dropped
    ptr = ex.pack(n, 0, st)
    matched = 0
    for flags in range(4):
        for use_skip in (False, True):
            skip = _skip_words(rng, n, len(planes)) if use_skip else None
            ex.match_map(n, T, skip, flags | cape_amd.MATCH_MAP_AREAS, st)
            want = ex.map_matches(n, areas=True)
            ex.match_map_shards(ptr, 1, layout, T, skip, flags | cape_amd.MATCH_MAP_AREAS, st)
            got = ex.shard_map_matches(n, areas=True)
            _assert_same(got, want)
            assert int(np.count_nonzero(got[0]["flags"] == 0)) >= n - 4
            matched += int(got[0]["n_matched"].sum())
    assert matched > n  # the true poses find the planes the map was built from
    ex.close()


# ---- 2., 6., 7.: three ragged shards in a buffer of four -----------------------------------------------------------------------------

class _Ragged:
    pass


@pytest.fixture(scope="module")
def ragged(hip_library):
    """A producer of frames_capacity 8 packs shards of 5, 8 and 3 frames of three batches (first_frame 0, 5, 13); their bytes on the
    host, a map from some of their planes, poses and skip words by slot, and the baseline result of a handle that never extracted."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu
    from cape_amd.dist import slot_of

    R = _Ragged()
    R.sizes, R.first = (5, 8, 3), (0, 5, 13)
    total, start, stride, seed = 16, 20, 5, 11
    idx = [start + stride * i for i in range(total)]
    dev = torch.cat([synth_gpu.stream("room", seed, 1, start=f, device="cuda", chunk=1) for f in idx]).contiguous()
    poses = synth_gpu._poses("room", seed, 0, start + stride * total)
    R.c2w = [poses[f] for f in idx]
    prod = Extractor(640, 480, cylinders=False, max_batch=16, **synth.DEFAULT_INTRINSICS)
    st = torch.cuda.current_stream().cuda_stream
    R.layout = dict(prod.gather_configure(8, planes_per_frame=64, polygons=True, vertices_per_frame=prod.boundary_capacity))
    R.bytes = R.layout["bytes_per_rank"]
    R.shards = []
    for n, first in zip(R.sizes, R.first):
        prod.extract_device(dev[first:first + n].data_ptr(), n, st)
        prod.build_polygons(n, st)
        prod.pack(n, first, st)
        R.shards.append(prod.packed_host())
    # (the last batch once more without polygons, for the bad-shard cases)
    plain = prod.gather_configure(8, planes_per_frame=64)
    prod.pack(R.sizes[-1], R.first[-1], st)
    R.without_polygons = np.zeros(R.bytes, np.uint8)
    R.without_polygons[: plain["bytes_per_rank"]] = prod.packed_host()
    prod.gather_configure(8, planes_per_frame=64, polygons=True, vertices_per_frame=prod.boundary_capacity)
    R.producer, R.stream = prod, st
    # the kept planes of every frame from the shard bytes, a map of about 60 planes out of three of them
    kept = {}
    for s, (n, first) in enumerate(zip(R.sizes, R.first)):
        for k in range(n):
            det, segs = cape_amd.host_shard_frame(R.shards[s], R.layout, k)
            kept[first + k] = [(int(sg), d[:7]) for sg, d in zip(segs, det)]
    rng = np.random.default_rng(7)
    R.planes = _map_from(kept, R.c2w, (1, 6, 14), rng, size=60)
    R.arrays = cape_amd.pack_map(R.planes)
    R.n_slots = 3 * 8
    R.T = np.stack([np.eye(4)] * R.n_slots)
    for s, (n, first) in enumerate(zip(R.sizes, R.first)):
        for k in range(n):
            R.T[slot_of(s, k, R.layout)] = _w2c(*R.c2w[first + k])
    R.skip = _skip_words(rng, R.n_slots, len(R.planes))
    # FOUR shards' length: the fourth stays zero and is never passed -- a wrong bounds check then reads zeros, not beyond the tensor
    R.host = np.zeros(4 * R.bytes, np.uint8)
    for s in range(3):
        R.host[s * R.bytes:(s + 1) * R.bytes] = R.shards[s]
    R.device = torch.from_numpy(R.host).cuda()
    R.owner = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)  # never extracts
    R.owner.upload_map(R.planes)
    R.owner.match_map_shards(R.device.data_ptr(), 3, R.layout, R.T, R.skip, cape_amd.MATCH_MAP_AREAS, st)
    R.baseline = R.owner.shard_map_matches(R.n_slots, areas=True)
    yield R
    R.owner.close()
    prod.close()


def test_three_ragged_shards_on_a_handle_that_never_extracted(ragged):
    import cape_amd
    from cape_amd.dist import shard_of, slot_of

    R = ragged
    frames, match, inter = R.baseline
    served = 0
    for s, n in enumerate(R.sizes):
        for k in range(8):
            slot = slot_of(s, k, R.layout)
            assert shard_of(slot, R.layout) == (s, k)
            g = frames[slot]
            assert g["n_map"] == len(R.planes)
            if k >= n:  # an empty slot
                assert g["n_cur"] == 0 and g["n_matched"] == 0 and g["flags"] == 0
                assert np.all(match[slot] == -1) and np.all(g["seg_cur"] == -1) and np.all(g["map_of"] == -1) and np.all(inter[slot] == -1.0)
            elif not g["flags"] & cape_amd.MATCH_EXACT_OVERFLOW:
                _assert_equals_host_route(R.baseline, slot, R.shards[s], R.layout, k, R.arrays, R.T[slot], R.skip[slot], 0)
                served += 1
            else:
                _assert_flagged(R.baseline, slot, cape_amd.MATCH_EXACT_OVERFLOW)
    assert served >= sum(R.sizes) - 2 and int(frames["n_matched"].sum()) > 8
    # the producer: a cape_match_map between two shard calls -- neither call disturbs the other's copy-out
    prod, st = R.producer, R.stream
    prod.upload_map(R.planes)
    n, first = R.sizes[-1], R.first[-1]
    Tb = np.stack([_w2c(*R.c2w[first + k]) for k in range(n)])
    prod.match_map_shards(R.device.data_ptr(), 3, R.layout, R.T, R.skip, cape_amd.MATCH_MAP_AREAS, st)
    prod.match_map(n, Tb, None, cape_amd.MATCH_MAP_AREAS, st)
    records = prod.map_matches(n, areas=True)
    _assert_same(prod.shard_map_matches(R.n_slots, areas=True), R.baseline)
    prod.match_map_shards(R.device.data_ptr(), 2, R.layout, R.T[:16], None, 0, st)
    _assert_same(prod.map_matches(n, areas=True), records)
    assert np.array_equal(prod.shard_map_matches(16)[0]["n_cur"], frames["n_cur"][:16])


def _polygons_view(buf, layout):
    import cape_amd

    o = layout["polygons_offset"]
    return buf[o: o + layout["polygons_capacity"] * cape_amd.POLYGON_DTYPE.itemsize].view(cape_amd.POLYGON_DTYPE)


def _frames_view(buf, layout):
    import cape_amd

    o = layout["frames_offset"]
    return buf[o: o + layout["frames_capacity"] * cape_amd.PACKED_FRAME_DTYPE.itemsize].view(cape_amd.PACKED_FRAME_DTYPE)


def _header_view(buf):
    import cape_amd

    return buf[: cape_amd.PACKED_HEADER_DTYPE.itemsize].view(cape_amd.PACKED_HEADER_DTYPE)


@pytest.mark.parametrize("case", ["magic", "without_polygons", "planes_capacity", "n_frames", "plane_offset", "ring"])
def test_bad_shards_are_refused_without_being_read(ragged, case):
    """One corruption per case, in a copy of shard 1 inside the four-shard buffer (values small enough that even an unchecked read
    would stay inside the tensor): the affected slots carry BAD_SHARD | OVERFLOW and report nothing, every other slot is unchanged."""
    import torch
    import cape_amd
    from cape_amd.dist import slot_of

    R = ragged
    host = R.host.copy()
    shard = host[R.bytes: 2 * R.bytes]
    affected = [slot_of(1, k, R.layout) for k in range(8)]
    if case == "magic":
        _header_view(shard)["magic"] = 0
    elif case == "without_polygons":
        shard[:] = R.without_polygons
        assert not int(_header_view(shard)["flags"][0]) & cape_amd.GATHER_POLYGONS
    elif case == "planes_capacity":
        _header_view(shard)["planes_capacity"] += 1
    elif case == "n_frames":
        _header_view(shard)["n_frames"] = R.layout["frames_capacity"] + 1
    elif case == "plane_offset":
        fr = _frames_view(shard, R.layout)
        fr["plane_offset"][2], fr["n_planes"][2] = R.layout["planes_capacity"] - 1, 3
        affected = [slot_of(1, 2, R.layout)]
    else:
        fr = _frames_view(shard, R.layout)
        pol = _polygons_view(shard, R.layout)
        k = next(k for k in range(R.sizes[1]) if fr["n_planes"][k] > 0 and pol["vertex_count"][fr["plane_offset"][k]] >= 3)
        first = int(fr["plane_offset"][k])
        pol["vertex_offset"][first], pol["vertex_count"][first] = R.layout["vertices_capacity"] - 1, 5
        affected = [slot_of(1, k, R.layout)]
        assert R.baseline[0][affected[0]]["n_cur"] > 0 and R.baseline[0][affected[0]]["flags"] == 0
    dev = torch.from_numpy(host).cuda()
    R.owner.match_map_shards(dev.data_ptr(), 3, R.layout, R.T, R.skip, cape_amd.MATCH_MAP_AREAS, R.stream)
    got = R.owner.shard_map_matches(R.n_slots, areas=True)
    for s in affected:
        _assert_flagged(got, s, cape_amd.MATCH_EXACT_BAD_SHARD | cape_amd.MATCH_EXACT_OVERFLOW)
        assert got[0][s]["n_cur"] == 0 and np.all(got[0][s]["seg_cur"] == -1)
    others = np.array([s for s in range(R.n_slots) if s not in affected])
    _assert_same(got, R.baseline, others)
    assert not np.any(R.baseline[0]["flags"][affected] & cape_amd.MATCH_EXACT_BAD_SHARD)


def test_arguments(ragged):
    import cape_amd
    from cape_amd import CapeError, Extractor, synth

    R = ragged
    own, ptr, st = R.owner, R.device.data_ptr(), R.stream
    with pytest.raises(CapeError, match=r"\(-1\)"):
        own.match_map_shards(0, 3, R.layout, R.T, R.skip, 0, st)  # a NULL pointer
    with pytest.raises(CapeError, match=r"\(-1\)"):
        own.match_map_shards(ptr, 0, R.layout, None, None, 0, st)
    with pytest.raises(CapeError, match=r"\(-1\)"):
        own.match_map_shards(ptr, 3, R.layout, R.T, R.skip, 1 << 7, st)
    for field, value in (("vertices_offset", R.layout["vertices_offset"] + 8),      # not 16-byte aligned
                         ("bytes_per_rank", R.layout["bytes_per_rank"] - 16),       # the vertex section does not fit
                         ("planes_offset", R.layout["bytes_per_rank"]),
                         ("polygons_offset", R.layout["planes_offset"]),                  # two sections overlap
                         ("polygons_capacity", R.layout["polygons_capacity"] + 1)):
        with pytest.raises(CapeError, match=r"\(-1\)"):
            own.match_map_shards(ptr, 3, dict(R.layout, **{field: value}), R.T, R.skip, 0, st)
    fresh = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)
    with pytest.raises(CapeError, match=r"\(-1\)"):  # no map uploaded
        fresh.match_map_shards(ptr, 3, R.layout, None, None, 0, st)
    with pytest.raises(CapeError, match=r"\(-4\)"):  # nothing matched yet
        fresh.shard_map_matches(1)
    # the dense table beyond 1 GiB: refused before anything is launched (the shards are never touched)
    too_many = (1 << 30) // (8 * 64 * len(R.planes) * R.layout["frames_capacity"]) + 1
    with pytest.raises(CapeError, match=r"\(-4\)"):
        own.match_map_shards(ptr, too_many, R.layout, None, None, cape_amd.MATCH_MAP_AREAS, st)
    # an empty map: all -1
    fresh.upload_map([])
    fresh.match_map_shards(ptr, 3, R.layout, R.T, None, 0, st)
    frames, match = fresh.shard_map_matches(R.n_slots)
    assert match.shape == (R.n_slots, 0) and np.all(frames["map_of"] == -1) and np.all(frames["n_matched"] == 0) and np.all(frames["n_map"] == 0)
    assert np.array_equal(frames["n_cur"], R.baseline[0]["n_cur"])
    with pytest.raises(CapeError, match=r"\(-1\)"):  # the call did not keep the table
        fresh.shard_map_matches(R.n_slots, areas=True)
    with pytest.raises(CapeError, match=r"\(-4\)"):
        fresh.shard_map_matches(R.n_slots + 1)
    fresh.close()
    # (the refused calls left the owner's last result alone only where they failed before touching it; a served call follows)
    own.match_map_shards(ptr, 3, R.layout, R.T, R.skip, cape_amd.MATCH_MAP_AREAS, st)
    _assert_same(own.shard_map_matches(R.n_slots, areas=True), R.baseline)


# ---- 3. more than 16 and up to 64 kept planes ------------------------------------------------------------------------------------

def test_more_than_16_kept_planes_are_served_from_a_shard():
    import torch
    import cape_amd
    from cape_amd import Extractor, synth

    W, H = 640, 480
    big, intr = _checker_frames(W, H, 80)
    dev = torch.from_numpy(np.stack([big, synth.room(seed=2, frame=5, width=W, height=H, intr=intr)])).cuda()
    ex = Extractor(W, H, cylinders=False, max_batch=2, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), 2, st)
    ex.build_polygons(2, st)
    kept = _kept(ex, 2)
    assert 16 < len(kept[0]) <= 64, len(kept[0])
    planes = [(nn, d, x, y, c, ring + [7.0, 5.0], h) for nn, d, x, y, c, ring, h in _map_from(kept, [EYE, EYE], [0], np.random.default_rng(4), size=120)]
    ex.upload_map(planes)
    layout = ex.gather_configure(2, planes_per_frame=64, polygons=True, vertices_per_frame=ex.boundary_capacity)
    ptr = ex.pack(2, 0, st)
    for flags in (cape_amd.MATCH_ALLOW_INDEX0, 0):
        ex.match_map(2, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        want = ex.map_matches(2, areas=True)
        ex.match_map_shards(ptr, 1, layout, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        got = ex.shard_map_matches(2, areas=True)
        _assert_same(got, want)
        assert got[0][0]["flags"] == 0 and got[0][0]["n_cur"] == len(kept[0])
        assert int(got[1][0].max()) >= 16, "kept planes beyond the first 16 are matched"
    ex.close()


# ---- 4. chained frames -----------------------------------------------------------------------------------------------------------

def test_chained_frames():
    """A frame that continued in spill records on its producer has all its planes side by side in the shard.  The 1280x960
    checkerboard of 116 facets keeps more than 64 planes: its slot is flagged, and the room frame beside it is served.

    The other half -- a chained frame that keeps AT MOST 64 planes is served, seg_cur beyond 63 included -- has no test: no generator
    input was found that has more than 64 plane segments and at most 64 kept planes.  Every checkerboard of facets tried (1280x960
    tiles 100..150, 1280x720 tiles 90..150, 960x720 tiles 90..150, and the same with a crease of 0.05..0.3 through every facet) has
    exactly as many output planes and kept planes as segments (e.g. 70 / 70 / 70 at 1280x960 tile 130, 63 / 63 / 63 at tile 135),
    synth.facets with 150..600 planes gives 3..6 segments, and coplanar half-facets with a depth step between them (cell-aligned,
    tile 160, steps 25..85 mm) either grow through, or split without merging (95 / 95), or give 16..36 segments that are all planes.  A wall behind a lattice
    with stepped half-panes meant to merge (tests/capacity_cases.py's lattice, depth steps of 20 to 60 mm) was tried too: 47, 0 or 111 segments, with as many planes.  The path itself is the one this test and
    test_more_than_16_kept_planes_are_served_from_a_shard run: the gate kernel never looks at the segment count."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth

    W, H = 1280, 960
    big, intr = _checker_frames(W, H, 100)
    dev = torch.from_numpy(np.stack([synth.room(seed=1, frame=0, width=W, height=H, intr=intr), big])).cuda()
    ex = Extractor(W, H, cylinders=False, max_batch=2, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), 2, st)
    ex.build_polygons(2, st)
    assert ex.results(2).records["header"]["n_plane_segments"][1] == 116
    # a budget the chain cannot exceed: boundary_capacity vertices per record of it
    layout = ex.gather_configure(2, planes_per_frame=128, polygons=True, vertices_per_frame=2 * ex.boundary_capacity)
    ptr = ex.pack(2, 0, st)
    buf = ex.packed_host()
    assert int(_header_view(buf)["overflow"][0]) == 0
    det = [cape_amd.host_shard_frame(buf, layout, k) for k in range(2)]
    assert len(det[1][0]) > 64 and max(det[1][1]) >= 64
    # the room's planes and every third facet, shifted (see _oracle_decisions); index 0 allowed: the room keeps few planes
    planes = [_lift(d[:7], *EYE, ring=d[5] + [7.0, 5.0]) for d in det[0][0] + det[1][0][::3]]
    flags = cape_amd.MATCH_ALLOW_INDEX0
    ex.upload_map(planes)
    ex.match_map(2, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
    records = ex.map_matches(2, areas=True)
    assert records[0][0]["flags"] == 0 and records[0][1]["flags"] == cape_amd.MATCH_EXACT_OVERFLOW
    ex.match_map_shards(ptr, 1, layout, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
    got = ex.shard_map_matches(2, areas=True)
    _assert_same(got, records, slice(0, 1))  # the room frame beside it is served
    assert got[0][0]["flags"] == 0 and got[0][0]["n_matched"] > 0
    _assert_flagged(got, 1, cape_amd.MATCH_EXACT_OVERFLOW)
    _assert_equals_host_route(got, 0, buf, layout, 0, cape_amd.pack_map(planes), None, None, flags)
    ex.close()


# ---- 5. dropped rings and planes ---------------------------------------------------------------------------------------------------

def test_dropped_rings_and_planes_flag_the_frames_that_hold_them():
    import cape_amd

    n = 24
    ex, st, c2w = _stream("room", 11, 20, 5, n)
    kept = _kept(ex, n)
    planes = _map_from(kept, c2w, (0, 9, 23), np.random.default_rng(5))
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    want = ex.map_matches(n, areas=True)
    total, _ = ex.count_polygon_vertices(n)
    for budget, dropped_flag in ((dict(planes_per_frame=64, vertices_per_frame=max(1, total // (2 * n))), cape_amd.PACKED_VERTICES_DROPPED),
                                 (dict(planes_per_frame=2, vertices_per_frame=ex.boundary_capacity), cape_amd.PACKED_PLANES_DROPPED)):
        layout = ex.gather_configure(n, polygons=True, **budget)
        ptr = ex.pack(n, 0, st)
        buf = ex.packed_host()
        assert int(_header_view(buf)["overflow"][0]) == dropped_flag
        ex.match_map_shards(ptr, 1, layout, T, None, cape_amd.MATCH_MAP_AREAS, st)
        got = ex.shard_map_matches(n, areas=True)
        fr, pol = _frames_view(buf, layout), _polygons_view(buf, layout)
        whole, cut = [], []
        for k in range(n):
            a, b = int(fr["plane_offset"][k]), int(fr["plane_offset"][k]) + int(fr["n_planes"][k])
            lost = b > layout["planes_capacity"] or bool(np.any(pol["vertex_offset"][a:b] == 0xFFFFFFFF))
            (cut if lost else whole).append(k)
        assert whole and cut, (whole, cut)
        _assert_same(got, want, np.array(whole))  # wholly before the first dropped ring / plane: served like the record path
        for k in cut:
            _assert_flagged(got, k, cape_amd.MATCH_EXACT_OVERFLOW)
    ex.close()
