"""CAPE_GATHER_POLYGONS on the host (no GPU): the layout arithmetic, the parser of the packed bytes, a world-2 gloo all-gather of
hand-built shards, and the host helper that turns a shard's frame into the detected planes of cape_host_match_map /
cape_host_map_update.  The device side of the same wire format is tests/test_gpu_gather_polygons.py."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = 768


def _frame_of(normal):
    """a plane frame (x_axis, y_axis) for a unit normal"""
    n = np.asarray(normal, float)
    r = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    x = np.cross(n, r)
    x /= np.linalg.norm(x)
    y = np.cross(n, x)
    return x, y / np.linalg.norm(y)


def _ring(cx, cy, rx, ry, n, phase=0.0):
    """an open clockwise ring: a polygon inscribed in an ellipse"""
    t = phase - 2 * np.pi * np.arange(n) / n
    return np.ascontiguousarray(np.stack([cx + rx * np.cos(t), cy + ry * np.sin(t)], axis=1))


def _planes_of(frame_index):
    """[(normal, d, ring or None, flags)] of one hand-made frame; frame 1 has no plane at all"""
    from cape_amd import POLY_OVERFLOW, POLY_SIMPLIFIED, POLY_VALID

    if frame_index % 4 == 1:
        return []
    out = [((0.0, 0.0, -1.0), 1500.0 + 10 * frame_index, _ring(20, -30, 400 + frame_index, 300, 7, 0.1), POLY_VALID),
           ((0.0, -1.0, 0.0), 900.0, _ring(0, 0, 250, 500, 11), POLY_VALID | POLY_SIMPLIFIED),
           ((-1.0, 0.0, 0.0), 700.0, None, POLY_OVERFLOW)]          # an output plane whose polygon was left to the host class
    if frame_index % 4 == 2:
        out.append(((0.6, 0.0, -0.8), 1200.0, _ring(5, 5, 100, 120, 3), POLY_VALID))
    return out


def _build_shard(frame_ids, first_frame, lay, drop_from=None):
    """the packed bytes of a shard holding frames `frame_ids`, as cape_pack_primitives lays them out (numpy only).  drop_from: the
    vertex budget in force (rings beyond it do not travel)."""
    import cape_amd as ca

    buf = np.zeros(lay["bytes_per_rank"], np.uint8)
    frames = buf[lay["frames_offset"]:][: lay["frames_capacity"] * 24].view(ca.PACKED_FRAME_DTYPE)
    planes = buf[lay["planes_offset"]:][: lay["planes_capacity"] * 152].view(ca.PACKED_PLANE_DTYPE)
    pol = buf[lay["polygons_offset"]:][: lay["polygons_capacity"] * 96].view(ca.POLYGON_DTYPE)
    ver = buf[lay["vertices_offset"]:][: lay["vertices_capacity"] * 16].view("<f8").reshape(-1, 2)
    cap = lay["vertices_capacity"] if drop_from is None else drop_from
    k = at = total = valid = 0
    dropped = False
    for slot, f in enumerate(frame_ids):
        rows = _planes_of(f)
        frames[slot] = (k, len(rows), 0, 0, 0, len(rows) + 1)
        for i, (normal, d, ring, flags) in enumerate(rows):
            x, y = _frame_of(normal)
            planes[k]["normal"], planes[k]["d"], planes[k]["segment"], planes[k]["point_count"] = normal, d, i + 1, 4000 + i
            planes[k]["sums"] = [1.0, 2.0, 3.0, 50.0 + i, 60.0, 70.0, 1.5, 2.5, 0.5]
            g = pol[k]
            g["x_axis"], g["y_axis"], g["center"], g["flags"], g["segment"] = x, y, -d * np.asarray(normal), flags, i + 1
            n = 0 if ring is None else len(ring)
            total += n
            valid += 1 if (flags & ca.POLY_VALID and n >= 3) else 0
            if n and at + n <= cap and not dropped:
                g["vertex_offset"], g["vertex_count"], g["area"] = at, n, 0.5 * abs(np.sum(ring[:, 0] * np.roll(ring[:, 1], -1) - np.roll(ring[:, 0], -1) * ring[:, 1]))
                ver[at:at + n] = ring
                at += n
            elif n:
                dropped = True
                g["vertex_offset"], g["vertex_count"] = 0xFFFFFFFF, 0
            k += 1
    hd = buf[:48].view(ca.PACKED_HEADER_DTYPE)
    hd[0] = (ca.PACKED_MAGIC, len(frame_ids), first_frame, k, 0, lay["planes_capacity"], lay["cylinders_capacity"],
             ca.PACKED_VERTICES_DROPPED if dropped else 0, 0, CELLS, lay["frames_capacity"], ca.GATHER_POLYGONS)
    buf[lay["polygon_header_offset"]:][:16].view(ca.PACKED_POLYGON_HEADER_DTYPE)[0] = (total, lay["vertices_capacity"], valid)
    return buf


def test_layout_with_polygons_extends_todays_layout():
    from cape_amd import GATHER_DEFAULT_VERTICES_PER_FRAME
    from cape_amd.dist import packed_layout

    # the default call is today's dict, key for key (tests/test_multigpu_gloo.py pins its numbers)
    assert packed_layout(4, 768, 16, 8, labels=True) == dict(
        frames_capacity=4, planes_capacity=64, cylinders_capacity=32, cells=768, frames_offset=48, planes_offset=144,
        cylinders_offset=144 + 64 * 152, plane_labels_offset=144 + 64 * 152 + 1024, cyl_labels_offset=144 + 64 * 152 + 1024 + 3072,
        bytes_per_rank=144 + 64 * 152 + 1024 + 2 * 3072)
    for frames, cells, ppf, cpf, labels, vpf in itertools.product((1, 5, 2048), (768, 3072, 1001), (1, 16, 37), (1, 8), (False, True), (0, 1, 7, 1536)):
        base = packed_layout(frames, cells, ppf, cpf, labels=labels)
        assert "polygons_offset" not in base and packed_layout(frames, cells, ppf, cpf, labels=labels, polygons=False, vertices_per_frame=vpf) == base
        lay = packed_layout(frames, cells, ppf, cpf, labels=labels, polygons=True, vertices_per_frame=vpf)
        for key, val in base.items():  # every existing section where it was
            assert lay[key] == val or key == "bytes_per_rank", key
        assert lay["polygons_capacity"] == base["planes_capacity"]
        assert lay["vertices_capacity"] == frames * (vpf or GATHER_DEFAULT_VERTICES_PER_FRAME)
        assert lay["polygon_header_offset"] == base["bytes_per_rank"]  # appended behind the last existing section, labels included
        assert lay["polygons_offset"] == lay["polygon_header_offset"] + 16
        assert lay["vertices_offset"] == lay["polygons_offset"] + lay["polygons_capacity"] * 96
        assert lay["bytes_per_rank"] == lay["vertices_offset"] + lay["vertices_capacity"] * 16
        assert all(lay[k] % 16 == 0 for k in lay if k.endswith("_offset") or k == "bytes_per_rank")


def test_shard_parses_polygons_and_rings():
    from cape_amd import PACKED_VERTICES_DROPPED
    from cape_amd.dist import Shard, packed_layout, primitives_by_frame, primitives_by_frame_with_polygons

    lay = packed_layout(6, CELLS, 4, 1, labels=True, polygons=True, vertices_per_frame=16)
    ids = [0, 1, 2, 3, 4]  # frame 1 holds no plane; one frame slot stays unused
    sh = Shard(_build_shard(ids, 10, lay), lay)
    assert len(sh.frames) == 5 and sh.first_frame == 10 and int(sh.polygon_header["n_vertices_total"]) == 4 * 18 + 3
    assert int(sh.polygon_header["n_polygons_valid"]) == 9
    for slot, f in enumerate(ids):
        rows = _planes_of(f)
        pol, rings = sh.frame_polygons(slot)
        assert len(pol) == len(rings) == len(sh.frame_planes(slot)) == len(rows)
        for (normal, d, ring, flags), g, r, pl in zip(rows, pol, rings, sh.frame_planes(slot)):
            assert int(g["flags"]) == flags and int(g["segment"]) == int(pl["segment"]) and float(pl["d"]) == d
            assert r.shape == ((0, 2) if ring is None else ring.shape) and (ring is None or r.tobytes() == ring.tobytes())
        kept = sh.kept_planes(slot)
        assert [int(g["segment"]) for _, g, _ in kept] == [i + 1 for i, row in enumerate(rows) if row[2] is not None]
    both = primitives_by_frame_with_polygons([sh])
    assert sorted(both) == [10, 11, 12, 13, 14] and len(both[11][0]) == len(both[11][2]) == 0 and len(both[12]) == 4
    assert {k: len(v) for k, v in primitives_by_frame([sh]).items()} == {k: 2 for k in both}  # the old sibling keeps its shape
    # a budget of 30 vertices: the rings of the first frame and the first of frame 2 travel, every later ring is dropped
    cut = Shard(_build_shard(ids, 10, lay, drop_from=30), lay)
    assert int(cut.header["overflow"]) == PACKED_VERTICES_DROPPED and int(cut.polygon_header["n_vertices_total"]) == 75
    assert [len(r) for r in cut.frame_polygons(0)[1]] == [7, 11, 0] and [len(r) for r in cut.frame_polygons(2)[1]] == [7, 0, 0, 0]
    assert [int(g["vertex_offset"]) for g in cut.frame_polygons(2)[0]] == [18, 0xFFFFFFFF, 0, 0xFFFFFFFF]
    with pytest.raises(ValueError):
        cut.kept_planes(0)
    # what is no shard of this layout raises
    bad = _build_shard(ids, 10, lay)
    bad[0] ^= 0xFF
    with pytest.raises(ValueError, match="magic"):
        Shard(bad, lay)
    with pytest.raises(AssertionError):
        Shard(_build_shard(ids, 10, lay)[:-16], lay)
    plain = packed_layout(6, CELLS, 4, 1, labels=True)
    flagless = _build_shard(ids, 10, lay)
    flagless[44:48] = 0  # header.flags
    with pytest.raises(ValueError, match="CAPE_GATHER_POLYGONS"):
        Shard(flagless, lay)
    with pytest.raises(ValueError, match="CAPE_GATHER_POLYGONS"):
        Shard(flagless[: plain["bytes_per_rank"]], plain).frame_polygons(0)


def _worker(rank, world, port, q):
    for p in (os.path.join(ROOT, "rgb-d-slam_amd", "python"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cape_amd.dist import all_gather_bytes, largest_shard, packed_layout, primitives_by_frame_with_polygons, shard_range, unpack_gathered

    n = 7  # ragged: 4 + 3
    lay = packed_layout(largest_shard(n, world), CELLS, 4, 1, labels=False, polygons=True, vertices_per_frame=24)
    a, b = shard_range(n, rank, world)
    local = _build_shard(list(range(a, b)), a, lay)
    shards = unpack_gathered(all_gather_bytes(torch.from_numpy(local), world).numpy(), world, lay)
    ok = [s.first_frame for s in shards] == [shard_range(n, r, world)[0] for r in range(world)]
    ok = ok and [len(s.frames) for s in shards] == [4, 3]
    by_frame = primitives_by_frame_with_polygons(shards)
    ok = ok and sorted(by_frame) == list(range(n))
    for f in range(n):
        planes, _, pol, rings = by_frame[f]
        rows = _planes_of(f)
        ok = ok and len(planes) == len(pol) == len(rings) == len(rows)
        for (normal, d, ring, flags), pl, g, r in zip(rows, planes, pol, rings):
            ok = ok and float(pl["d"]) == d and int(g["flags"]) == flags and (len(r) == 0 if ring is None else r.tobytes() == ring.tobytes())
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, bool(ok)))


def test_gloo_all_gather_of_shards_with_polygons():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + os.getpid() % 150
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_host_helper_feeds_the_map_matcher_from_a_shard(host_binaries):
    """cape_host_shard_frame: the kept planes of a shard's frame through the host class's Polygon constructor.  The polygons equal
    those built from the same rings directly (area and vertex list bit for bit), and cape_host_match_map fed from the shard gives the
    match row it gives fed from the arrays."""
    import cape_amd as ca
    from cape_amd.dist import Shard, packed_layout

    lay = packed_layout(3, CELLS, 4, 1, polygons=True, vertices_per_frame=32)
    buf = _build_shard([0, 1, 2], 0, lay)
    sh = Shard(buf, lay)
    H = ca._host_library()
    H.cape_host_polygon_inter_area.restype = C.c_double
    H.cape_host_polygon_inter_area.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 5

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    # the map: the three kept planes of frame 2 seen before (a little smaller), in an order of its own
    rows = [row for row in _planes_of(2) if row[2] is not None]
    world = []
    for normal, d, ring, _ in (rows[2], rows[0], rows[1]):
        x, y = _frame_of(normal)
        world.append((normal, d, x, y, -d * np.asarray(normal), 0.9 * ring, []))
    M = ca.pack_map(world)
    assert [len(v) for v in ca.host_shard_frame(buf, lay, 1)] == [0, 0]  # the frame without planes
    for frame in (0, 2):
        detected, segments = ca.host_shard_frame(buf, lay, frame)
        kept = sh.kept_planes(frame)
        assert len(detected) == len(kept) == (3 if frame == 2 else 2) and list(segments) == [int(g["segment"]) for _, g, _ in kept]
        direct = []
        for (normal, d, x, y, c, ring, area, cov), (pl, g, r) in zip(detected, kept):
            # built from the same ring directly: Polygon(ring, xAxis, yAxis, center) of the host class
            a_out = C.c_double(0)
            rr, gx, gy, gc = (np.ascontiguousarray(v, np.float64) for v in (r, g["x_axis"], g["y_axis"], g["center"]))
            H.cape_host_polygon_inter_area(ptr(rr), len(rr), ptr(gx), ptr(gy), ptr(gc), ptr(rr), len(rr), ptr(gx), ptr(gy), ptr(gc),
                                           C.byref(a_out), None)
            assert np.float64(area).tobytes() == np.float64(a_out.value).tobytes() and area > 0
            assert ring.tobytes() == rr.tobytes()
            assert x.tobytes() == gx.tobytes() and y.tobytes() == gy.tobytes() and c.tobytes() == gc.tobytes()
            assert normal.tobytes() == pl["normal"].tobytes() and d == float(pl["d"])
            S = pl["sums"]
            hess = np.array([[S[3], S[6], S[8]], [S[6], S[4], S[7]], [S[8], S[7], S[5]]])
            assert np.allclose(cov @ hess, np.eye(3), atol=1e-12)  # the covariance is the inverse of the second-moment matrix
            direct.append((pl["normal"].copy(), float(pl["d"]), gx, gy, gc, rr, None))
        got = ca.host_match_map(M, [det[:7] for det in detected], flags=ca.MATCH_ALLOW_INDEX0)
        want = ca.host_match_map(M, direct, flags=ca.MATCH_ALLOW_INDEX0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if frame == 2:
            assert list(got[0]) == [2, 0, 1], got  # map plane j took the kept plane it was made from
    # a shard that dropped rings is refused: its kept-plane indices would not be the reference's
    with pytest.raises(ca.CapeError):
        ca.host_shard_frame(_build_shard([0, 1, 2], 0, lay, drop_from=10), lay, 0)
    with pytest.raises(ca.CapeError):
        ca.host_shard_frame(buf, lay, 3)  # no such frame in the shard


def test_abi_of_the_polygon_gather(hip_library):
    import re

    import cape_amd as ca

    lib = ca.load_library()
    assert lib.cape_abi_version() == ca.CAPE_ABI_VERSION == 2
    for name in ("cape_gather_configure_polygons", "cape_count_polygon_vertices"):
        assert name in ca.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ca.PACKED_POLYGON_HEADER_DTYPE.itemsize == 16 and ca.POLYGON_DTYPE.itemsize == 96
    assert C.sizeof(ca.cape_gather_polygon_layout) == 3 * 8 + 2 * 4
    assert C.sizeof(ca.cape_gather_config) == 16 and C.sizeof(ca.cape_gather_layout) == 6 * 8 + 4 * 4  # unchanged
    src = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    assert re.search(r"#define CAPE_ABI_VERSION 2\b", src)
    assert re.search(r"CAPE_GATHER_POLYGONS = 1u << 1\b", src) and ca.GATHER_POLYGONS == 2
    assert re.search(r"CAPE_PACKED_VERTICES_DROPPED = 1u << 3\b", src) and ca.PACKED_VERTICES_DROPPED == 8
    assert int(re.search(r"#define CAPE_GATHER_DEFAULT_VERTICES_PER_FRAME (\d+)", src).group(1)) == ca.GATHER_DEFAULT_VERTICES_PER_FRAME
    # argument checks that need no device: a null handle, and (through the handle-less path) nothing else to call
    assert lib.cape_gather_configure_polygons(None, None, 0, None, None) == -1
    assert lib.cape_count_polygon_vertices(None, 0, None, None) == -1
