"""CAPE_GATHER_POLYGONS on the device: the packed buffer of a rank carries, for every packed plane, the cape_polygon and the ring
that cape_build_polygons built -- bit for bit what cape_copy_polygons / cape_copy_spill_polygons show for the same segment, so the
expected value is the existing device path and there is no tolerance anywhere in this file.  Everything goes through the C ABI
(the ctypes binding), on the scene generators of tests/test_gpu_gather.py.

The two-process test starts this file as its own worker (`python test_gpu_gather_polygons.py --worker ...`), each child under a
`timeout` of its own."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY_FIELDS = ("x_axis", "y_axis", "center", "area", "vertex_count", "flags")  # everything but vertex_offset and segment
NO_RING = 0xFFFFFFFF


def _mixed(n, seed=2):
    """room / tunnel frames in turn (host rendered, 640 x 480)"""
    from cape_amd import synth

    return np.stack([synth.tunnel(seed=seed, frame=f) if f % 4 == 3 else synth.room(seed=seed, frame=f) for f in range(n)])


def _mixed_device(n, seed=41):
    """the same mix rendered on the device: three room frames, then a tunnel frame"""
    import torch
    from cape_amd import synth_gpu

    room = synth_gpu.stream("room", seed, n, start=0, device="cuda", chunk=64)
    tun = synth_gpu.stream("tunnel", seed, n, start=0, device="cuda", chunk=64)
    pick = (torch.arange(n, device="cuda") % 4 == 3).view(n, 1, 1)
    return torch.where(pick, tun, room).contiguous()


def _unpacked(ex, n):
    """[[(segment index in the frame's list, polygon record, ring)] per frame] for the output planes of the last batch, from
    cape_copy_results + cape_copy_polygons + cape_copy_spill_polygons: the path that exists without the gather."""
    res = ex.results(n, with_boundary=False)
    pol, ver = ex.polygons(n)
    spol = sver = None
    if res.spill_records is not None:
        spol, sver = ex.spill_polygons(0, len(res.spill_records))
    out = []
    for f in range(n):
        rows = []
        rec, P, V = res.records[f], pol[f], ver[f]
        while True:
            hdr = rec["header"]
            base = int(hdr["segment_base"])
            for i in np.flatnonzero(rec["segments"]["is_output"][: min(64, int(hdr["n_plane_segments"]))]):
                o, c = int(P[i]["vertex_offset"]), int(P[i]["vertex_count"])
                rows.append((base + int(i), P[i], V[o:o + c]))
            nxt = int(hdr["next_record"])
            if nxt < ex.max_batch:
                break
            rec, P, V = res.spill_records[nxt - ex.max_batch], spol[nxt - ex.max_batch], sver[nxt - ex.max_batch]
        out.append(rows)
    return out


def _same_polygon(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in POLY_FIELDS)


def _assert_shard_equals_unpacked(sh, want, first=0):
    """every frame, every packed plane: polygon fields and ring bit for bit; returns (planes, vertices) compared"""
    n_planes = n_vertices = 0
    for k in range(len(sh.frames)):
        planes = sh.frame_planes(k)
        pol, rings = sh.frame_polygons(k)
        rows = want[first + k]
        assert len(planes) == len(pol) == len(rings) == len(rows) == int(sh.frames[k]["n_planes"]), (k, len(pol), len(rows))
        for i, (seg, g, ring) in enumerate(rows):
            assert int(pol[i]["segment"]) == seg == int(planes[i]["segment"]), (k, i)
            assert _same_polygon(pol[i], g), (k, i, pol[i], g)
            assert rings[i].tobytes() == np.ascontiguousarray(ring).tobytes(), (k, i)
            n_vertices += len(ring)
        n_planes += len(rows)
    return n_planes, n_vertices


def _setup(n, width=640, height=480, intr=None, cylinders=True, **gather):
    from cape_amd import Extractor, synth

    intr = dict(intr or synth.DEFAULT_INTRINSICS)
    ex = Extractor(width, height, cylinders=cylinders, max_batch=n, **intr)
    lay = ex.gather_configure(n, **gather)
    return ex, lay


def test_packed_polygons_equal_the_unpacked_path():
    """A few hundred mixed room / tunnel frames: every packed polygon and ring against cape_copy_polygons of the same batch."""
    import torch
    from cape_amd import GATHER_LABELS, GATHER_POLYGONS, POLY_VALID
    from cape_amd.dist import Shard, packed_layout

    n = 320
    dev = _mixed_device(n)
    ex, lay = _setup(n, labels=True, polygons=True, vertices_per_frame=0)
    assert lay == packed_layout(n, ex.cells, 16, 8, labels=True, polygons=True)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    ex.pack(n, first_frame=7, stream=st)
    sh = Shard(ex.packed_host(), lay)
    want = _unpacked(ex, n)
    assert int(sh.header["overflow"]) == 0 and int(sh.header["flags"]) == GATHER_LABELS | GATHER_POLYGONS and sh.first_frame == 7
    n_planes, n_vertices = _assert_shard_equals_unpacked(sh, want)
    assert n_planes == int(sh.header["n_planes_total"]) > n and n_vertices > 3 * n
    total, most = ex.count_polygon_vertices(n)
    assert int(sh.polygon_header["n_vertices_total"]) == total == n_vertices
    assert most == max(sum(len(r) for _, _, r in rows) for rows in want)
    assert int(sh.polygon_header["vertices_capacity"]) == lay["vertices_capacity"]
    kept = sum(1 for rows in want for _, g, r in rows if int(g["flags"]) & POLY_VALID and len(r) >= 3)
    assert int(sh.polygon_header["n_polygons_valid"]) == kept == sum(len(sh.kept_planes(k)) for k in range(n))
    # rings lie in plane order without gaps, each on a 16-byte boundary by construction (pairs of doubles)
    at = 0
    for g in sh.polygons[:n_planes]:
        if int(g["vertex_count"]):
            assert int(g["vertex_offset"]) == at
            at += int(g["vertex_count"])
    assert at == total
    ex.close()


def test_flag_clear_is_todays_buffer_and_flag_set_extends_it():
    """Flag clear: bytes and layout of a handle that was given the flag before equal those of a handle that never was.  Flag set: the
    first bytes_per_rank(flag clear) bytes are the flag-clear buffer except header.flags and bit 3 of header.overflow."""
    from cape_amd import GATHER_POLYGONS, PACKED_HEADER_DTYPE, PACKED_VERTICES_DROPPED
    from cape_amd.dist import packed_layout

    n = 24
    frames = _mixed(n)
    plain, lay0 = _setup(n, labels=True)
    assert lay0 == packed_layout(n, plain.cells, 16, 8, labels=True) and "polygons_offset" not in lay0
    plain.extract_host(frames)
    plain.pack(n, first_frame=3)
    base = plain.packed_host()
    ex, lay1 = _setup(n, labels=True, polygons=True, vertices_per_frame=2)  # (2 per frame: rings are dropped, bit 3 is set)
    for key, val in lay0.items():
        assert lay1[key] == val or key == "bytes_per_rank"
    assert lay1["polygon_header_offset"] == lay0["bytes_per_rank"] and lay1["bytes_per_rank"] > lay0["bytes_per_rank"]
    assert all(lay1[k] % 16 == 0 for k in ("polygon_header_offset", "polygons_offset", "vertices_offset", "bytes_per_rank"))
    ex.extract_host(frames)
    ex.build_polygons(n)
    ex.pack(n, first_frame=3)
    got = ex.packed_host()
    hd0 = base[:48].view(PACKED_HEADER_DTYPE)[0]
    hd1 = got[:48].copy().view(PACKED_HEADER_DTYPE)[0]
    assert int(hd1["flags"]) == int(hd0["flags"]) | GATHER_POLYGONS
    assert int(hd1["overflow"]) == int(hd0["overflow"]) | PACKED_VERTICES_DROPPED
    head = got[: lay0["bytes_per_rank"]].copy()
    head[:48].view(PACKED_HEADER_DTYPE)["flags"] = hd0["flags"]
    head[:48].view(PACKED_HEADER_DTYPE)["overflow"] = hd0["overflow"]
    assert np.array_equal(head, base), "the sections that exist without the flag changed"
    # the same handle configured back without the flag: today's layout, today's bytes
    lay2 = ex.gather_configure(n, labels=True)
    assert lay2 == lay0
    ex.pack(n, first_frame=3)
    assert np.array_equal(ex.packed_host(), base)
    ex.close()
    plain.close()


def test_polygons_of_a_chained_frame():
    """A frame of 116 plane segments continues in a spill record: the polygons of the planes of that record arrive behind those of
    the first with their frame-wide segment index, their rings equal to cape_copy_spill_polygons."""
    from cape_amd import Extractor, synth
    from cape_amd.dist import Shard
    from test_gpu_parity import _checkerboard_of_facets

    W, H = 1280, 960
    big, intr = _checkerboard_of_facets(W, H)
    frames = np.stack([synth.room(seed=1, frame=0, width=W, height=H, intr=intr), big,
                       synth.tunnel(seed=1, frame=0, width=W, height=H, intr=intr), big])
    n = len(frames)
    ex = Extractor(W, H, cylinders=True, max_batch=n, **intr)
    lay = ex.gather_configure(n, 80, 8, labels=True, polygons=True, vertices_per_frame=ex.boundary_capacity)
    ex.extract_host(frames)
    ex.build_polygons(n)
    ex.pack(n, first_frame=8)
    sh = Shard(ex.packed_host(), lay)
    want = _unpacked(ex, n)
    assert int(sh.header["overflow"]) == 0
    assert len(want[1]) > 64 and max(seg for seg, _, _ in want[1]) >= 64, "the generator no longer fills a spill record"
    assert sum(len(r) for seg, _, r in want[1] if seg >= 64) > 0
    _assert_shard_equals_unpacked(sh, want)
    total, most = ex.count_polygon_vertices(n)  # (follows the chain)
    assert total == sum(len(r) for rows in want for _, _, r in rows) == int(sh.polygon_header["n_vertices_total"])
    assert most == sum(len(r) for _, _, r in want[1])
    ex.close()


@pytest.mark.parametrize("vertices_per_frame", [1, 2])
def test_vertex_overflow_ships_the_longest_prefix(vertices_per_frame):
    """A budget of one or two vertices per frame: the header says so, the total is the true one, and the rings that travel are
    exactly the longest prefix in packed-plane order whose vertices fit -- each complete, the others with count 0 / offset ~0."""
    from cape_amd import PACKED_VERTICES_DROPPED
    from cape_amd.dist import Shard

    n = 48
    frames = _mixed(n, seed=5)
    ex, lay = _setup(n, polygons=True, vertices_per_frame=vertices_per_frame)
    cap = lay["vertices_capacity"]
    assert cap == n * vertices_per_frame
    ex.extract_host(frames)
    ex.build_polygons(n)
    ex.pack(n)
    sh = Shard(ex.packed_host(), lay)
    want = [row for rows in _unpacked(ex, n) for row in rows]
    total = sum(len(r) for _, _, r in want)
    assert total == ex.count_polygon_vertices(n)[0] == int(sh.polygon_header["n_vertices_total"]) > cap
    assert int(sh.header["overflow"]) == PACKED_VERTICES_DROPPED
    assert len(want) == int(sh.header["n_planes_total"]) <= lay["planes_capacity"]
    at, shipped, open_prefix = 0, 0, True
    for k, (seg, g, ring) in enumerate(want):
        p = sh.polygons[k]
        assert all(p[f].tobytes() == g[f].tobytes() for f in POLY_FIELDS if f != "vertex_count") and int(p["segment"]) == seg
        open_prefix = open_prefix and at + len(ring) <= cap
        if len(ring) == 0:
            assert int(p["vertex_count"]) == 0 and int(p["vertex_offset"]) == 0
        elif open_prefix:
            assert int(p["vertex_count"]) == len(ring) and int(p["vertex_offset"]) == at
            assert sh.vertices[at:at + len(ring)].tobytes() == np.ascontiguousarray(ring).tobytes()
            at += len(ring)
            shipped += 1
        else:
            assert int(p["vertex_count"]) == 0 and int(p["vertex_offset"]) == NO_RING
    assert shipped >= 1 and at <= cap and not sh.vertices[at:].any()
    with pytest.raises(ValueError):
        sh.kept_planes(0)
    # the bound the header states: boundary_capacity vertices per frame never overflow for unchained frames
    lay = ex.gather_configure(n, polygons=True, vertices_per_frame=ex.boundary_capacity)
    ex.pack(n)
    assert int(Shard(ex.packed_host(), lay).header["overflow"]) == 0
    ex.close()


def test_wire_bytes_depend_on_the_frames_only():
    """A large batch, then a smaller one into the same slots, then the smaller one on a fresh handle: equal bytes."""
    n, m = 40, 13
    frames = _mixed(n, seed=9)
    ex, lay = _setup(n, labels=True, polygons=True, vertices_per_frame=96)
    for _ in range(2):  # both staging slots hold the large batch
        ex.extract_host(frames)
        ex.build_polygons(n)
        ex.pack(n)
    assert ex.packed_host().any()
    reused = []
    for _ in range(2):
        ex.extract_host(frames[:m])
        ex.build_polygons(m)
        ex.pack(m, first_frame=4)
        reused.append(ex.packed_host())
    ex.close()
    fresh, lay2 = _setup(n, labels=True, polygons=True, vertices_per_frame=96)
    assert lay2 == lay
    fresh.extract_host(frames[:m])
    fresh.build_polygons(m)
    fresh.pack(m, first_frame=4)
    want = fresh.packed_host()
    fresh.close()
    assert np.array_equal(reused[0], want) and np.array_equal(reused[1], want)


def test_preconditions_and_argument_checks():
    import ctypes as C

    import cape_amd
    from cape_amd import CapeError

    n = 6
    frames = _mixed(n)
    ex, lay = _setup(n, polygons=True)
    assert lay["vertices_capacity"] == n * cape_amd.GATHER_DEFAULT_VERTICES_PER_FRAME and lay["polygons_capacity"] == lay["planes_capacity"]
    ex.extract_host(frames)
    before = ex.packed_host()
    with pytest.raises(CapeError, match=r"\(-4\).*cape_build_polygons"):  # CAPE_ERR_CAPACITY: no polygons of this batch yet
        ex.pack(n)
    assert np.array_equal(ex.packed_host(), before), "a refused pack wrote something"
    with pytest.raises(CapeError, match=r"\(-4\).*cape_build_polygons"):
        ex.count_polygon_vertices(n)
    ex.build_polygons(n - 2)
    with pytest.raises(CapeError, match=r"\(-4\).*cape_build_polygons"):  # fewer frames built than packed
        ex.pack(n)
    ex.pack(n - 2)
    ex.extract_host(frames)  # a new batch: the polygons on the device are the previous batch's
    with pytest.raises(CapeError, match=r"\(-4\).*cape_build_polygons"):
        ex.pack(1)
    # plain cape_gather_configure with the flag = the default budget; unknown bits and a negative budget are rejected
    L = ex.L
    out = cape_amd.cape_gather_layout()
    cfg = cape_amd.cape_gather_config(n, 0, 0, cape_amd.GATHER_POLYGONS)
    assert L.cape_gather_configure(ex.h, C.byref(cfg), C.byref(out)) == 0 and out.bytes_per_rank == lay["bytes_per_rank"]
    for bad in (1 << 2, cape_amd.GATHER_POLYGONS | 1 << 5):
        cfg = cape_amd.cape_gather_config(n, 0, 0, bad)
        assert L.cape_gather_configure(ex.h, C.byref(cfg), None) == -1
        assert L.cape_gather_configure_polygons(ex.h, C.byref(cfg), 0, None, None) == -1
    cfg = cape_amd.cape_gather_config(n, 0, 0, 0)
    assert L.cape_gather_configure_polygons(ex.h, C.byref(cfg), -1, None, None) == -1
    assert L.cape_gather_configure_polygons(ex.h, C.byref(cfg), 1 << 30, None, None) == -1  # n x 2^30 does not fit an int32
    pl = cape_amd.cape_gather_polygon_layout()
    assert L.cape_gather_configure_polygons(ex.h, C.byref(cfg), 5, C.byref(out), C.byref(pl)) == 0  # (flag implied)
    assert pl.vertices_capacity == 5 * n and pl.polygons_capacity == out.planes_capacity and pl.vertices_offset % 16 == 0
    ex.close()


def test_native_rccl_gather_with_polygons():
    """cape_gather_primitives at world 1 through librccl: the larger bytes_per_rank is all the collective needs to know."""
    import torch
    from cape_amd.dist import primitives_by_frame_with_polygons, unpack_gathered

    n = 8
    frames = _mixed(n, seed=5)
    ex, lay = _setup(n, labels=True, polygons=True, vertices_per_frame=128)
    ex.comm_init(ex.comm_unique_id(), 0, 1)
    recv = torch.zeros(lay["bytes_per_rank"], dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for rep in range(3):  # both staging slots get reused
        ex.extract_host(frames, stream)
        if rep == 0:
            with pytest.raises(Exception, match="cape_build_polygons"):
                ex.gather(n, 0, recv.data_ptr(), stream)
        ex.build_polygons(n, stream)
        ex.gather(n, 0, recv.data_ptr(), stream)
    ex.gather_wait(host_sync=True)
    got = recv.cpu().numpy()
    assert np.array_equal(got, ex.packed_host()), "gathered bytes differ from the packed staging slot"
    shards = unpack_gathered(got, 1, lay)
    assert int(shards[0].header["overflow"]) == 0
    want = _unpacked(ex, n)
    _assert_shard_equals_unpacked(shards[0], want)
    by_frame = primitives_by_frame_with_polygons(shards)
    assert sorted(by_frame) == list(range(n)) and all(len(v) == 4 and len(v[0]) == len(v[2]) == len(v[3]) for v in by_frame.values())
    ex.comm_destroy()
    ex.close()


def _kept_blobs(sh, k):
    """the kept planes of a shard's frame as bytes: plane record, polygon fields, ring"""
    return [pl.tobytes() + b"".join(g[f].tobytes() for f in POLY_FIELDS) + np.ascontiguousarray(r).tobytes() for pl, g, r in sh.kept_planes(k)]


def _worker(rank, world, port, n_frames, out_path):
    for p in (os.path.join(ROOT, "rgb-d-slam_amd", "python"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cape_amd import Extractor, synth
    from cape_amd.dist import all_gather_bytes, largest_shard, shard_range, unpack_gathered

    intr = dict(synth.DEFAULT_INTRINSICS)
    a, b = shard_range(n_frames, rank, world)
    frames = _mixed(n_frames)
    cap = largest_shard(n_frames, world)
    ex = Extractor(640, 480, cylinders=True, device=0, max_batch=cap, **intr)
    lay = ex.gather_configure(cap, 16, 8, labels=True, polygons=True, vertices_per_frame=160)
    ex.extract_host(frames[a:b])
    ex.build_polygons(b - a)
    ex.pack(b - a, first_frame=a)
    local = torch.from_numpy(ex.packed_host().copy())  # the device-packed shard of THIS process
    shards = unpack_gathered(all_gather_bytes(local, world).numpy(), world, lay)
    blobs = {}
    for sh in shards:
        for k in range(len(sh.frames)):
            blobs[sh.first_frame + k] = _kept_blobs(sh, k)
    ex.close()
    dist.barrier()
    dist.destroy_process_group()
    with open(out_path, "wb") as fh:
        pickle.dump(blobs, fh)


def test_two_process_sharded_gather_with_polygons_on_one_gpu(tmp_path):
    """Two processes shard an 11-frame stream (6 + 5), pack their shards with polygons on the device and all-gather the bytes
    (gloo: RCCL refuses two ranks on one GPU).  Shard.kept_planes of the assembled batch -- the reference's plane_container of
    every frame, polygons included -- equal those of one handle that ran the whole batch."""
    from cape_amd.dist import Shard

    n, world = 11, 2
    port = 29950 + os.getpid() % 40
    outs = [str(tmp_path / f"rank{r}.pkl") for r in range(world)]
    # the ranks meet in the all-gather, so both run at once; each under its own time limit, and nothing else runs on the GPU
    # before both have ended with status 0
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--worker", str(r), str(world),
                               str(port), str(n), outs[r]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0] * world, "\n".join(log[-1500:] for log in logs)
    gathered = [pickle.load(open(o, "rb")) for o in outs]
    assert gathered[0] == gathered[1] and sorted(gathered[0]) == list(range(n))
    ex, lay = _setup(n, labels=True, polygons=True, vertices_per_frame=160)
    ex.extract_host(_mixed(n))
    ex.build_polygons(n)
    ex.pack(n)
    whole = Shard(ex.packed_host(), lay)
    ex.close()
    assert sum(len(_kept_blobs(whole, k)) for k in range(n)) > n
    for k in range(n):
        assert gathered[0][k] == _kept_blobs(whole, k), f"frame {k}: kept planes of the sharded run differ from the single handle's"


def test_full_size_room_batch_every_frame():
    """The 4 096-frame room batch of BASELINE.json configs[1] (planes only): every frame, every packed plane."""
    import torch
    from cape_amd import Extractor, synth_gpu
    from cape_amd.dist import Shard
    from test_gpu_parity import _intr

    n = 4096
    intr = _intr("room", 1.0)
    dev = synth_gpu.stream("room", 100, n, width=640, height=480, start=0, device="cuda", chunk=64)
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    n_pl, _, _ = ex.count_primitives(n)
    total, most = ex.count_polygon_vertices(n)
    lay = ex.gather_configure(n, planes_per_frame=int(np.ceil(1.25 * n_pl / n)) + 1, polygons=True,
                              vertices_per_frame=int(np.ceil(1.25 * total / n)) + 1)
    ex.pack(n, stream=st)
    sh = Shard(ex.packed_host(), lay)
    assert int(sh.header["overflow"]) == 0 and int(sh.header["n_frames"]) == n
    n_planes, n_vertices = _assert_shard_equals_unpacked(sh, _unpacked(ex, n))
    assert n_planes == n_pl and n_vertices == total and most <= ex.boundary_capacity
    ex.close()


if __name__ == "__main__":
    assert sys.argv[1] == "--worker"
    _worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
