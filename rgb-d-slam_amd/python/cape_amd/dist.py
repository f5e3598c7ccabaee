"""Multi-GPU plumbing.  Frames shard by contiguous blocks, one process per GPU, no collective inside a
frame; once per batch the ranks all-gather their PACKED primitive lists (include/cape_hip.h: cape_packed_*), a fixed byte
count per rank.  On the GPU box the collective is ONE ncclAllGather issued by libcape_hip itself
(cape_gather_primitives, RCCL over xGMI); this module holds the host-side pieces around it: shard arithmetic, the
exchange of the communicator id, and the parser of the gathered bytes.  The CPU tests drive the same parser through a
world_size-2 gloo all-gather."""
import numpy as np


def shard_range(n_frames, rank, world):
    """Contiguous block of frames owned by `rank`: the first (n % world) ranks get one extra frame."""
    q, r = divmod(n_frames, world)
    start = rank * q + min(rank, r)
    return start, start + q + (1 if rank < r else 0)


def largest_shard(n_frames, world):
    return -(-n_frames // world)


def slot_of(shard, k, layout):
    """The slot of frame k of shard `shard` (rank order) in the arrays of Extractor.match_map_shards / shard_map_matches: a shard owns
    frames_capacity slots whatever it holds, because how many frames it holds is known on the device only."""
    F = int(layout["frames_capacity"])
    if shard < 0 or not 0 <= k < F:
        raise ValueError(f"frame {k} of shard {shard}: outside [0, {F}) frames per shard")
    return shard * F + k


def shard_of(slot, layout):
    """(shard, k) of a slot: the inverse of slot_of."""
    if slot < 0:
        raise ValueError("negative slot")
    return divmod(slot, int(layout["frames_capacity"]))


def packed_layout(frames_capacity, cells, planes_per_frame=16, cylinders_per_frame=8, labels=False, polygons=False, vertices_per_frame=0):
    """Host restatement of cape_gather_configure's layout arithmetic (sections on 16-byte boundaries).  polygons=True: that of
    cape_gather_configure_polygons -- the polygon sections behind everything else, their fields added to the dict."""
    from . import (GATHER_DEFAULT_VERTICES_PER_FRAME, PACKED_CYLINDER_DTYPE, PACKED_FRAME_DTYPE, PACKED_HEADER_DTYPE, PACKED_PLANE_DTYPE,
                   PACKED_POLYGON_HEADER_DTYPE, POLYGON_DTYPE)

    def a16(v):
        return (v + 15) & ~15

    lay = dict(frames_capacity=frames_capacity, planes_capacity=frames_capacity * planes_per_frame,
               cylinders_capacity=frames_capacity * cylinders_per_frame, cells=cells,
               plane_labels_offset=0, cyl_labels_offset=0)
    off = a16(PACKED_HEADER_DTYPE.itemsize)
    lay["frames_offset"] = off
    off = a16(off + frames_capacity * PACKED_FRAME_DTYPE.itemsize)
    lay["planes_offset"] = off
    off = a16(off + lay["planes_capacity"] * PACKED_PLANE_DTYPE.itemsize)
    lay["cylinders_offset"] = off
    off = a16(off + lay["cylinders_capacity"] * PACKED_CYLINDER_DTYPE.itemsize)
    if labels:
        lay["plane_labels_offset"] = off
        off = a16(off + frames_capacity * cells)
        lay["cyl_labels_offset"] = off
        off = a16(off + frames_capacity * cells)
    if polygons:
        lay["polygons_capacity"] = lay["planes_capacity"]
        lay["vertices_capacity"] = frames_capacity * (vertices_per_frame or GATHER_DEFAULT_VERTICES_PER_FRAME)
        lay["polygon_header_offset"] = off
        off = a16(off + PACKED_POLYGON_HEADER_DTYPE.itemsize)
        lay["polygons_offset"] = off
        off = a16(off + lay["polygons_capacity"] * POLYGON_DTYPE.itemsize)
        lay["vertices_offset"] = off
        off = a16(off + lay["vertices_capacity"] * 16)
    lay["bytes_per_rank"] = off
    return lay


class Shard:
    """One rank's packed buffer, parsed (views into the bytes, no copies)."""

    def __init__(self, buf, layout):
        from . import (GATHER_POLYGONS, PACKED_CYLINDER_DTYPE, PACKED_FRAME_DTYPE, PACKED_HEADER_DTYPE, PACKED_MAGIC, PACKED_PLANE_DTYPE,
                       PACKED_POLYGON_HEADER_DTYPE, POLYGON_DTYPE)

        buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf)
        assert buf.size == layout["bytes_per_rank"], (buf.size, layout["bytes_per_rank"])
        self.header = buf[: PACKED_HEADER_DTYPE.itemsize].view(PACKED_HEADER_DTYPE)[0]
        if int(self.header["magic"]) != PACKED_MAGIC:
            raise ValueError("not a packed cape shard (bad magic)")
        F, P, Cy = layout["frames_capacity"], layout["planes_capacity"], layout["cylinders_capacity"]
        o = layout["frames_offset"]
        self.frames = buf[o: o + F * PACKED_FRAME_DTYPE.itemsize].view(PACKED_FRAME_DTYPE)[: int(self.header["n_frames"])]
        o = layout["planes_offset"]
        self.planes = buf[o: o + P * PACKED_PLANE_DTYPE.itemsize].view(PACKED_PLANE_DTYPE)
        o = layout["cylinders_offset"]
        self.cylinders = buf[o: o + Cy * PACKED_CYLINDER_DTYPE.itemsize].view(PACKED_CYLINDER_DTYPE)
        cells = layout["cells"]
        self.plane_labels = self.cyl_labels = None
        if layout["plane_labels_offset"]:
            o = layout["plane_labels_offset"]
            self.plane_labels = buf[o: o + F * cells].reshape(F, cells)[: len(self.frames)]
            o = layout["cyl_labels_offset"]
            self.cyl_labels = buf[o: o + F * cells].reshape(F, cells)[: len(self.frames)]
        # CAPE_GATHER_POLYGONS: polygon k belongs to plane k; the rings are (x, y) pairs in the polygon's plane frame
        self.polygon_header = self.polygons = self.vertices = None
        if "polygons_offset" in layout:
            if not int(self.header["flags"]) & GATHER_POLYGONS:
                raise ValueError("the layout has polygon sections, the shard was packed without CAPE_GATHER_POLYGONS")
            o = layout["polygon_header_offset"]
            self.polygon_header = buf[o: o + PACKED_POLYGON_HEADER_DTYPE.itemsize].view(PACKED_POLYGON_HEADER_DTYPE)[0]
            o = layout["polygons_offset"]
            self.polygons = buf[o: o + layout["polygons_capacity"] * POLYGON_DTYPE.itemsize].view(POLYGON_DTYPE)
            o = layout["vertices_offset"]
            self.vertices = buf[o: o + layout["vertices_capacity"] * 16].view("<f8").reshape(-1, 2)

    @property
    def first_frame(self):
        return int(self.header["first_frame"])

    def frame_planes(self, k):
        """Planes of the shard's k-th frame (fewer than n_planes only if the header reports an overflow)."""
        fr = self.frames[k]
        a = int(fr["plane_offset"])
        b = min(a + int(fr["n_planes"]), len(self.planes))
        return self.planes[a:max(a, b)]

    def frame_cylinders(self, k):
        fr = self.frames[k]
        a = int(fr["cylinder_offset"])
        b = min(a + int(fr["n_cylinders"]), len(self.cylinders))
        return self.cylinders[a:max(a, b)]


    def frame_polygons(self, k):
        """(polygon records, [ring as an (n, 2) view]) of the shard's k-th frame, aligned with frame_planes(k).  A ring that did not
        travel (PACKED_VERTICES_DROPPED: vertex_offset = 0xFFFFFFFF) or that the producer did not build is an empty (0, 2) view."""
        if self.polygons is None:
            raise ValueError("the shard was packed without CAPE_GATHER_POLYGONS")
        fr = self.frames[k]
        a = int(fr["plane_offset"])
        b = min(a + int(fr["n_planes"]), len(self.polygons))
        pol = self.polygons[a:max(a, b)]
        rings = []
        for g in pol:
            n, o = int(g["vertex_count"]), int(g["vertex_offset"])
            if n and o + n > len(self.vertices):
                raise ValueError("a packed ring lies outside the vertex section")
            rings.append(self.vertices[o:o + n] if n else self.vertices[:0])
        return pol, rings

    def kept_planes(self, k):
        """[(plane, polygon, ring)] of the frame's planes that Primitive_Detection keeps -- CAPE_POLY_VALID and >= 3 vertices
        (primitive_detection.cpp:623-631) -- in order: entry i is plane i of the reference's plane_container, the index every matcher
        result is expressed in.  Refuses a shard that dropped planes or rings: its indices would not be the reference's."""
        from . import PACKED_PLANES_DROPPED, PACKED_VERTICES_DROPPED

        if int(self.header["overflow"]) & (PACKED_PLANES_DROPPED | PACKED_VERTICES_DROPPED):
            raise ValueError("the shard dropped planes or rings (header.overflow): the kept planes are not known")
        planes = self.frame_planes(k)
        pol, rings = self.frame_polygons(k)
        return [(planes[i], pol[i], rings[i]) for i in range(len(pol)) if polygon_is_kept(pol[i])]


def polygon_is_kept(polygon):
    """The kept-plane rule on one POLYGON_DTYPE record: Primitive_Detection keeps the plane if its polygon is CAPE_POLY_VALID with
    >= 3 vertices (primitive_detection.cpp:623-631)."""
    from . import POLY_VALID

    return bool(int(polygon["flags"]) & POLY_VALID) and int(polygon["vertex_count"]) >= 3


def kept_segments(results, polygons, f):
    """Segment indices of the planes of frame f that Primitive_Detection keeps, in order (the index every matcher result is expressed
    in counts these): results = Extractor.results(n), polygons = the records of Extractor.polygons(n)."""
    return [i for i, s in enumerate(results.segments(f)) if s["is_output"] and polygon_is_kept(polygons[f, i])]


def unpack_gathered(buf, world, layout):
    """world x bytes_per_rank gathered bytes -> list of Shard, rank order."""
    buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf).reshape(-1)
    n = layout["bytes_per_rank"]
    assert buf.size == world * n
    return [Shard(buf[r * n:(r + 1) * n], layout) for r in range(world)]


def primitives_by_frame(shards):
    """{global frame index: (planes, cylinders)} over all shards -- what one unsharded run would have produced."""
    out = {}
    for sh in shards:
        for k in range(len(sh.frames)):
            out[sh.first_frame + k] = (sh.frame_planes(k), sh.frame_cylinders(k))
    return out


def primitives_by_frame_with_polygons(shards):
    """{global frame index: (planes, cylinders, polygons, rings)} over shards packed with CAPE_GATHER_POLYGONS."""
    out = {}
    for sh in shards:
        for k in range(len(sh.frames)):
            out[sh.first_frame + k] = (sh.frame_planes(k), sh.frame_cylinders(k)) + sh.frame_polygons(k)
    return out


def broadcast_unique_id(make_id, rank, group=None, device=None):
    """Rank 0 makes the RCCL unique id (cape_comm_unique_id); every rank ends up with the same 128 bytes.
    torch.distributed is only the messenger here (any byte transport would do)."""
    import torch
    import torch.distributed as dist

    t = torch.zeros(128, dtype=torch.uint8, device=device)
    if rank == 0:
        t.copy_(torch.frombuffer(bytearray(make_id()), dtype=torch.uint8))
    dist.broadcast(t, src=0, group=group)
    return bytes(t.cpu().numpy().tobytes())


def all_gather_bytes(local, world, group=None):
    """torch.distributed all-gather of equal-sized uint8 tensors (the CPU tests' stand-in for ncclAllGather)."""
    import torch
    import torch.distributed as dist

    out = torch.empty(world * local.numel(), dtype=torch.uint8, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous().view(-1), group=group)
    return out
