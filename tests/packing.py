"""Test helper: the packed gather payload (include/cape_hip.h, cape_packed_*) built on the host from ORACLE results.
Restates what cape_pack_scan_kernel / cape_pack_copy_kernel write, so that the GPU's bytes can be compared with it and
the world_size-2 gloo test can ship real primitive lists without a GPU.

make_shard writes a shard with polygon sections by hand: the bytes cape_pack_primitives with CAPE_GATHER_POLYGONS would produce for
frames whose planes the test chooses, for tests that feed cape_match_map_shards rings no depth image would give."""
import numpy as np


def pack_oracle(results, first_frame, layout, labels=False, status=None):
    from cape_amd import (PACKED_CYLINDER_DTYPE, PACKED_FRAME_DTYPE, PACKED_HEADER_DTYPE, PACKED_MAGIC, PACKED_PLANE_DTYPE,
                          PACKED_PLANES_DROPPED, PACKED_CYLINDERS_DROPPED, GATHER_LABELS)

    buf = np.zeros(layout["bytes_per_rank"], np.uint8)
    F, P, Cy, cells = layout["frames_capacity"], layout["planes_capacity"], layout["cylinders_capacity"], layout["cells"]
    hdr = buf[: PACKED_HEADER_DTYPE.itemsize].view(PACKED_HEADER_DTYPE)
    frames = buf[layout["frames_offset"]: layout["frames_offset"] + F * PACKED_FRAME_DTYPE.itemsize].view(PACKED_FRAME_DTYPE)
    planes = buf[layout["planes_offset"]: layout["planes_offset"] + P * PACKED_PLANE_DTYPE.itemsize].view(PACKED_PLANE_DTYPE)
    cyls = buf[layout["cylinders_offset"]: layout["cylinders_offset"] + Cy * PACKED_CYLINDER_DTYPE.itemsize].view(PACKED_CYLINDER_DTYPE)
    po = co = 0
    st_or = 0
    clipped = False
    for f, r in enumerate(results):
        st = int(status[f]) if status is not None else 0
        st_or |= st & 0xFF  # flag bits only: bits 8..15 of a frame's status are a count
        frames[f] = (po, len(r.planes), co, len(r.cylinders), st, len(r.segments))
        for k in range(len(r.planes)):
            o = r.planes[k]
            if po + k < P:
                q = planes[po + k]
                q["normal"] = o[0:3]
                q["d"] = o[3]
                q["centroid"] = o[4:7]
                q["mse"] = o[7]
                q["score"] = o[8]
                seg = int(o[19])
                q["sums"] = r.segments[seg, 9:18]
                q["point_count"] = int(o[9])
                q["segment"] = seg
        for k in range(len(r.cylinders)):
            if co + k < Cy:
                cyls[co + k]["axis"] = r.cylinders[k, 0:3]
                cyls[co + k]["radius"] = r.cylinders[k, 3]
        po += len(r.planes)
        co += len(r.cylinders)
        if labels:
            o1, o2 = layout["plane_labels_offset"], layout["cyl_labels_offset"]
            # one byte per cell on the wire: a label beyond 255 reads 255 (CAPE_PACKED_LABELS_CLIPPED in the header)
            buf[o1 + f * cells: o1 + (f + 1) * cells] = np.minimum(r.plane_labels, 255).astype(np.uint8)
            buf[o2 + f * cells: o2 + (f + 1) * cells] = np.minimum(r.cyl_labels, 255).astype(np.uint8)
            clipped = clipped or len(r.segments) > 255 or int(r.cyl_labels.max(initial=0)) > 255
    hdr[0] = (PACKED_MAGIC, len(results), first_frame, po, co, P, Cy,
              (PACKED_PLANES_DROPPED if po > P else 0) | (PACKED_CYLINDERS_DROPPED if co > Cy else 0) | (4 if clipped else 0), st_or, cells, F,
              GATHER_LABELS if labels else 0)
    return buf


def ring_area(ring):
    """|ring_area_signed| in the host class's order of operations"""
    s = 0.0
    for i in range(len(ring)):
        j = i - 1 if i else len(ring) - 1
        s += (ring[j][0] * ring[i][1] - ring[i][0] * ring[j][1])
    return abs(0.5 * s), s


def clockwise(ring):
    """the ring as the polygon kernel leaves it and the host class's constructor keeps it: clockwise (a counter-clockwise one reversed)"""
    ring = np.ascontiguousarray(ring, np.float64).reshape(-1, 2)
    return ring[::-1].copy() if ring_area(ring)[1] > 0 else ring


def make_shard(cases_per_frame, layout, first_frame=0):
    """cases_per_frame: per frame the list of its detected planes, each (normal[3], d, x_axis[3], y_axis[3], center[3], ring) with the
    ring as (n, 2) plane coordinates; layout: cape_amd.dist.packed_layout(..., polygons=True) or what gather_configure returned.
    Returns the shard's bytes_per_rank bytes: header, frames, planes (segment = the plane's position in its frame, a point-cloud
    covariance of identity), polygon header, polygons (CAPE_POLY_VALID, area from the ring) and vertices (clockwise rings, back to
    back)."""
    import cape_amd as ca

    buf = np.zeros(layout["bytes_per_rank"], np.uint8)

    def section(offset, count, dtype):
        return buf[offset: offset + count * dtype.itemsize].view(dtype)

    n_frames, n_planes = len(cases_per_frame), sum(len(f) for f in cases_per_frame)
    assert n_frames <= layout["frames_capacity"] and n_planes <= layout["planes_capacity"] == layout["polygons_capacity"]
    hd = section(0, 1, ca.PACKED_HEADER_DTYPE)
    hd["magic"], hd["n_frames"], hd["first_frame"], hd["n_planes_total"] = ca.PACKED_MAGIC, n_frames, first_frame, n_planes
    hd["planes_capacity"], hd["cylinders_capacity"], hd["cells"] = layout["planes_capacity"], layout["cylinders_capacity"], layout["cells"]
    hd["frames_capacity"], hd["flags"] = layout["frames_capacity"], ca.GATHER_POLYGONS
    fr = section(layout["frames_offset"], layout["frames_capacity"], ca.PACKED_FRAME_DTYPE)
    pl = section(layout["planes_offset"], layout["planes_capacity"], ca.PACKED_PLANE_DTYPE)
    ph = section(layout["polygon_header_offset"], 1, ca.PACKED_POLYGON_HEADER_DTYPE)
    pol = section(layout["polygons_offset"], layout["polygons_capacity"], ca.POLYGON_DTYPE)
    ver = section(layout["vertices_offset"], layout["vertices_capacity"] * 2, np.dtype("<f8")).reshape(-1, 2)
    at = nv = 0
    for k, planes in enumerate(cases_per_frame):
        fr[k]["plane_offset"], fr[k]["n_planes"], fr[k]["n_plane_segments"] = at, len(planes), len(planes)
        for i, (normal, d, x_axis, y_axis, center, ring) in enumerate(planes):
            ring = clockwise(ring)
            assert len(ring) >= 3 and nv + len(ring) <= layout["vertices_capacity"]
            p, g = pl[at], pol[at]
            p["normal"], p["d"], p["centroid"], p["point_count"], p["segment"] = normal, d, center, 1000, i
            p["sums"] = [0, 0, 0, 1, 1, 1, 0, 0, 0]  # Sxs = Sys = Szs = 1: a covariance of identity
            g["x_axis"], g["y_axis"], g["center"], g["area"] = x_axis, y_axis, center, ring_area(ring)[0]
            g["vertex_offset"], g["vertex_count"], g["flags"], g["segment"] = nv, len(ring), ca.POLY_VALID, i
            ver[nv: nv + len(ring)] = ring
            at, nv = at + 1, nv + len(ring)
    ph["n_vertices_total"], ph["vertices_capacity"], ph["n_polygons_valid"] = nv, layout["vertices_capacity"], at
    return buf
