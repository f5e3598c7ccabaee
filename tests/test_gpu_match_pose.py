"""cape_match_polygons_pose: MapPlane::find_matches with the camera motion between the frames (missing #2).

The reference projects the map plane and its polygon with worldToCamera BEFORE the gates (map_primitive.cpp:100-104):
PlaneWorldCoordinates::to_camera_coordinates (plane_coordinates.cpp:20-24) and WorldPolygon::to_camera_space
(polygon_coordinates.cpp:135-165).  Here the "map" is the previous frame, the pose the known relative motion of the synthetic
trajectory.  Checked three ways: bit for bit against this repo's host class (same statements), against the ORACLE of the
reference's algorithm (decisions identical, areas within 1e-9 relative), and by the property that makes a pose worth having:
on a stream whose camera moves between the frames, the true relative pose finds at least as many matches as the identity."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_pose(host_binaries):
    import cape_amd

    cape_amd.load_library()
    lib = C.CDLL(os.path.join(host_binaries, "libcape_primitives.so"))
    vp = C.c_void_p
    lib.cape_host_polygon_inter_area_pose.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.cape_host_polygon_inter_area_pose.restype = C.c_double

    def run(ring_a, pa, ring_b, pb, T, plane):
        ra, rb = np.ascontiguousarray(ring_a, np.float64), np.ascontiguousarray(ring_b, np.float64)
        arrs = [np.ascontiguousarray(pa[k], np.float64) for k in ("x_axis", "y_axis", "center")] + \
               [np.ascontiguousarray(pb[k], np.float64) for k in ("x_axis", "y_axis", "center")]
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        pin, pout = np.ascontiguousarray(plane, np.float64), np.zeros(4)
        v = lib.cape_host_polygon_inter_area_pose(ra.ctypes.data_as(vp), len(ra), *[a.ctypes.data_as(vp) for a in arrs[:3]],
                                                  rb.ctypes.data_as(vp), len(rb), *[a.ctypes.data_as(vp) for a in arrs[3:]],
                                                  T.ctypes.data_as(vp), pin.ctypes.data_as(vp), pout.ctypes.data_as(vp))
        return v, pout

    return run


@pytest.fixture(scope="module")
def P():
    import polygon_oracle_py

    polygon_oracle_py.build()
    return polygon_oracle_py


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _strided(scene, seed, start, stride, n):
    import torch
    from cape_amd import synth_gpu

    frames = [start + stride * i for i in range(n)]
    dev = torch.cat([synth_gpu.stream(scene, seed, 1, start=f, device="cuda", chunk=1) for f in frames]).contiguous()
    return dev, synth_gpu.relative_poses(scene, seed, frames)


def _kept(res, pol, f):
    from cape_amd.dist import kept_segments

    return kept_segments(res, pol, f)


def _run(scene, seed, start, stride, n, poses=True, flags=0, cyl=False):
    import torch
    from cape_amd import Extractor, synth

    intr = synth.TUM_FR1_INTRINSICS if scene == "tumlike" else synth.DEFAULT_INTRINSICS
    dev, T = _strided(scene, seed, start, stride, n)
    ex = Extractor(640, 480, cylinders=cyl, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    if poses:
        ex.match_polygons_pose(n, T, flags, st)
    else:
        ex.match_polygons(n, flags, st)
    out = ex.results(n), *ex.polygons(n), ex.polygon_matches(n), T
    ex.close()
    return out


@pytest.mark.parametrize("scene,stride,flags", [("room", 9, 0), ("tumlike", 7, 2), ("room", 25, 3)])
def test_pose_matches_equal_the_host_class_bit_for_bit(host_pose, scene, stride, flags):
    import cape_amd

    n = 20
    res, pol, ver, got, T = _run(scene, 31, 40, stride, n, flags=flags)
    min_cos = abs(math.cos(20.0 * math.pi / 180.0))
    overlap = float(np.float32(0.4)) / (2 if flags & cape_amd.MATCH_ADVANCED else 1)
    pairs = 0
    for f in range(1, n):
        g = got[f]
        prev, cur = _kept(res, pol, f - 1), _kept(res, pol, f)
        assert not (g["flags"] & cape_amd.MATCH_EXACT_OVERFLOW)
        assert list(g["seg_prev"][: len(prev)]) == prev and list(g["seg_cur"][: len(cur)]) == cur
        sp, sc = res.segments(f - 1), res.segments(f)
        matched = [False] * len(cur)
        for j, sj in enumerate(prev):
            q, pq = sp[sj], pol[f - 1, sj]
            ring_q = ver[f - 1, pq["vertex_offset"]: pq["vertex_offset"] + pq["vertex_count"]]
            selected, greatest = -1, 0.0
            for i, si in enumerate(cur):
                s, ps = sc[si], pol[f, si]
                ring_s = ver[f, ps["vertex_offset"]: ps["vertex_offset"] + ps["vertex_count"]]
                ia, plane = host_pose(ring_s, ps, ring_q, pq, T[f], list(q["out_normal"]) + [q["d"]])
                ns = s["out_normal"]
                cos = (ns[0] * plane[0] + ns[1] * plane[1]) + ns[2] * plane[2]
                gated = abs(s["d"] - plane[3]) < 100.0 and abs(cos) > min_cos
                if not gated:
                    assert g["inter_area"][j][i] == -1.0, f"frame {f} pair ({j},{i}): the device gates a pair the host rejects"
                    continue
                assert _bits(g["inter_area"][j][i]) == _bits(ia), f"frame {f} pair ({j},{i}): {g['inter_area'][j][i]!r} vs {ia!r}"
                pairs += 1
                if matched[i] or not pq["area"] > 0.0:
                    continue
                if ia > greatest and ia / ps["area"] >= overlap:
                    selected, greatest = i, ia
            if selected <= 0 and not (flags & cape_amd.MATCH_ALLOW_INDEX0):
                selected = -1
            if selected >= 0:
                matched[selected] = True
            assert g["match"][j] == selected, f"frame {f} previous plane {j}"
    assert pairs > n


def test_pose_matches_equal_the_reference_algorithm(P):
    """Decisions of cape_match_polygons_pose == MapPlane::find_matches run by the oracle (oracle polygons, oracle intersection,
    oracle to_camera_space / to_camera_coordinates); areas within 1e-9 relative."""
    import cape_amd

    n = 16
    res, pol, ver, got, T = _run("tumlike", 8, 60, 11, n, cyl=True)
    pairs = decided = 0
    kept, skip = [], set()
    for f in range(n):
        planes = []
        for i, s in enumerate(res.segments(f)):
            if not s["is_output"]:
                continue
            c0 = np.asarray(s["normal"], np.float64) * (-np.float64(s["d"]))
            ref = P.Polygon.from_points(res.boundary_points(f, s), s["normal"], c0)
            if ref.flags & P.NEEDS_DISSOLVE:
                skip.add(f)
            elif ref.valid and ref.boundary_length() >= 3:
                planes.append((i, np.asarray(s["out_normal"], np.float64), float(s["d"]), ref))
        kept.append(planes)
    for f in range(1, n):
        if f in skip or (f - 1) in skip or (got[f]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW):
            continue
        prev, cur = kept[f - 1], kept[f]
        want, inter = P.find_matches([q[1:] for q in prev], [q[1:] for q in cur], T[f])
        assert list(got[f]["match"][: len(prev)]) == want, f"frame {f}"
        decided += sum(1 for m in want if m >= 0)
        for j in range(len(prev)):
            for i in range(len(cur)):
                b = float(inter[j, i])
                if b < 0:
                    continue
                a = float(got[f]["inter_area"][j][i])
                assert a >= 0 and abs(a - b) <= 1e-9 * max(b, cur[i][3].area) + 1e-6, f"frame {f} pair ({j},{i}): {a} vs {b}"
                pairs += 1
    assert pairs >= n and decided >= n // 2


def test_true_pose_finds_at_least_the_matches_of_the_identity():
    """A camera that moves ~10 degrees / 25 cm between the frames: seen through the identity the previous planes miss the
    distance / normal gates or overlap too little; seen through the true relative pose they are found."""
    import cape_amd

    n = 24
    flags = cape_amd.MATCH_ALLOW_INDEX0
    tot = {}
    for scene, stride in (("room", 40), ("tumlike", 30)):
        _, _, _, with_pose, _ = _run(scene, 4, 10, stride, n, poses=True, flags=flags)
        _, _, _, identity, _ = _run(scene, 4, 10, stride, n, poses=False, flags=flags)
        a = int((with_pose["match"] >= 0).sum())
        b = int((identity["match"] >= 0).sum())
        prev_planes = int(with_pose["n_prev"].sum())
        tot[scene] = (a, b, prev_planes)
        assert a >= b, tot
    assert sum(v[0] for v in tot.values()) > sum(v[1] for v in tot.values()), tot
    assert sum(v[0] for v in tot.values()) >= 0.6 * sum(v[2] for v in tot.values()), tot


def test_null_pose_is_the_identity_entry_point():
    import torch
    from cape_amd import Extractor, synth, synth_gpu

    n = 8
    dev = synth_gpu.stream("room", 2, n, start=5, device="cuda", chunk=8)
    ex = Extractor(640, 480, max_batch=n, **synth.DEFAULT_INTRINSICS)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    ex.match_polygons(n, 0, st)
    a = ex.polygon_matches(n)
    ex.L.cape_match_polygons_pose(ex.h, n, None, 0, C.c_void_p(st))
    b = ex.polygon_matches(n)
    assert a.tobytes() == b.tobytes()
    eye = np.tile(np.eye(4), (n, 1, 1))
    ex.match_polygons_pose(n, eye, 0, st)
    c = ex.polygon_matches(n)
    assert np.array_equal(a["match"], c["match"])
    ex.close()
