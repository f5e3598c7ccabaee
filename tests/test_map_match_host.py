"""cape_host_match_map -- MapPlane::find_matches over a persistent map on the host class (the twin of cape_match_map and the answer
for the frames the device flags) -- against the oracle's restatement of Feature_Map::get_matches (polygon_oracle_py.find_matches),
plus the semantics of the map order, the skip bits and the holes.  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def P(host_binaries):
    import polygon_oracle_py

    polygon_oracle_py.build()
    return polygon_oracle_py


def _axes(n):
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(n, a)
    x /= np.linalg.norm(x)
    y = np.cross(n, x)
    return x, y / np.linalg.norm(y)


def _rot(rng, max_angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    t = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * K @ K


def _star(rng, r, n):
    """a simple ring (vertices in angle order around the origin), clockwise like every polygon the product stores"""
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    rad = r * rng.uniform(0.6, 1.0, n)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    x, y = ring[:, 0], ring[:, 1]
    signed = 0.5 * np.sum(np.roll(x, 1) * y - x * np.roll(y, 1))
    return (ring[::-1] if signed > 0 else ring).copy()


def _config(rng, n_map, n_det):
    """Random detected planes in camera coordinates and map planes in world coordinates near them, with a random rigid pose."""
    R, t = _rot(rng, math.pi), rng.uniform(-2000, 2000, 3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    det = []
    for _ in range(n_det):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        d = rng.uniform(-3000, -500)
        x, y = _axes(n)
        det.append((n, d, x, y, -d * n, _star(rng, rng.uniform(200, 900), int(rng.integers(3, 20)))))
    maps = []
    for _ in range(n_map):
        n, d, x, y, c, ring = det[int(rng.integers(n_det))]
        # the plane slightly tilted and moved, the outline shifted / scaled in it: some pairs pass the gates, some do not
        Rp = _rot(rng, math.radians(25))
        nc = Rp @ n
        nc /= np.linalg.norm(nc)
        cc = c + nc * rng.uniform(-150, 150) + x * rng.uniform(-400, 400) + y * rng.uniform(-400, 400)
        xc = Rp @ x
        xc /= np.linalg.norm(xc)
        yc = np.cross(nc, xc)
        yc /= np.linalg.norm(yc)
        mring = ring * rng.uniform(0.5, 1.5) if rng.uniform() < 0.7 else _star(rng, rng.uniform(200, 900), int(rng.integers(3, 30)))
        # to world: p_w = R^T (p_c - t)
        nw, cw, xw, yw = R.T @ nc, R.T @ (cc - t), R.T @ xc, R.T @ yc
        maps.append((nw, float(-(nw @ cw)), xw, yw, cw, mring, []))
    return T, det, maps


def _oracle(P, T, det, maps, flags):
    from cape_amd import MATCH_ADVANCED, MATCH_ALLOW_INDEX0

    mp = [(n, d, P.Polygon(ring, x, y, c)) for n, d, x, y, c, ring, _ in maps]
    dp = [(n, d, P.Polygon(ring, x, y, c)) for n, d, x, y, c, ring in det]
    return P.find_matches(mp, dp, T, advanced=bool(flags & MATCH_ADVANCED), allow_index0=bool(flags & MATCH_ALLOW_INDEX0))


def _twin(T, det, maps, flags, skip=None):
    import cape_amd

    return cape_amd.host_match_map(cape_amd.pack_map(maps), [(n, d, x, y, c, r, None) for n, d, x, y, c, r in det], T, skip, flags,
                                   areas=True)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_twin_equals_the_oracle_on_random_maps(P, flags):
    """Decisions: against find_matches, every configuration.  Areas: against the oracle's find_matches table where it has one,
    and for the pairs it does not intersect (a detected plane taken earlier) against its own steps -- to_camera_space, project
    into the detected frame, intersection of the rings -- 1e-9 relative."""
    pairs = matches = 0
    for seed in range(12):
        rng = np.random.default_rng(1000 * flags + seed)
        T, det, maps = _config(rng, int(rng.integers(1, 65)), int(rng.integers(1, 65)))
        match, map_of, inter = _twin(T, det, maps, flags)
        om, oi = _oracle(P, T, det, maps, flags)
        for j, i in enumerate(match):
            if i >= 0:
                assert map_of[i] == j
        assert sorted(i for i in map_of if i >= 0) == sorted(j for j, i in enumerate(match) if i >= 0)
        assert list(match) == list(om), f"seed {seed}: {list(match)} vs {list(om)}"
        for j in range(len(maps)):
            n, d, x, y, c, ring, _ = maps[j]
            proj = P.Polygon(ring, x, y, c).to_camera_space(T)
            for i in range(len(det)):
                if inter[j, i] < 0:
                    continue
                _, _, dx, dy, dc, dring = det[i]
                want = P.rings_inter_area(dring, proj.project(dx, dy, dc).ring)
                assert inter[j, i] == pytest.approx(want, rel=1e-9, abs=1e-6), (seed, j, i)
                if oi[j, i] >= 0:
                    assert inter[j, i] == pytest.approx(oi[j, i], rel=1e-9, abs=1e-6), (seed, j, i)
                pairs += 1
            assert all(inter[j, i] >= 0 for i in range(len(det)) if oi[j, i] >= 0)
        matches += sum(1 for i in match if i >= 0)
    assert pairs > 50 and matches > 10, (pairs, matches)


def _square(h, cx=0.0, cy=0.0):
    return np.array([[cx - h, cy - h], [cx - h, cy + h], [cx + h, cy + h], [cx + h, cy - h]])


def _plane_z(d=-1000.0):
    n = np.array([0.0, 0.0, 1.0])
    return n, d, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), -d * n


def test_hole_over_the_detected_plane_gives_zero(P):
    n, d, x, y, c = _plane_z()
    maps = [(n, d, x, y, c, _square(1000), [_square(500)])]
    det = [(n, d, x, y, c, _square(2000, 9000)), (n, d, x, y, c, _square(500))]
    match, map_of, inter = _twin(None, det, maps, 2)
    assert inter[0, 1] == 0.0 and match[0] == -1 and map_of[1] == -1
    # without the hole the same detected plane is covered and taken
    match, _, inter = _twin(None, det, [(n, d, x, y, c, _square(1000), [])], 2)
    assert inter[0, 1] == pytest.approx(1e6, rel=1e-12) and match[0] == 1


def test_holes_subtract_in_order_against_the_oracle_rings(P):
    rng = np.random.default_rng(7)
    n, d, x, y, c = _plane_z()
    checked = 0
    for _ in range(30):
        outer = _star(rng, 1500, int(rng.integers(8, 40)))
        holes = [_square(rng.uniform(50, 200), *rng.uniform(-500, 500, 2)) for _ in range(int(rng.integers(1, 4)))]
        det_ring = _star(rng, 1000, int(rng.integers(3, 30))) + rng.uniform(-300, 300, 2)
        match, _, inter = _twin(None, [(n, d, x, y, c, det_ring)], [(n, d, x, y, c, outer, holes)], 2)
        want = P.rings_inter_area(det_ring, outer)
        for h in holes:
            want -= P.rings_inter_area(det_ring, h[::-1].copy())
        want = max(want, 0.0)
        assert inter[0, 0] == pytest.approx(want, rel=1e-9, abs=1e-6)
        checked += 1
    assert checked == 30


def test_map_order_skip_bits_and_the_index0_quirk():
    n, d, x, y, c = _plane_z()
    far = (n, d, x, y, c, _square(300, 20000))
    det = [far, (n, d, x, y, c, _square(400))]
    twin = (n, d, x, y, c, _square(500), [])
    match, map_of, _ = _twin(None, det, [twin, twin], 0)
    assert list(match) == [1, -1] and list(map_of) == [-1, 0]  # the first map plane takes it, the second finds it taken
    match, map_of, _ = _twin(None, det, [twin, twin], 0, skip=np.array([1], np.uint32))
    assert list(match) == [-1, 1] and list(map_of) == [-1, 1]  # map plane 0 is not visited
    # the `selectedIndex <= 0` quirk: detected plane 0 is never selected unless ALLOW_INDEX0
    match, _, inter = _twin(None, det[1:], [twin], 0)
    assert inter[0, 0] > 0 and list(match) == [-1]
    match, map_of, _ = _twin(None, det[1:], [twin], 2)
    assert list(match) == [0] and list(map_of) == [0]
    # a map plane behind the gates: 150 mm away
    match, _, inter = _twin(None, det, [(n, d + 150.0, x, y, c, _square(500), [])], 2)
    assert list(match) == [-1] and inter[0, 1] == -1.0


class _MapPlane(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("d", C.c_double), ("x_axis", C.c_double * 3), ("y_axis", C.c_double * 3),
                ("center", C.c_double * 3), ("ring_first", C.c_uint32), ("ring_count", C.c_uint32)]


class _MapRing(C.Structure):
    _fields_ = [("vertex_offset", C.c_uint32), ("vertex_count", C.c_uint32)]


class _FrameMapMatch(C.Structure):
    _fields_ = [("n_map", C.c_int32), ("n_cur", C.c_int32), ("flags", C.c_uint32), ("n_matched", C.c_int32),
                ("seg_cur", C.c_int32 * 64), ("map_of", C.c_int32 * 64)]


def test_map_dtypes_mirror_the_header():
    import cape_amd

    assert cape_amd.MAP_PLANE_DTYPE.itemsize == C.sizeof(_MapPlane) == 112
    assert cape_amd.MAP_RING_DTYPE.itemsize == C.sizeof(_MapRing) == 8
    assert cape_amd.FRAME_MAP_MATCH_DTYPE.itemsize == C.sizeof(_FrameMapMatch) == 528
    for dt, st in ((cape_amd.MAP_PLANE_DTYPE, _MapPlane), (cape_amd.FRAME_MAP_MATCH_DTYPE, _FrameMapMatch)):
        for name, *_ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "cape_hip.h")).read()
    assert "#define CAPE_MAP_MAX_PLANES 1024" in hdr and "#define CAPE_MAP_MAX_RING 512" in hdr and "#define CAPE_MAP_MAX_HOLES 8" in hdr
    assert (cape_amd.MAP_MAX_PLANES, cape_amd.MAP_MAX_RING, cape_amd.MAP_MAX_HOLES, cape_amd.MATCH_MAP_AREAS) == (1024, 512, 8, 4)
