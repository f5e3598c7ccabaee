"""cape_host_match_planes -- MapPlane::find_matches between two consecutive frames on the host class, with no limit on the planes
(the twin of cape_match_polygons_wide and the answer for the frames it flags) -- on hand-built polygons and against the oracle's
restatement of the reference's loop (polygon_oracle_py.find_matches); the layout of cape_frame_match_wide and the constants of the
binding against the header.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

from test_map_match_host import _config, _plane_z, _square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P(host_binaries):
    import polygon_oracle_py

    polygon_oracle_py.build()
    return polygon_oracle_py


def _twin(prev, cur, T=None, flags=0):
    import cape_amd

    return cape_amd.host_match_planes([(*q, None) for q in prev], [(*q, None) for q in cur], T, flags, areas=True)


def _oracle(P, prev, cur, T, flags):
    from cape_amd import MATCH_ADVANCED, MATCH_ALLOW_INDEX0

    mp = [(n, d, P.Polygon(ring, x, y, c)) for n, d, x, y, c, ring in prev]
    dp = [(n, d, P.Polygon(ring, x, y, c)) for n, d, x, y, c, ring in cur]
    return P.find_matches(mp, dp, T, advanced=bool(flags & MATCH_ADVANCED), allow_index0=bool(flags & MATCH_ALLOW_INDEX0))


def _on_z(ring, d=-1000.0):
    return (*_plane_z(d), ring)


def test_the_index0_quirk_and_the_flags_carried_between_previous_planes():
    far = _on_z(_square(300, 20000))
    cur = [_on_z(_square(400)), far]
    prev = [_on_z(_square(500)), _on_z(_square(500))]
    match, inter = _twin(prev, cur)
    assert inter[0, 0] == 640000.0 and list(match) == [-1, -1]  # detected plane 0 is never selected (map_primitive.cpp:146)
    match, _ = _twin(prev, cur, flags=2)
    assert list(match) == [0, -1]  # ... unless asked for; the second previous plane finds it taken
    match, inter = _twin(prev, [far, cur[0]])
    assert list(match) == [1, -1] and inter[1, 1] == 640000.0  # (the area of a taken plane is still reported)
    # the advanced search halves the overlap threshold: 0.25 of the detected plane is covered
    quarter = [_on_z(_square(500, 500, 500))]
    assert list(_twin(quarter, [far, _on_z(_square(500))])[0]) == [-1]
    assert list(_twin(quarter, [far, _on_z(_square(500))], flags=1)[0]) == [1]


def test_a_tie_goes_to_the_lowest_index():
    far = _on_z(_square(300, 20000))
    cur = [far, _on_z(_square(200, 250)), _on_z(_square(200, -250)), _on_z(_square(200, 0, 250))]
    match, inter = _twin([_on_z(_square(500))], cur)
    assert inter[0, 1] == inter[0, 2] == inter[0, 3] == 160000.0 and inter[0, 0] == 0.0
    assert list(match) == [1]
    match, _ = _twin([_on_z(_square(500))], [far, cur[3], cur[2], cur[1]])
    assert list(match) == [1]


def test_a_pair_behind_the_gates_is_not_intersected():
    far = _on_z(_square(300, 20000))
    cur = [far, _on_z(_square(400))]
    match, inter = _twin([_on_z(_square(500), d=-1150.0)], cur)  # 150 mm away
    assert list(match) == [-1] and np.all(inter == -1.0)
    n = np.array([0.0, np.sin(np.radians(25)), np.cos(np.radians(25))])  # 25 degrees off
    x, y = np.array([1.0, 0.0, 0.0]), np.cross(n, [1.0, 0.0, 0.0])
    match, inter = _twin([(n, -1000.0, x, y, 1000.0 * n, _square(500))], cur)
    assert list(match) == [-1] and np.all(inter == -1.0)


def test_the_pose_goes_on_the_plane_and_on_its_polygon(P):
    far = _on_z(_square(300, 20000), d=-1130.0)
    cur = [far, _on_z(_square(400), d=-1130.0)]
    prev = [_on_z(_square(500))]
    match, inter = _twin(prev, cur)
    assert list(match) == [-1] and inter[0, 1] == -1.0  # seen through the identity the plane is 130 mm away
    T = np.eye(4)
    T[:3, 3] = [40.0, -30.0, 130.0]  # the camera moved: the previous plane lies at z = 1130 of the new frame, its outline shifted
    match, inter = _twin(prev, cur, T)
    assert list(match) == [1] and inter[0, 1] == pytest.approx(640000.0, rel=1e-12)
    T[:3, 3] = [400.0, 0.0, 130.0]
    match, inter = _twin(prev, cur, T)
    assert inter[0, 1] == pytest.approx(500.0 * 800.0, rel=1e-12)  # the outline moved with the camera: x in [-100, 900] against [-400, 400]
    om, oi = _oracle(P, prev, cur, T, 0)
    assert list(match) == list(om) and inter[0, 1] == pytest.approx(oi[0, 1], rel=1e-9)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_twin_equals_the_oracle_on_random_frames(P, flags):
    """Decisions against find_matches on every configuration, areas where the oracle has one (it does not intersect a detected
    plane taken earlier; the twin, like the device, reports every gated pair), 1e-9 relative."""
    pairs = matches = 0
    for seed in range(10):
        rng = np.random.default_rng(2000 * flags + seed)
        T, det, maps = _config(rng, int(rng.integers(1, 65)), int(rng.integers(1, 65)))
        prev = [m[:6] for m in maps]
        match, inter = _twin(prev, det, T, flags)
        om, oi = _oracle(P, prev, det, T, flags)
        assert list(match) == list(om), f"seed {seed}: {list(match)} vs {list(om)}"
        for j, i in zip(*np.nonzero(oi >= 0)):
            assert inter[j, i] == pytest.approx(oi[j, i], rel=1e-9, abs=1e-6), (seed, j, i)
            pairs += 1
        assert np.all((inter >= 0) | (oi < 0))
        matches += sum(1 for i in match if i >= 0)
    assert pairs > 50 and matches > 10, (pairs, matches)


def test_130_planes(P):
    """More planes than any device table holds: 130 squares in a row, the previous frame's shifted by 60 mm and listed in another
    order.  Every previous plane finds its square, but the one whose square is detected plane 0."""
    rng = np.random.default_rng(3)
    n = 130
    cur = [_on_z(_square(400, 1000.0 * i)) for i in range(n)]
    order = rng.permutation(n)
    prev = [_on_z(_square(400, 1000.0 * int(k) + 60.0, 35.0)) for k in order]
    for flags in (0, 2):
        match, inter = _twin(prev, cur, None, flags)
        want = [int(k) if (k > 0 or flags & 2) else -1 for k in order]
        assert list(match) == want
        assert np.count_nonzero(inter > 0) == n and inter.shape == (n, n) and not np.any(inter == -1.0)  # one plane: every pair is gated
        assert all(inter[j, int(k)] == 740.0 * 765.0 for j, k in enumerate(order))
        om, _ = _oracle(P, prev, cur, None, flags)
        assert list(match) == list(om)


def test_argument_checks():
    import cape_amd

    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        cape_amd.host_match_planes([(*_on_z(_square(400)), None)], [(*_on_z(_square(400)), None)], None, 1 << 5)
    assert len(cape_amd.host_match_planes([], [(*_on_z(_square(400)), None)])) == 0


class _FrameMatchWide(C.Structure):
    _fields_ = [("n_prev", C.c_int32), ("n_cur", C.c_int32), ("flags", C.c_uint32), ("n_matched", C.c_int32)]


def test_wide_struct_and_constants_mirror_the_header(hip_library):
    import re

    import cape_amd

    assert cape_amd.FRAME_MATCH_WIDE_DTYPE.itemsize == C.sizeof(_FrameMatchWide) == 16
    for name, *_ in _FrameMatchWide._fields_:
        assert cape_amd.FRAME_MATCH_WIDE_DTYPE.fields[name][1] == getattr(_FrameMatchWide, name).offset, name
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    body = re.search(r"typedef struct cape_frame_match_wide\s*\{(.*?)\}\s*cape_frame_match_wide;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(u?int32_t)\s+([a-z_, ]+);", body) == [("int32_t", "n_prev, n_cur"), ("uint32_t", "flags"), ("int32_t", "n_matched")]
    assert f"#define CAPE_MATCH_WIDE_MAX_PLANES {cape_amd.MATCH_WIDE_MAX_PLANES}\n" in hdr and cape_amd.MATCH_WIDE_MAX_PLANES == 128
    for name, value in (("CAPE_MATCH_ADVANCED", cape_amd.MATCH_ADVANCED), ("CAPE_MATCH_ALLOW_INDEX0", cape_amd.MATCH_ALLOW_INDEX0),
                        ("CAPE_MATCH_MAP_AREAS", cape_amd.MATCH_MAP_AREAS), ("CAPE_MATCH_EXACT_OVERFLOW", cape_amd.MATCH_EXACT_OVERFLOW)):
        shift = int(re.search(name + r"\s*=\s*1u\s*<<\s*(\d+)", hdr).group(1))
        assert value == 1 << shift, name
    lib = cape_amd.load_library()
    assert hasattr(lib, "cape_match_polygons_wide") and hasattr(lib, "cape_copy_polygon_matches_wide")
    # argument checks that need no device
    assert lib.cape_match_polygons_wide(None, 1, None, 0, None) == -1
    assert lib.cape_copy_polygon_matches_wide(None, 1, None, None, None, None, None) == -1
