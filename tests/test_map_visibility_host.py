"""cape_host_map_visibility: MapPlane::is_visible for one frame on the host class (the twin of cape_map_visibility, without its
bounding-box shortcut).  Its decisions are compared with the polygon oracle's rings_inter_area(screen ring, rectangle) > 0 on screen
rings restated here in numpy, case by case; no case is left out.  The cases are shared with tests/test_gpu_map_visibility.py."""
import ctypes as C
import math

import numpy as np
import pytest

W, H = 640, 480
INTR = dict(fx=550.0, fy=550.0, cx=320.0, cy=240.0)
Z0 = 1000.0  # depth of the fronto-parallel case planes (mm)


def _fronto(uv, holes=(), intr=INTR, z=Z0):
    """the map plane Z = z (axes X, Y) whose outer ring lands on the screen polygon `uv` under the identity pose"""
    def back(r):
        r = np.asarray(r, np.float64).reshape(-1, 2)
        return np.stack([(r[:, 0] - intr["cx"]) * z / intr["fx"], (r[:, 1] - intr["cy"]) * z / intr["fy"]], 1)

    return (np.array([0.0, 0.0, 1.0]), -z, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, z]), back(uv),
            [back(h) for h in holes])


def _box(u0, u1, v0, v1):
    return np.array([[u0, v0], [u1, v0], [u1, v1], [u0, v1]], np.float64)


def _ngon(cu, cv, r, k):
    a = 0.1 + np.linspace(0, 2 * math.pi, k, endpoint=False)
    return np.stack([cu + r * np.cos(a), cv + r * np.sin(a)], 1)


def _through_axis(ring, cy_mm):
    """a plane that contains the camera's viewing direction (axes X and Z, at height Y = cy_mm): ring (a, b) -> (a, cy_mm, 500 + b)"""
    return (np.array([0.0, -1.0, 0.0]), float(cy_mm), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([0.0, float(cy_mm), 500.0]),
            np.asarray(ring, np.float64), [])


# (name, map plane, visible under the identity pose or None where only the twin defines it, compared with the oracle under every pose)
HAND_CASES = [
    ("inside", _fronto(_box(200, 400, 150, 300)), True, True),
    ("outside left", _fronto(_box(-300, -100, 100, 300)), False, True),
    ("outside right", _fronto(_box(800, 1000, 100, 300)), False, True),
    ("outside above", _fronto(_box(200, 400, -300, -100)), False, True),
    ("outside below", _fronto(_box(200, 400, 600, 800)), False, True),
    # its bounding box [-200, 100]^2 covers the corner (1, 1); its long edge u + v = -100 passes 72 px outside it
    ("thin triangle across a corner", _fronto([[-200, 100], [100, -200], [-60, -60]]), False, True),
    ("contains the screen", _fronto(_box(-500, 1200, -500, 1000)), True, True),
    ("straddles the left edge", _fronto(_box(-100, 100, 100, 300)), True, True),
    ("hole around the screen", _fronto(_box(-600, 1300, -600, 1100), holes=[_box(-500, 1200, -500, 1000)]), True, True),
    # one vertex at exactly Z = 0: (100, 200, 0) -> u, v infinite; (0, 0, 0) -> NaN
    # (planes through the camera: under the identity pose only -- from elsewhere the second one is seen edge-on, a sliver of no area)
    ("vertex at Z = 0 beside the axis", _through_axis([[100, -500], [100, 500], [-100, 500]], 200.0), False, False),
    ("vertex at the optical centre", _through_axis([[0, -500], [100, 500], [-100, 500]], 0.0), False, False),
]
# rings in every capacity tier, straddling the left edge
GON_CASES = [(f"{k}-gon", _fronto(_ngon(1.0, 240.0, 100.0, k)), True, True) for k in (4, 33, 129, 512)]
# behind the camera: a floor (Y = 300 mm) from Z = -2000 to 5000, and a quad entirely at Z < 0 -- the twin's answer, whatever it is
BEHIND_CASES = [
    ("floor through the camera", _through_axis([[-1500, -2500], [1500, -2500], [1500, 4500], [-1500, 4500]], 300.0), None, False),
    ("quad behind the camera", _through_axis([[-1500, -2500], [1500, -2500], [1500, -1000], [-1500, -1000]], 300.0), None, False),
]


def generated_cases(count, seed=3):
    """fronto-parallel boxes on the grid of screen coordinates = 5 mod 10: an edge is never within 4 px of a rectangle edge (1, 639,
    479), so a box overlaps the rectangle by at least 4 x 4 px or not at all"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        u0, v0 = 10 * int(rng.integers(-60, 100)) + 5, 10 * int(rng.integers(-60, 90)) + 5
        out.append((f"generated {k}", _fronto(_box(u0, u0 + 10 * int(rng.integers(1, 60)), v0, v0 + 10 * int(rng.integers(1, 60)))), None, True))
    return out


def all_cases(n_map):
    cases = HAND_CASES + GON_CASES + BEHIND_CASES
    return cases + generated_cases(n_map - len(cases))


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    i, j = [k for k in range(3) if k != axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def poses():
    """five world-to-camera poses: the identity, then pans, a roll and translations that move walls off the screen"""
    out = [np.eye(4)]
    for R, t in ((_rot(1, 25.0), [0, 0, 0]), (_rot(0, -18.0), [150, -40, 0]), (_rot(2, 30.0) @ _rot(1, -35.0), [0, 0, 200]), (np.eye(3), [600, 300, -400])):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        out.append(T)
    return out


def screen_ring(plane, T, intr=INTR):
    """steps 1-3 of the visibility test restated in numpy (float64, one operation at a time): the outer ring through to_camera_space
    (polygon_coordinates.cpp:135-162), get_point_from_plane_coordinates and to_screen_coordinates (point_coordinates.cpp:203)"""
    _, _, x, y, c, ring, _ = plane
    R, t = T[:3, :3], T[:3, 3]
    nc = R @ c + t
    nx, ny = R @ x, R @ y
    nx, ny = nx / np.linalg.norm(nx), ny / np.linalg.norm(ny)
    out = []
    for a, b in np.asarray(ring, np.float64):
        d = (R @ (c + a * x + b * y) + t) - nc
        qa, qb = float(nx @ d), float(ny @ d)
        X, Y, Z = nc + qa * nx + qb * ny
        with np.errstate(all="ignore"):
            inv = np.float64(1.0) / Z
            out.append((inv * (intr["fx"] * X + intr["cx"] * Z), inv * (intr["fy"] * Y + intr["cy"] * Z)))
    return np.array(out, np.float64)


def min_depth(plane, T):
    """the smallest camera Z of the outer ring's vertices: a ring that reaches Z < 0 has a screen image that may cross itself, where
    the twin alone defines the answer"""
    _, _, x, y, c, ring, _ = plane
    return min(float((T[:3, :3] @ (c + a * x + b * y) + T[:3, 3])[2]) for a, b in np.asarray(ring, np.float64))


def _clockwise(ring):
    x, y = ring[:, 0], ring[:, 1]
    return (ring[::-1] if np.sum(np.roll(x, 1) * y - x * np.roll(y, 1)) > 0 else ring).copy()


def oracle_visible(plane, T, intr=INTR, width=W, height=H):
    """(visible, area): a non-finite screen coordinate is not visible, else the oracle's area of (screen ring n rectangle) > 0"""
    import polygon_oracle_py as P

    P.build()
    uv = screen_ring(plane, T, intr)
    if not np.all(np.isfinite(uv)):
        return False, 0.0
    rect = np.array([[1, 1], [width - 1, 1], [width - 1, height - 1], [1, height - 1]], np.float64)
    area = P.rings_inter_area(_clockwise(uv), _clockwise(rect))
    return area > 0, area


def bits(words, n):
    return [bool((int(words[j >> 5]) >> (j & 31)) & 1) for j in range(n)]


@pytest.fixture(scope="module")
def cape(hip_library):
    import cape_amd

    return cape_amd


def _twin(cape, planes, T, moving=None, intr=INTR):
    return cape.host_map_visibility(cape.pack_map(planes), T, W, H, intr["fx"], intr["fy"], intr["cx"], intr["cy"], moving)


def test_hand_built_cases_under_the_identity_pose(cape):
    cases = HAND_CASES + GON_CASES
    words = _twin(cape, [c[1] for c in cases], None)
    skipped = bits(words, len(cases))
    for j, (name, plane, visible, _) in enumerate(cases):
        want, area = oracle_visible(plane, np.eye(4))
        print(f"{name}: oracle area {area!r}, twin {'skips' if skipped[j] else 'visits'}")
        assert not 0 < area <= 1, f"{name}: an oracle area of {area} px^2 is no test case"
        assert want == visible, name
        assert skipped[j] == (not visible), name


def test_every_case_and_pose_against_the_oracle(cape):
    cases = all_cases(70)
    planes = [c[1] for c in cases]
    for f, T in enumerate(poses()):
        skipped = bits(_twin(cape, planes, T), len(cases))
        n_visible = compared = 0
        for j, (name, plane, _, with_oracle) in enumerate(cases):
            if not with_oracle or min_depth(plane, T) < 0:
                continue  # (a ring behind the camera, by construction or under this pose: defined by the twin alone; the planes through
                          # the camera are compared under the identity pose, in the test above)
            want, area = oracle_visible(plane, T)
            assert not 0 < area <= 1, f"pose {f}, {name}: an oracle area of {area} px^2 is no test case"
            assert skipped[j] == (not want), f"pose {f}, {name}: oracle area {area}"
            n_visible += want
            compared += 1
        assert 5 < n_visible < compared - 5, f"pose {f} decides nothing"


def test_moving_planes_are_skipped_and_tail_bits_are_zero(cape):
    cases = all_cases(37)
    planes = [c[1] for c in cases]
    plain = _twin(cape, planes, None)
    assert len(plain) == 2 and plain[1] >> 5 == 0  # n_map = 37: bits 37 .. 63 are 0
    moving = np.array([0x00000181, 0x00000010], np.uint32)  # planes 0, 7, 8 (0, 7 and 8 are visible) and 36
    assert not bits(plain, 37)[0] and not bits(plain, 37)[7] and not bits(plain, 37)[8]
    got = _twin(cape, planes, None, moving)
    assert np.array_equal(got, plain | moving) and got[1] >> 5 == 0
    assert bits(got, 37)[0] and bits(got, 37)[7] and bits(got, 37)[8] and bits(got, 37)[36]


def test_map_and_camera_moved_together_decide_the_same(cape):
    """exact only where no operation rounds differently: integer ring coordinates, a translation by powers of two, no rotation"""
    rng = np.random.default_rng(9)
    planes = []
    for _ in range(24):
        a0, b0 = int(rng.integers(-1500, 1000)), int(rng.integers(-1200, 800))
        ring = np.array([[a0, b0], [a0 + int(rng.integers(40, 900)), b0], [a0 + 300, b0 + int(rng.integers(40, 900))]], np.float64)
        planes.append((np.array([0.0, 0.0, 1.0]), -1024.0, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1024.0]), ring, []))
    shift = np.array([1024.0, -2048.0, 4096.0])
    moved = [(n, d - shift[2], x, y, c + shift, ring, holes) for n, d, x, y, c, ring, holes in planes]
    T = np.eye(4)
    T[:3, 3] = -shift
    here, there = _twin(cape, planes, None), _twin(cape, moved, T)
    assert np.array_equal(here, there)
    assert 0 < sum(bits(here, len(planes))) < len(planes)


def test_argument_checks(cape):
    from cape_amd import _host_library, _map_arrays

    L = _host_library()
    planes = [c[1] for c in HAND_CASES[:3]]
    arrays, view = _map_arrays(cape.pack_map(planes))
    out = np.full(1, 0xFFFFFFFF, np.uint32)
    call = lambda m, w, h, o: L.cape_host_map_visibility(m, None, w, h, 550.0, 550.0, 320.0, 240.0, None, o)  # noqa: E731
    po = out.ctypes.data_as(C.POINTER(C.c_uint32))
    assert call(None, W, H, po) == -1
    assert call(C.byref(view), W, H, None) == -1
    assert call(C.byref(view), 2, H, po) == -1 and call(C.byref(view), W, 2, po) == -1
    P, R, V = cape.pack_map(planes)
    R["vertex_count"][1] = 2  # a ring of 2 vertices
    with pytest.raises(cape.CapeError, match=r"\(-1\)"):
        cape.host_map_visibility((P, R, V), None, W, H, **INTR)
    assert out[0] == 0xFFFFFFFF  # nothing was written
    assert call(C.byref(view), W, H, po) == 0 and out[0] == 0b110
    with pytest.raises(cape.CapeError):
        cape.host_map_visibility(cape.pack_map(planes), None, W, H, moving=np.zeros(2, np.uint32), **INTR)
    assert len(cape.host_map_visibility(cape.pack_map([]), None, W, H, **INTR)) == 0  # an empty map
