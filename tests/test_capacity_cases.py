"""The generators of tests/capacity_cases.py meet their targets EXACTLY, on the CPU oracle: the conditions under which
tests/test_gpu_capacity_edges.py puts a frame at a table's last slot, or one past it.  A target that cannot be met is replaced here
(another tile, seed or drop order) -- never skipped or widened on the GPU."""
import numpy as np
import pytest

import capacity_cases as K

MAX_BOUNDARY = 256  # the small instance of the device polygon kernel: every plane of these frames stays inside it


def _check(n_planes, depth, intr, res):
    import polygon_oracle_py as P

    P.build()
    assert len(res.segments) == n_planes, "plane segments"
    assert len(res.planes) == n_planes, "output planes"
    assert len(set(res.merge_labels.tolist())) == n_planes, "distinct merge labels: no two segments merge"
    assert len(res.boundary) == n_planes
    for k in range(n_planes):
        normal, d = res.planes[k][0:3], res.planes[k][3]
        pts = res.boundary[k]
        assert 3 <= len(pts) <= MAX_BOUNDARY, f"plane {k}: {len(pts)} boundary candidates"
        # Plane_Segment::get_center(): normal * (-d), the origin the reference gives its polygons
        pol = P.Polygon.from_points(pts, normal, normal * (-d))
        assert not pol.threw and pol.valid and pol.is_valid(), f"plane {k}: polygon not valid (flags {pol.flags})"
        assert not pol.flags & (P.NEEDS_DISSOLVE | P.HULL_FAILED), f"plane {k}: flags {pol.flags}"
        assert len(pol.ring) >= 3 and pol.area > 0.0, f"plane {k}: degenerate polygon"  # -> a kept plane
    assert intr == K._intr(depth.shape[1])
    assert not depth.flags.writeable, "the cached frame is shared between tests"


@pytest.mark.parametrize("case", K.CHECKER_CASES, ids=lambda c: "-".join(map(str, c)))
def test_checkerboard_counts(oracle_mod, case):
    _check(case[0], *K.checker_with(*case))
    # the extraction tests run with the cylinder branch too: the same count, no cylinder
    with_cyl = K.checker_oracle(*case, True)
    assert len(with_cyl.segments) == len(with_cyl.planes) == case[0] and len(with_cyl.cylinders) == 0


@pytest.mark.parametrize("case", K.LATTICE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_lattice_counts(oracle_mod, case):
    n, W, H, a, b = case
    depth, intr, res = K.lattice_with(*case)
    _check(n, depth, intr, res)
    # coplanar: every pair of these planes passes the matchers' gates (angle under 20 degrees, distance under 100 mm)
    normals, d = res.planes[:, 0:3], res.planes[:, 3]
    assert np.abs(normals @ normals.T).min() > np.cos(np.radians(20.0)) and np.ptp(np.abs(d)) < 100.0


def test_generators_are_deterministic_and_refuse_what_they_cannot_meet(oracle_mod):
    a = K.checker_with(16, 640, 480, 80)
    K.checker_with.cache_clear()
    b = K.checker_with(16, 640, 480, 80)
    assert a[0] is not b[0] and a[0].tobytes() == b[0].tobytes()
    assert a[2].segments.tobytes() == b[2].segments.tobytes()
    with pytest.raises(K.CapacityCaseError):
        K.checker_with(49, 640, 480, 80)  # the whole checkerboard has 48
    with pytest.raises(K.CapacityCaseError):
        K.lattice_with(104, 1280, 960, 4, 5)  # 104 panes, 103 segments
