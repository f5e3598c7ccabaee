"""cylinder_fitting at its cell-count edges and down its RANSAC branches (tests/cylinder_cases.py), on every route of the device that owns
a copy of its bookkeeping: the lone-wave code of cape_cylinder.h inside the cylinder kernel (CAPE_SCHEDULE=single), inside its RESUME
instance (CAPE_RESUME=wave) and, with 16-bit labels, inside the general instance (CAPE_GROW=general); the workgroup finisher of
cape_resume.hip (CAPE_RESUME=group); the plane pass followed by the cylinder kernel from scratch (CAPE_RESUME=off).  The twin library
built with -DCAPE_CYL_EPS=0.25 runs the same file through the ordered-sum fallback.  Everything is compared with the oracle bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import cylinder_cases as CC
from test_gpu_parity import compare_frame

pytestmark = pytest.mark.gpu

ROUTES = {
    "two-wave": {"CAPE_SCHEDULE": "two", "CAPE_RESUME": "wave"},
    "two-group": {"CAPE_SCHEDULE": "two", "CAPE_RESUME": "group"},
    "two-off": {"CAPE_SCHEDULE": "two", "CAPE_RESUME": "off"},
    "single": {"CAPE_SCHEDULE": "single"},
    "general": {"CAPE_GROW": "general"},
}
KNOBS = ("CAPE_SCHEDULE", "CAPE_RESUME", "CAPE_NO_RESUME", "CAPE_GROW")

_expected = {}


def _batch(oracle_mod, size):
    """(cases, frames, oracle results) of one size, computed once and left unchanged: every case, then the first multi-pass sheet
    again -- the same frame twice in one batch restarts the RNG and reuses the frame's scratch."""
    if size not in _expected:
        cases = CC.cases_of_size(*size)
        again = next(c for c in cases if c.name.startswith("B "))
        cases = cases + [again]
        orc = oracle_mod.Oracle(size[0], size[1], cylinders=True, **CC.intrinsics(cases[0]))
        frames = np.stack([c.build() for c in cases])
        frames.setflags(write=False)
        _expected[size] = (cases, frames, [orc.run(f) for f in frames])
    return _expected[size]


@pytest.mark.parametrize("size", CC.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("route", list(ROUTES))
def test_cylinder_edges(oracle_mod, monkeypatch, route, size):
    from cape_amd import Extractor

    cases, frames, expected = _batch(oracle_mod, size)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    ex = Extractor(size[0], size[1], cylinders=True, max_batch=len(frames), **CC.intrinsics(cases[0]))
    try:
        n = ex.extract_host(frames)
        assert n == len(frames)
        res = ex.results(n)
        if route == "general":
            assert ex.spill_info()[2] == n, "every frame went through the general instance"
        for f, (case, want) in enumerate(zip(cases, expected)):
            try:
                compare_frame(want, ex, res, f, check_cells=(route == "two-wave"))
                assert res.records["header"][f]["n_cylinder_labels"] == int(want.cyl_labels.max()), "cylinder label count"
            except AssertionError as e:
                loops = " ".join("%d/%d/%d" % (lp.m, lp.wins, lp.iterations) for lp in want.cyl_loops)
                raise AssertionError("%s (frame %d, route %s; the oracle's loops m/wins/iterations: %s): %s" % (case.name, f, route, loops, e)) from e
    finally:
        ex.close()


@pytest.mark.parametrize("size", CC.SIZES, ids=lambda s: "%dx%d" % s)
def test_cylinder_edges_ordered_sum_fallback(size):
    """test_gpu_parity.py's test_cylinder_ordered_sum_fallback on this file's cases: the twin library takes the reference's ordered sums on
    most `dist < minHypothesisDist` and `plane MSE < cylinder MSE` decisions, on every route and at every cell count."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    twin = os.path.join(root, "rgb-d-slam_amd", "lib", "libcape_hip_cyl_exact.so")
    if not os.path.exists(twin):
        subprocess.check_call(["make", "-C", os.path.join(root, "rgb-d-slam_amd", "csrc"), "variants"])
    env = dict(os.environ, CAPE_HIP_LIB=twin)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                          "test_cylinder_edges and not fallback and %dx%d" % size], env=env, capture_output=True, text=True, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "%d passed" % len(ROUTES) in out.stdout and "failed" not in out.stdout
