"""tests/host/map_union_holes_algebra.cpp: the holes mode of csrc/cape_map_union.h one lane at a time, bit for bit against the host class
on the tables of tests/map_union_hole_cases.py and on 2 200 star pairs, under the address and undefined-behaviour sanitizers.  A
stand-alone executable: built with the line of the program's header comment and run directly.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_the_one_lane_port_equals_the_host_class(tmp_path):
    exe = str(tmp_path / "map_union_holes_algebra.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-Irgb-d-slam_amd/host", "-Irgb-d-slam_amd/host/compat", "-o", exe, "tests/host/map_union_holes_algebra.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_union_holes_algebra.cpp")) as f:
        header = f.read().split("#define main", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_union_holes_algebra.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "tables: 26 pairs" in r.stdout and "stars: 2200 pairs" in r.stdout
    assert "pairs that differ from the host class in a bit: 0" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
