"""tests/host/map_union_cut_algebra.cpp: the cut mode of csrc/cape_map_union.h one lane at a time, bit for bit against the host class on
the table of tests/map_union_cut_cases.py and on the 2 200 star pairs of the holes mode's port (142 of them partly covered), under the
address and undefined-behaviour sanitizers.  A stand-alone executable: built with the line of the program's header comment and run
directly.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_the_one_lane_port_equals_the_host_class(tmp_path):
    exe = str(tmp_path / "map_union_cut_algebra.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-Irgb-d-slam_amd/host", "-Irgb-d-slam_amd/host/compat", "-o", exe, "tests/host/map_union_cut_algebra.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_union_cut_algebra.cpp")) as f:
        header = f.read().split("#define main", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_union_cut_algebra.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    # the table: the port hands away the one row named for it (the second arrangement's node limit) and nothing else
    assert "table: 21 pairs; served without / with pieces 2 / 16, capacity 2, handed away by the port alone 1" in r.stdout
    # the stars: every pair the host class serves is served, none trips the guard band of the second walk
    assert "stars: 2200 pairs; served without / with pieces 2058 / 142, capacity 0, handed away by the port alone 0" in r.stdout
    assert "pairs that differ from the host class in a bit: 0" in r.stdout
    assert "HANDED AWAY" not in r.stdout and "DIFFERS" not in r.stdout and "OUTCOME" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
