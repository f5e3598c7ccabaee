"""tests/host/pose_score_pairs.cpp: the pair list of cape_map_pose_score (csrc/cape_pose_score.h: the map planes in ascending order
whose match names a kept plane) compiled for the host, its serial statement against the pairs kernel's chunked ballot compaction
restated lane by lane, on maps of 0, 1, 63, 64, 65, 128, 1023 and 1024 planes with 0, 1, 64, 65 and 128 pairs, under the address and
undefined-behaviour sanitizers.  A stand-alone executable: built with the line of the program's header comment and run directly.
CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_the_serial_pair_list_equals_the_kernels_compaction(tmp_path):
    exe = str(tmp_path / "pose_score_pairs.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-o", exe, "tests/host/pose_score_pairs.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "pose_score_pairs.cpp")) as f:
        header = f.read().split("#include", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "pose_score_pairs.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    frames, full, overflow = (int(v) for v in re.search(r"frames: (\d+); with 128 pairs: (\d+); with more than 128: (\d+)", r.stdout).groups())
    # sizes 0: {0}; 1, 63: {0, 1}; 64: {0, 1, 64}; 65: {0, 1, 64, 65}; 128, 1023, 1024: all five -- four frames each
    assert frames == 4 * (1 + 2 + 2 + 3 + 4 + 5 + 5 + 5) and full == 4 * 3 and overflow == 6
    for n_map in (0, 1, 63, 64, 65, 128, 1023, 1024):
        assert re.search(rf"n_map +{n_map}: ", r.stdout), n_map
    for pairs in (0, 1, 64, 65, 128):
        assert re.search(rf": +{pairs} pairs made, +{pairs} listed", r.stdout), pairs
    assert "frames whose kernel list differs from the serial one or breaks a rule: 0" in r.stdout
    assert "FAILED" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
