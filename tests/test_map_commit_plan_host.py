"""tests/host/map_commit_plan.cpp: the plan of cape_map_commit (csrc/cape_map_commit.h: the per-plane decisions and the serial scan over
them) compiled for the host, against a naive loop on maps of 0, 1, 255, 256, 257 and 1024 planes, under the address and
undefined-behaviour sanitizers.  A stand-alone executable: built with the line of the program's header comment and run directly.  CPU
only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_the_serial_plan_equals_the_naive_loop(tmp_path):
    exe = str(tmp_path / "map_commit_plan.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-o", exe, "tests/host/map_commit_plan.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_commit_plan.cpp")) as f:
        header = f.read().split("#include", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_commit_plan.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    frames, done = (int(v) for v in re.search(r"frames: (\d+), of them DONE: (\d+)", r.stdout).groups())
    assert frames == 6 * 40 + 5 and done >= 60
    refused = [int(v) for v in re.search(r"FRAME_OVERFLOW (\d+), BAD_POSE_COV (\d+), HOST_PAIR (\d+), FAIL_POLYGON (\d+), CAPACITY (\d+)", r.stdout).groups()]
    assert min(refused) >= 10, refused  # every refusal cause is met
    assert "frames whose plan differs from the naive loop: 0" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
