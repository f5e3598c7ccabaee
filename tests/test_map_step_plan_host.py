"""tests/host/map_step_plan.cpp: the hand-off of cape_map_step (csrc/cape_map_step.h: step_map_after) compiled for the host between the
two serial plans it joins -- commit_plan_serial, then maintain_plan_serial on the committed map, each applied as its copy kernel applies
it -- against a naive loop that appends to and then partitions a plain list, on maps of 0, 1, 255, 256, 257, 1020 and 1024 planes whose
committed counts cross 256 and reach 1024, under the address and undefined-behaviour sanitizers.  A stand-alone executable: built with
the line of the program's header comment and run directly.  CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_the_two_plans_joined_by_the_hand_off_equal_the_naive_loop(tmp_path):
    exe = str(tmp_path / "map_step_plan.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-o", exe, "tests/host/map_step_plan.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_step_plan.cpp")) as f:
        header = f.read().split("#include", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_step_plan.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    cases, refused, nothing, done, refused_maintain = (int(v) for v in re.search(
        r"cases: (\d+); commit refused (\d+), DONE \+ NOTHING (\d+), DONE \+ DONE (\d+), DONE \+ a refused maintenance (\d+)", r.stdout).groups())
    assert cases == 7 * 42 and refused + nothing + done + refused_maintain == cases
    assert min(refused, nothing, done, refused_maintain) >= 3, (refused, nothing, done, refused_maintain)  # every outcome of the table is met
    across, full = (int(v) for v in re.search(r"committed counts that cross 256: (\d+), that reach 1024 from below: (\d+)", r.stdout).groups())
    assert across >= 3 and full >= 3
    assert "cases whose step differs from the naive loop: 0" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
