"""tests/host/map_work_layout.cpp: the work layouts of the map's entry points (csrc/cape_api_map.h) compiled for the host against
the offsets recorded from the three layout functions they replace, at batch sizes 1, 2 and 4 096, capacities 1, 255, 256, 257 and
kMapWorkMax and 0, 1 and 2 mask words -- every section 256-byte aligned, in the documented order, not overlapping the next -- under
the address and undefined-behaviour sanitizers.  A stand-alone executable: built with the line of the program's header comment and
run directly.  CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgb-d-slam_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_every_offset_is_the_recorded_one(tmp_path):
    exe = str(tmp_path / "map_work_layout.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Itests/host/hip_stub", "-Irgb-d-slam_amd/csrc",
             "-o", exe, "tests/host/map_work_layout.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_work_layout.cpp")) as f:
        header = f.read().split("#include", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_work_layout.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    rows, n_map, n_wide, n_vis = (int(v) for v in re.search(r"rows: (\d+) \(map (\d+), wide (\d+), visibility (\d+)\)", r.stdout).groups())
    assert (n_map, n_wide, n_vis) == (3 * 5 * 3, 3 * 5, 5) and rows == n_map + n_wide + n_vis  # batches x capacities x mask words
    assert "offsets that differ from the recorded ones or break a rule: 0" in r.stdout
    assert "FAILED" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_layouts_have_one_definition():
    """cape_api_map.h defines the two layouts; no API file defines one of its own, and the three that use them include the header"""
    header = open(os.path.join(CSRC, "cape_api_map.h")).read()
    for name in ("map_work_layout", "visibility_work_layout"):
        assert len(re.findall(r"WorkLayout " + name + r"\(", header)) == 1, name
    for name in sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")):
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"WorkLayout \w+_work_layout\(", text), name
        if "_work_layout(" in text:
            assert '#include "cape_api_map.h"' in text, name
