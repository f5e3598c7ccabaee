"""tests/host/map_step_visible_words.cpp: the ownership and word rules of cape_map_step_visible's one-frame classify kernel
(csrc/cape_map_step_visible.h) compiled for the host and driven serially as the kernel drives them -- which group, wave and round
decides which plane, which group writes which skip word, how the zero bits beyond n_map arise -- against a naive per-bit loop, on maps
of 0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023 and 1024 planes, under the address and undefined-behaviour sanitizers.  A
stand-alone executable: built with the line of the program's header comment and run directly.  CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_every_word_is_written_once_and_equals_the_naive_loop(tmp_path):
    exe = str(tmp_path / "map_step_visible_words.exe")
    build = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-Irgb-d-slam_amd/csrc",
             "-o", exe, "tests/host/map_step_visible_words.cpp"]
    with open(os.path.join(ROOT, "tests", "host", "map_step_visible_words.cpp")) as f:
        header = f.read().split("#include", 1)[0]
    for word in build[1:]:
        assert word.replace(exe, "map_step_visible_words.exe") in header, word  # the documented build line is the one that runs
    r = subprocess.run(build, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert sorted({int(v) for v in re.findall(r"^n_map +(\d+):", r.stdout, re.M)}) == SIZES
    maps, sizes = (int(v) for v in re.search(r"maps: (\d+); sizes: (\d+)", r.stdout).groups())
    assert maps == 4 * len(SIZES) and sizes == len(SIZES)
    for n, groups, words in re.findall(r"^n_map +(\d+): +(\d+) groups, +(\d+) words", r.stdout, re.M):
        assert (int(groups), int(words)) == ((int(n) + 63) // 64, (int(n) + 31) // 32), n
    assert "maps whose words differ from the naive loop or break a rule: 0" in r.stdout
    assert "FAILED" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_kernel_and_the_program_compile_the_same_rules():
    """the rules are defined once, in cape_map_step_visible.h; the kernel's file uses them and defines none of them"""
    csrc = os.path.join(ROOT, "rgb-d-slam_amd", "csrc")
    rule = open(os.path.join(csrc, "cape_map_step_visible.h")).read()
    kernel = open(os.path.join(csrc, "cape_map_visibility.hip")).read()
    for name in ("step_vis_groups", "step_vis_plane", "step_vis_slot", "step_vis_present", "step_vis_store_words"):
        assert len(re.findall(r"CAPE_STEP_VIS_FN [a-z0-9_ ]+\b" + name + r"\(", rule)) == 1, name
        assert name + "(" in kernel and "CAPE_STEP_VIS_FN" not in kernel, name
    assert '#include "cape_map_step_visible.h"' in kernel
