"""cape_map_pose_score's ABI without a device: the declarations of include/cape_hip.h and host/cape_host_map.h, the exported symbols and
their ctypes signatures, the layouts of cape_pose_score and cape_pose_feature against the numpy dtypes (compiled and measured, not
restated), the flag constants, the thresholds of the rules header, and the argument checks that run before the device probe."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(*path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, *path)).read(), flags=re.S)


def test_declarations_symbols_and_signatures(hip_library, host_binaries):
    import cape_amd

    public = _header("include", "cape_hip.h")
    want = {
        "cape_map_pose_score": r"int cape_map_pose_score\(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double\* world_to_camera, "
                               r"uint32_t flags, void\* stream\);",
        "cape_copy_pose_scores": r"int cape_copy_pose_scores\(cape_handle h, int32_t n_frames, cape_pose_score\* scores, cape_pose_feature\* features, "
                                 r"double\* residuals\);",
        "cape_pose_score_device": r"int cape_pose_score_device\(cape_handle h, const cape_pose_score\*\* scores, const cape_pose_feature\*\* features\);",
    }
    for name, pattern in want.items():
        assert re.search(pattern, public), f"{name} is not declared as the issue states it"
        assert name in cape_amd.EXPORTED_SYMBOLS
    host = re.sub(r"\s+", " ", _header("rgb-d-slam_amd", "host", "cape_host_map.h"))
    assert re.search(r"int cape_host_pose_score\(const cape_host_map\* map, const int32_t\* match, const cape_host_planes\* detected, uint32_t "
                     r"frame_flags, int32_t n_hypotheses, const double\* world_to_camera, cape_pose_score\* scores_out, cape_pose_feature\* "
                     r"features_out, double\* residuals_out\);", host)
    L = cape_amd.load_library()
    vp = C.c_void_p
    assert L.cape_map_pose_score.argtypes == [vp, C.c_int32, C.c_int32, vp, C.c_uint32, vp]
    assert L.cape_copy_pose_scores.argtypes == [vp, C.c_int32, vp, vp, vp]
    assert L.cape_pose_score_device.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    H = cape_amd._host_library()
    assert len(H.cape_host_pose_score.argtypes) == 9
    for name in ("map_pose_score", "pose_scores", "pose_features"):
        assert callable(getattr(cape_amd.Extractor, name))
    assert callable(cape_amd.host_pose_score)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_struct_layouts_match_the_dtypes(tmp_path):
    import cape_amd

    fields = {"cape_pose_score": ["n_pairs", "n_inliers", "n_invalid", "flags", "score", "sum_sq", "inlier_words"],
              "cape_pose_feature": ["matched", "map_plane", "stddev", "map_id", "map_index", "kept_plane"]}
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "cape_hip.h"', "int main() {"]
    for struct, names in fields.items():
        lines.append(f'  std::printf("{struct} %zu\\n", sizeof({struct}));')
        for name in names:
            lines.append(f'  std::printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));')
    lines += ['  std::printf("flags %u %u %u %u\\n", (unsigned)CAPE_POSE_SCORE_DEVICE_POSES, (unsigned)CAPE_POSE_SCORE_RESIDUALS, '
              "(unsigned)CAPE_POSE_SCORE_INVALID_FEATURE, (unsigned)CAPE_MATCH_EXACT_OVERFLOW);", "  return 0;", "}"]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout.exe")
    r = subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()
               if not line.startswith("flags"))
    flags = subprocess.run([exe], capture_output=True, text=True).stdout.splitlines()[-1].split()[1:]
    for struct, dtype in (("cape_pose_score", cape_amd.POSE_SCORE_DTYPE), ("cape_pose_feature", cape_amd.POSE_FEATURE_DTYPE)):
        assert int(out[struct]) == dtype.itemsize, struct
        assert list(dtype.names) == fields[struct]
        for name in fields[struct]:
            assert int(out[f"{struct}.{name}"]) == dtype.fields[name][1], f"{struct}.{name}"
    assert cape_amd.POSE_SCORE_DTYPE.itemsize == 48 and cape_amd.POSE_FEATURE_DTYPE.itemsize == 112
    assert [int(v) for v in flags] == [cape_amd.POSE_SCORE_DEVICE_POSES, cape_amd.POSE_SCORE_RESIDUALS, cape_amd.POSE_SCORE_INVALID_FEATURE,
                                       cape_amd.MATCH_EXACT_OVERFLOW] == [1, 2, 256, 1]
    # the row's flags share a word with the wide match's: the new bit is none of an existing enum's
    assert cape_amd.POSE_SCORE_INVALID_FEATURE & (cape_amd.MATCH_EXACT_OVERFLOW | 2 | 8) == 0


def test_thresholds_of_the_rules_header_are_the_references_floats():
    src = open(os.path.join(ROOT, "rgb-d-slam_amd", "csrc", "cape_pose_score.h")).read()
    assert re.search(r"constexpr float kPoseInlierAngleThreshold = 0\.2f;", src)
    assert re.search(r"constexpr float kPoseInlierDistanceThreshold = 50\.0f;", src)
    # ... and they are compared as doubles widened from those floats, nowhere as double literals
    assert "static_cast<double>(kPoseInlierAngleThreshold)" in src and "static_cast<double>(kPoseInlierDistanceThreshold)" in src
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"<= *0\.2\b|<= *50\.0\b", code)


def test_argument_checks_before_the_device_probe(hip_library):
    import numpy as np

    import cape_amd

    L = cape_amd.load_library()
    poses = np.tile(np.eye(4), (1, 1, 1, 1))
    p = poses.ctypes.data_as(C.c_void_p)
    assert L.cape_map_pose_score(None, 1, 1, p, 0, None) == -1 and b"null handle" in L.cape_last_error()
    assert L.cape_map_pose_score(None, 1, 0, p, 0, None) == -1 and b"n_hypotheses" in L.cape_last_error()
    assert L.cape_map_pose_score(None, 1, -3, p, 0, None) == -1 and b"n_hypotheses" in L.cape_last_error()
    assert L.cape_map_pose_score(None, 1, 1, p, 1 << 2, None) == -1 and b"unknown pose-score flag" in L.cape_last_error()
    assert L.cape_map_pose_score(None, 1, 1, p, 1 << 8, None) == -1 and b"unknown pose-score flag" in L.cape_last_error()
    assert L.cape_copy_pose_scores(None, 1, None, None, None) == -1
    out = C.c_void_p()
    assert L.cape_pose_score_device(None, C.byref(out), None) == -1
