"""bench.py end to end on the GPU box: the launcher paths the driver uses, and the in-run proof of work."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=900):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must carry exactly one JSON line, got {len(lines)}: {p.stdout[-1000:]}"
    return json.loads(lines[0])


def test_self_spawned_launcher_with_gather():
    """`python bench.py --gpus N` with no launcher around it starts its own ranks under torch.distributed.run.  One GPU
    here, so the path runs at N = 1 (--spawn) with the multi-GPU exchange forced on: native RCCL communicator, device
    packing, one collective per step, the budget measured on the stream."""
    out = _run(["--full", "--gpus", "1", "--spawn", "--steps", "3", "--warmup", "1", "--frames", "256", "--no-cpu-baseline"],
               {"CAPE_BENCH_FORCE_GATHER": "1"})
    assert out["n_gpus"] == 1 and out["steps"] == 3
    assert out["ranks"]["launcher"].startswith("self-spawned")
    assert len(out["ranks"]["ms_per_step"]) == 1
    g = out["gather"]
    assert g["ok"] and g["overflow"] == 0 and g["frames"] == 256
    assert g["path"].startswith("native")
    # first-contact evidence for an N-GPU run: what RCCL itself reports for every rank's communicator (cape_comm_info)
    assert g["native_rccl"] and not g["torch_fallback_taken"]
    assert g["rccl_ranks_seen"] == [1] and g["rccl_devices_seen"] == [[0, 0]] and g["rccl_comm"][0]["has_comm"] == 1, g
    assert g["payload_bytes_per_frame"] <= 1229, g  # <= 1.2 KB per frame on the TUM-like stream
    assert "exposed_ms_per_step" in g
    pc = out["parity_check"]
    assert pc["frames"] == 256 and pc["labels_equal"] and pc["counts_equal"] and pc["segments_bitwise"] and pc["all_ranks_ok"]


def test_gather_to_root_path():
    out = _run(["--full", "--gpus", "1", "--spawn", "--steps", "2", "--warmup", "1", "--frames", "128", "--no-cpu-baseline", "--gather-root"],
               {"CAPE_BENCH_FORCE_GATHER": "1"})
    assert out["gather"]["ok"] and "root" in out["gather"]["path"]


def test_default_workload_proves_its_work():
    """The N = 1 line (reduced batch to keep the test short): parity_check against the oracle inside the run, the
    reference-faithful cylinders-on leg next to the plane-only value."""
    out = _run(["--full", "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "512", "--no-cpu-baseline"])
    assert out["ranks"]["launcher"] == "single process"
    pc = out["parity_check"]
    assert pc["frames"] == 512 and pc["labels_equal"] and pc["segments_bitwise"] and pc["planes"] > 0
    cyl = out["cylinders_on"]
    assert cyl["value"] > 0 and cyl["parity_check"]["labels_equal"] and cyl["parity_check"]["cylinders_bitwise"]
    assert set(cyl["kernel_ms"]) == {"cape_cell_moments_kernel", "cape_cell_plane_kernel", "cape_grow_kernel"}
    assert out["roofline"]["frac"] > 0.05 and out["roofline"]["bound"] == "hbm"
    # round 6: the legs beyond the fast kernels' fixed shapes, each checked against the oracle inside the run
    b = out["beyond_fixed_capacities"]
    assert b["wide_grid"]["general_instance_frames"] == 0 and b["wide_grid"]["frames"] == 256 and b["wide_grid"]["parity_check"]["labels_equal"]
    assert b["record_chain"]["frames_of_more_than_64_segments"] == 2 and b["record_chain"]["spill_records_used"] == 2
    assert b["record_chain"]["most_segments_in_a_frame"] == 116 and b["record_chain"]["parity_check"]["segments_bitwise"]


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_two_ranks_share_the_gpu_through_gloo(scaling):
    """the N > 1 branches of bench.py (shard arithmetic, the budget all-reduce, the torch gather, max over
    ranks, per-rank parity, weak / strong stream sizes) had never run with world > 1.  CAPE_BENCH_BACKEND=gloo lets two ranks
    share the one GPU of this box (RCCL refuses that); the line is a dry run of the code paths, not a scaling number."""
    out = _run(["--full", "--gpus", "2", "--gather", "torch", "--scaling", scaling, "--steps", "3", "--warmup", "1", "--frames", "128",
                "--no-cpu-baseline"], {"CAPE_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and out["scaling"] == scaling
    total = 8 * 128 if scaling == "strong" else 2 * 128
    assert out["config"]["stream_frames"] == total and out["config"]["frames_per_step_per_gpu"] == total // 2
    assert "gloo" in out["config"]["backend"]
    assert out["ranks"]["launcher"].startswith("self-spawned") and len(out["ranks"]["ms_per_step"]) == 2
    assert out["ranks"]["ms_per_step_max"] >= out["ranks"]["ms_per_step_min"] > 0
    g = out["gather"]
    assert g["ok"] and g["frames"] == total and g["overflow"] == 0 and g["path"].startswith("torch")
    assert not g["native_rccl"] and isinstance(g["rccl_comm"], str) and "absent by design" in g["rccl_comm"]
    assert "exposed_ms_per_step" in g and g["planes"] > 0
    pc = out["parity_check"]
    assert pc["ranks_checked"] == 2 and pc["all_ranks_ok"] and pc["labels_equal"] and pc["segments_bitwise"]
    assert abs(out["value"] - total * out["steps"] / (out["ms_per_step"] * 1e-3 * out["steps"])) < 1e-6 * out["value"]
    assert "cpu_baseline" not in out and "cylinders_on" not in out  # rank 0 at N = 1 only


def test_default_line_names_the_bound_that_holds():
    """the driver-visible line says that A1 sits at about half the HBM peak AND at about its VALU-issue floor,
    with the raw-uint16 launch (half the bytes, same time) beside it."""
    out = _run(["--full", "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-polygons", "--no-parity-check"])
    r = out["roofline"]
    assert r["bound"] == "hbm" and r["kernel"] == "cape_cell_moments_kernel"
    v = r["valu_issue"]
    assert v is not None and 0.5 < v["frac_of_issue_floor"] <= 1.05, v
    assert v["f64_rate_insts_per_launch"] > v["other_valu_insts_per_launch"] * 0.5
    u = r["u16_launch"]
    assert 0.7 < u["launch_ms"] / r["launch_ms"] < 1.4, "half the bytes in about the same time"
    assert u["frac"] < 0.75 * r["frac"]


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) reports the headline and nothing that needs runs of its own; --dump-outputs writes the last timed
    step's results in float32 / float64, within 64 MB, and the same arguments give the same files."""
    import numpy as np

    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "256"]
    a = _run(args + ["--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 2 and a["unit"] == "frames/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert a["ms_per_step"] > 0 and abs(a["value"] - 256 / (a["ms_per_step"] * 1e-3)) < 1e-6 * a["value"]
    for k in ("roofline", "parity_check", "cpu_baseline", "gather", "boundary_polygons", "cylinders_on", "find_primitives_equivalent",
              "beyond_fixed_capacities"):
        assert k not in a, k
    _run(args + ["--dump-outputs", str(tmp_path / "b")])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"frames.npy", "header.npy", "plane_labels.npy", "segments.npy", "boundary_points.npy"} <= set(names)
    assert not {"cyl_labels.npy", "cylinders.npy"} & set(names), "a plane-only run hands out no cylinder outputs"
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0, n
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f"{n} differs between two runs of the same arguments"
        total += x.nbytes
    assert total <= 64 << 20
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert np.array_equal(d["frames"], np.arange(256))
    assert len(d["segments"]) == d["header"][:, 0].sum() and d["header"][:, 1].sum() > 0
    out = d["segments"][d["segments"][:, -2] == 1]  # is_output, boundary_count are the last two columns
    assert len(d["boundary_points"]) == out[:, -1].sum() > 0


def test_two_ranks_dump_their_shards_and_the_gathered_lists(tmp_path):
    """--dump-outputs at N > 1 (two ranks sharing the GPU through gloo): each rank writes its shard's results under rank<r>_, rank 0
    also the gathered primitive lists -- which hold exactly the planes the two shards report."""
    import numpy as np

    out = _run(["--gpus", "2", "--gather", "torch", "--steps", "2", "--warmup", "1", "--frames", "128", "--dump-outputs", str(tmp_path)],
               {"CAPE_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and "parity_check" not in out and "gather" not in out
    d = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in d.values()) and sum(a.nbytes for a in d.values()) <= 64 << 20
    assert {"rank0_header", "rank1_header", "rank0_plane_labels", "rank1_segments", "gathered_frames", "gathered_planes"} <= set(d)
    assert np.array_equal(d["gathered_frames"][:, 0], np.arange(256))
    per_rank = np.concatenate([d["rank0_header"][:, 1], d["rank1_header"][:, 1]])  # n_planes of frames 0..127, then 128..255
    assert np.array_equal(d["gathered_frames"][:, 3], per_rank) and len(d["gathered_planes"]) == per_rank.sum() > 0


def test_cylinder_run_dumps_its_cylinders(tmp_path):
    """--cylinders on the tunnel stream: the dump holds the cylinder label grid and one row per cylinder label of the sampled
    frames (frame, axis, radius, kept, region)."""
    import numpy as np

    _run(["--gpus", "1", "--cylinders", "--scene", "tunnel", "--steps", "1", "--warmup", "1", "--frames", "64",
          "--dump-outputs", str(tmp_path)])
    d = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert all(a.size > 0 for a in d.values())
    assert d["cyl_labels"].shape == d["plane_labels"].shape == (64, 768)
    assert d["cylinders"].shape == (d["header"][:, 2].sum(), 7) and (d["cylinders"][:, 5] == 1).any()
