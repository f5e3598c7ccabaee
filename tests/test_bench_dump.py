"""bench.py --dump-outputs, without a GPU: the helpers that turn a batch's results into float arrays, on a hand-made batch."""
import numpy as np

import bench
import cape_amd
from cape_amd import dist


def _batch(n, max_batch=None, cylinder=False):
    """n frames: frame f holds f % 3 plane segments (every other one an output plane with f + 1 boundary points, written in
    reverse order); frame 1 continues in a spill record of two more segments; with `cylinder`, frame 0 holds one cylinder."""
    max_batch = max_batch or n
    rec = np.zeros(n, cape_amd.FRAME_RECORD_DTYPE)
    cells = 12
    bcap = 16
    bd = np.zeros((n, bcap, 3))
    for f in range(n):
        k = f % 3
        rec["header"]["n_plane_segments"][f] = k
        rec["header"]["n_planes"][f] = (k + 1) // 2
        rec["header"]["next_record"][f] = -1
        for s in range(k):
            seg = rec["segments"][f, s]
            seg["normal"] = (0.0, 0.0, 1.0)
            seg["d"] = -1000.0 - f - s
            seg["is_output"] = s % 2 == 0
            seg["boundary_offset"] = 8 * s
            seg["boundary_count"] = f % 8 + 1 if s % 2 == 0 else 0
            pts = np.stack([np.arange(f % 8 + 1)[::-1], np.full(f % 8 + 1, s), np.full(f % 8 + 1, f)], axis=1).astype(float)
            bd[f, 8 * s: 8 * s + len(pts)] = pts if s % 2 == 0 else 0
    if cylinder:
        rec["header"]["n_cylinder_labels"][0] = rec["header"]["n_cylinders"][0] = 1
        rec["cylinders"]["axis"][0, 0] = (1.0, 0.0, 0.0)
        rec["cylinders"]["kept"][0, 0] = 1
    spill = np.zeros(1, cape_amd.FRAME_RECORD_DTYPE)
    sbd = np.zeros((1, bcap, 3))
    if n > 1:
        rec["header"]["next_record"][1] = max_batch
        spill["header"]["n_plane_segments"][0] = 2
        spill["header"]["next_record"][0] = -1
        spill["segments"]["d"][0, :2] = (-7.0, -8.0)
        spill["segments"]["is_output"][0, :2] = 1
        spill["segments"]["boundary_count"][0, :2] = (1, 0)
        sbd[0, 0] = (5.0, 6.0, 7.0)
    labels = np.arange(n * cells, dtype=np.int32).reshape(n, cells) % 5
    return cape_amd.FrameResults(rec, labels, labels * 0, bd, max_batch, spill, sbd)


def test_batch_outputs_follow_chains_and_sort_boundary_points():
    res = _batch(6)
    d = bench._batch_outputs(res, None, np.arange(6))
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d["plane_labels"].shape == (6, 12) and d["plane_labels"].dtype == np.float32
    assert d["header"].shape == (6, len(bench.DUMP_HEADER_FIELDS))
    seg = d["segments"]
    # frame 1: its own segment, then the two of its spill record; the other frames their f % 3 segments
    assert len(seg) == sum(f % 3 for f in range(6)) + 2
    assert list(seg[seg[:, 0] == 1][:, 4]) == [-1001.0, -7.0, -8.0]  # (frame, normal x3, d, ...)
    assert seg.shape[1] == 1 + sum(int(np.prod(cape_amd.PLANE_SEGMENT_DTYPE[k].shape) or 1) for k in bench.DUMP_SEGMENT_FIELDS)
    b = d["boundary_points"]
    assert b.shape[1] == 5
    for f in range(6):
        for p in np.unique(b[b[:, 0] == f][:, 1]):
            pts = b[(b[:, 0] == f) & (b[:, 1] == p)][:, 2:]
            assert np.array_equal(pts, pts[np.lexsort(pts.T[::-1])]), "boundary points sorted within their plane"
    assert [5.0, 6.0, 7.0] in b[b[:, 0] == 1][:, 2:].tolist()  # the spill record's plane
    # a run without the cylinder branch hands out no cylinder outputs
    assert not {"cyl_labels", "cylinders"} & set(bench._batch_outputs(res, None, np.arange(6), cylinders=False))


def test_dump_outputs_samples_to_the_budget(tmp_path):
    res = _batch(3000)
    make = lambda fr: bench._batch_outputs(res, None, fr)  # noqa: E731
    total = bench.dump_outputs(str(tmp_path / "a"), make, 3000, 200_000)
    assert total <= 200_000
    fr = np.load(tmp_path / "a" / "frames.npy")
    assert fr.dtype == np.float64 and 1 <= len(fr) <= 1024 and np.all(np.diff(fr) > 0) and fr.max() < 3000
    bench.dump_outputs(str(tmp_path / "b"), make, 3000, 200_000)
    for n in sorted(p.name for p in (tmp_path / "a").iterdir()):
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)), n
    # a small batch goes out whole; no file is empty: the cylinder table is left out while no frame holds a cylinder
    bench.dump_outputs(str(tmp_path / "c"), lambda f: bench._batch_outputs(_batch(5), None, f), 5, 1 << 20)
    assert np.array_equal(np.load(tmp_path / "c" / "frames.npy"), np.arange(5))
    names = {p.name for p in (tmp_path / "c").iterdir()}
    assert "cylinders.npy" not in names and "cyl_labels.npy" in names
    assert all(np.load(tmp_path / "c" / n).size > 0 for n in names)
    bench.dump_outputs(str(tmp_path / "d"), lambda f: bench._batch_outputs(_batch(5, cylinder=True), None, f), 5, 1 << 20)
    cyl = np.load(tmp_path / "d" / "cylinders.npy")
    assert cyl.shape == (1, 1 + 3 + 1 + 1 + 1) and cyl[0, :4].tolist() == [0.0, 1.0, 0.0, 0.0]


def test_gathered_outputs_in_stream_order():
    lay = dist.packed_layout(4, 12, planes_per_frame=2, cylinders_per_frame=1)
    bufs = []
    for r, first in enumerate((0, 2)):
        buf = np.zeros(lay["bytes_per_rank"], np.uint8)
        hdr = buf[: cape_amd.PACKED_HEADER_DTYPE.itemsize].view(cape_amd.PACKED_HEADER_DTYPE)
        hdr["magic"], hdr["n_frames"], hdr["first_frame"] = cape_amd.PACKED_MAGIC, 2, first
        fr = buf[lay["frames_offset"]: lay["frames_offset"] + 2 * cape_amd.PACKED_FRAME_DTYPE.itemsize].view(cape_amd.PACKED_FRAME_DTYPE)
        fr["plane_offset"], fr["n_planes"] = (0, 1), (1, r + 1)
        pl = buf[lay["planes_offset"]: lay["planes_offset"] + 3 * cape_amd.PACKED_PLANE_DTYPE.itemsize].view(cape_amd.PACKED_PLANE_DTYPE)
        pl["d"] = np.arange(3) + 10 * r
        bufs.append(buf)
    shards = dist.unpack_gathered(np.concatenate(bufs), 2, lay)
    d = bench._gathered_outputs(shards, np.arange(4))
    assert "gathered_cylinders" not in bench._gathered_outputs(shards, np.arange(4), cylinders=False)
    assert d["gathered_frames"][:, 3].tolist() == [1, 1, 1, 2]
    assert d["gathered_planes"][:, 0].tolist() == [0, 1, 2, 3, 3] and d["gathered_planes"][:, 4].tolist() == [0, 1, 10, 11, 12]
    assert all(a.dtype == np.float64 for a in d.values())
