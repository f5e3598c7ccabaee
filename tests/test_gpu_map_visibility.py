"""cape_map_visibility: which map planes a frame's camera can see, decided on the device (the first statement of the get_matches
loop).  The words are compared bit for bit with the host twin cape_host_map_visibility, which takes no shortcut; with
MATCH_MAP_DEVICE_SKIP the matchers read them on the device and return what they return for the same words passed from the host."""
import numpy as np
import pytest

from test_gpu_map_match import _bits, _kept, _lift, _map_from, _stream, _w2c
from test_gpu_match_map_shards import ragged  # noqa: F401  (the module's fixture of ragged shards)
from test_map_visibility_host import H, HAND_CASES, INTR, W, all_cases, bits, poses

pytestmark = pytest.mark.gpu

N_FRAMES, N_MAP = 5, 70  # not a multiple of the 4 frames of a workgroup; more than 64 lanes and not a multiple of 32


def _handle(intr=INTR):
    from cape_amd import Extractor

    return Extractor(W, H, cylinders=False, max_batch=8, **intr)


def _twin_words(planes, T, intr=INTR, moving=None):
    import cape_amd

    arrays = cape_amd.pack_map(planes)
    return np.stack([cape_amd.host_map_visibility(arrays, t, W, H, intr["fx"], intr["fy"], intr["cx"], intr["cy"], moving) for t in T])


@pytest.fixture(scope="module")
def cases(hip_library):
    """the 70 case planes, the 5 poses and the twin's words for them (computed once)"""
    planes = [c[1] for c in all_cases(N_MAP)]
    T = np.stack(poses())
    assert len(planes) == N_MAP and len(T) == N_FRAMES
    return planes, T, _twin_words(planes, T)


def test_device_words_equal_the_twin(cases):
    planes, T, want = cases
    ex = _handle()
    ex.upload_map(planes)
    ex.map_visibility(N_FRAMES, T)
    words, undecided = ex.map_visibility_words(N_FRAMES)
    assert words.shape == (N_FRAMES, 3) and undecided == 0
    for f in range(N_FRAMES):
        got, ref = bits(words[f], N_MAP), bits(want[f], N_MAP)
        assert got == ref, f"frame {f}: planes {[j for j in range(N_MAP) if got[j] != ref[j]]} differ from the twin"
    assert np.array_equal(words, want)  # (the tail bits of the last word included: 0)
    # the hand-built expectations hold on the device under the identity pose
    for j, (name, _, visible, _) in enumerate(HAND_CASES):
        assert bits(words[0], N_MAP)[j] == (not visible), name
    # fewer frames than the call covered may be copied, more may not; poses None = identity
    import cape_amd

    assert np.array_equal(ex.map_visibility_words(2)[0], want[:2])
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.map_visibility_words(N_FRAMES + 1)
    ex.map_visibility(1, None)
    assert np.array_equal(ex.map_visibility_words(1)[0], want[:1])
    ex.close()


def test_rings_that_touch_the_rectangle_exactly():
    """fx = fy = 512 and a map plane at Z = 512: x = -319 mm lands on u == 1.0 and x = 319 on u == 639.0 without rounding"""
    intr = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    def square(x0, x1):
        ring = np.array([[x0, -50.0], [x1, -50.0], [x1, 50.0], [x0, 50.0]])
        return (np.array([0.0, 0.0, 1.0]), -512.0, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 512.0]), ring, [])

    planes = [square(-400.0, -319.0), square(-400.0, np.nextafter(-319.0, 0.0)), square(319.0, 400.0), square(np.nextafter(319.0, 0.0), 400.0),
              square(-100.0, 100.0)]
    T = np.stack([np.eye(4)])
    want = _twin_words(planes, T, intr)
    skipped = bits(want[0], len(planes))
    print("twin:", skipped)
    assert skipped[0] and skipped[2] and not skipped[4]  # max_u == 1.0 / min_u == 639.0: no area in common (the full computation)
    ex = _handle(intr)
    ex.upload_map(planes)
    ex.map_visibility(1, T)
    words, undecided = ex.map_visibility_words(1)
    assert undecided == 0 and np.array_equal(words, want)  # (planes 1 and 3, one ulp inside: whatever the twin says)
    ex.close()


def test_moving_composes(cases):
    planes, T, want = cases
    rng = np.random.default_rng(1)
    moving = rng.integers(0, 2**32, 3, dtype=np.uint64).astype(np.uint32)
    moving[2] &= np.uint32((1 << (N_MAP - 64)) - 1)
    ex = _handle()
    ex.upload_map(planes)
    ex.map_visibility(N_FRAMES, T, moving)
    words, undecided = ex.map_visibility_words(N_FRAMES)
    assert undecided == 0 and np.array_equal(words, want | moving[None, :])
    assert np.array_equal(words, _twin_words(planes, T, moving=moving))
    ex.close()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[2]), _bits(b[2]))


def test_the_flag_equals_the_host_route():
    import cape_amd

    n = 8
    ex, st, c2w = _stream("room", 4, 30, 5, n)
    kept = _kept(ex, n)
    planes = _map_from(kept, c2w, (0, 3), np.random.default_rng(6), size=40)
    # ... and walls far off to one side: never on the screen
    R, o = c2w[0]
    planes += [_lift(k, R, o, ring=k[5] + np.array([60000.0, 0.0])) for _, k in kept[0][:3]]
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    ex.map_visibility(n, T, None, st)
    words, undecided = ex.map_visibility_words(n)
    skipped = np.array([bits(words[f], len(planes)) for f in range(n)])
    assert undecided == 0 and skipped.any() and not skipped.all()
    assert np.array_equal(words, _twin_words(planes, T, synth_intr()))
    flags = cape_amd.MATCH_MAP_AREAS
    ex.match_map(n, T, None, flags | cape_amd.MATCH_MAP_DEVICE_SKIP, st)
    got = ex.map_matches(n, areas=True)
    ex.match_map(n, T, words, flags, st)
    want = ex.map_matches(n, areas=True)
    assert _same(got, want)
    assert int(want[0]["n_matched"].sum()) > 0
    ex.match_map(n, T, None, flags, st)
    assert not _same(ex.map_matches(n, areas=True), want)  # (the words do skip pairs the matcher would intersect)
    ex.close()


def synth_intr():
    from cape_amd import synth

    return synth.DEFAULT_INTRINSICS


def test_the_flag_through_match_map_shards(ragged):  # noqa: F811
    import cape_amd

    R = ragged
    n_shards, n_slots = 2, 16  # shards of 5 and 8 frames: slots 5, 6, 7 are empty
    owner, st, ptr = R.owner, R.stream, R.device.data_ptr()
    T = R.T[:n_slots]
    owner.map_visibility(n_slots, T, None, st)
    words, undecided = owner.map_visibility_words(n_slots)
    skipped = np.array([bits(words[s], len(R.planes)) for s in range(n_slots)])
    assert undecided == 0 and skipped.any() and not skipped.all()
    assert np.array_equal(words, _twin_words(R.planes, T, synth_intr()))
    flags = cape_amd.MATCH_MAP_AREAS
    owner.match_map_shards(ptr, n_shards, R.layout, T, None, flags | cape_amd.MATCH_MAP_DEVICE_SKIP, st)
    got = owner.shard_map_matches(n_slots, areas=True)
    owner.match_map_shards(ptr, n_shards, R.layout, T, words, flags, st)
    want = owner.shard_map_matches(n_slots, areas=True)
    assert _same(got, want)
    assert np.all(want[0]["n_cur"][5:8] == 0) and int(want[0]["n_matched"].sum()) > 0
    # three shards need 24 slots of words: the call above covered 16
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        owner.match_map_shards(ptr, 3, R.layout, R.T, None, flags | cape_amd.MATCH_MAP_DEVICE_SKIP, st)


def test_arguments(cases):
    import cape_amd

    planes, T, want = cases
    n = 4
    ex, st, c2w = _stream("room", 4, 30, 5, n)
    Tn = np.stack([_w2c(*c2w[f]) for f in range(n)])
    skip_flag = cape_amd.MATCH_MAP_DEVICE_SKIP
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):  # no map yet
        ex.map_visibility(n, Tn, None, st)
    ex.upload_map(planes)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.map_visibility(0, None, None, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # no visibility call yet
        ex.match_map(n, Tn, None, skip_flag, st)
    ex.map_visibility(n - 1, Tn[: n - 1], None, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # it covered fewer frames
        ex.match_map(n, Tn, None, skip_flag, st)
    ex.match_map(n - 1, Tn[: n - 1], None, skip_flag, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):  # the words come from the device: no skip argument
        ex.match_map(n - 1, Tn[: n - 1], np.zeros((n - 1, 3), np.uint32), skip_flag, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_map(n - 1, Tn[: n - 1], None, 1 << 7, st)
    ex.upload_map(planes)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # a new upload discards the words
        ex.match_map(n - 1, Tn[: n - 1], None, skip_flag, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.map_visibility_words(1)
    ex.upload_map([])
    ex.map_visibility(n, Tn, None, st)  # an empty map: nothing to write
    words, undecided = ex.map_visibility_words(n)
    assert words.shape == (n, 0) and undecided == 0
    ex.match_map(n, Tn, None, skip_flag, st)
    assert np.all(ex.map_matches(n)[0]["n_matched"] == 0)
    ex.close()


def test_other_calls_leave_the_words_alone(cases):
    import torch
    import cape_amd
    from cape_amd import synth_gpu

    planes, T, want = cases
    n = 4
    ex, st, c2w = _stream("room", 4, 30, 5, n)
    ex.upload_map(planes)
    ex.map_visibility(N_FRAMES, T, None, st)
    dev = torch.cat([synth_gpu.stream("room", 4, 1, start=90 + f, device="cuda", chunk=1) for f in range(n)]).contiguous()
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    ex.match_map(n, np.stack([_w2c(*c2w[f]) for f in range(n)]), None, cape_amd.MATCH_MAP_AREAS, st)
    ex.map_matches(n, areas=True)
    words, undecided = ex.map_visibility_words(N_FRAMES)
    assert undecided == 0 and np.array_equal(words, want)
    ex.close()
