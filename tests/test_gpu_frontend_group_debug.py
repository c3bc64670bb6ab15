"""Debug images in a slam::FrontendGroup: with FrontendConfig::debug_colour_seeded_ every member draws its stereo lines'
colours from a generator of its own (vsf_observe_set_debug_seeds), so every member's getDebugImages / getDebugStereoImages /
GetLast... / ...Compressed are those of a seeded Frontend of its own -- which in turn equals an unseeded Frontend after
srand(seed): the new path is tied to the old one.  Byte for byte; no tolerance."""
import ctypes as C
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import test_gpu_frontend_group as tg  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, NF, LIFE = tg.W, tg.H, tg.NF, tg.LIFE
SEEDS = [1, 7, 4242]


def _feed(calls, m, observe_odometry, observe_image):
    for c in calls:
        if c[1] != m:
            continue
        if c[0] == "odom":
            observe_odometry(c[2], tg.Q, c[3])
        else:
            observe_image(c[2], c[3], c[4])


def _pictures(fe, files=False):
    """Everything a Frontend hands out of its debug images, as bytes."""
    assert fe.flush()
    if files:
        return [(fe.last_debug_image_compressed(s), fe.last_debug_image_format(s)) for s in (False, True)]
    last = [fe.last_debug_image(s) for s in (False, True)]
    return ([im.tobytes() for im in fe.debug_images(False)], [im.tobytes() for im in fe.debug_images(True)],
            [None if im is None else im.tobytes() for im in last])


def _own_frontend(calls, m, seed=None, srand=None, fused=True, **form):
    """A synchronous Frontend of member m's configuration fed member m's calls.  seed: debug_colour_seed; srand: the process's
    rand() is seeded once the object (and its context) exists, before the first frame."""
    from vision_slam_frontend_amd import frontend
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=tg.FS[m], best_percent=tg.BPS[m], frame_life=LIFE, debug_images=True,
                           debug_colour_seed=seed, **form)
    try:
        fe.set_fused(fused)
        if srand is not None:
            C.CDLL("libc.so.6").srand(srand)
        _feed(calls, m, fe.observe_odometry, fe.observe_image)
        return _pictures(fe, files=bool(form))
    finally:
        fe.close()


@pytest.fixture(scope="module")
def world():
    calls = tg._calls()
    want = [_own_frontend(calls, m, seed=SEEDS[m]) for m in range(3)]
    for m in range(3):  # match images from the second node on, a stereo image per node, and nobody's are another's
        assert len(want[m][0]) == len(want[m][1]) - 1 >= tg.N - 2 and want[m][2][0] == want[m][0][-1]
    assert len({w[1][-1] for w in want}) == 3
    return calls, want


def test_a_seeded_frontend_is_the_old_switch_after_srand(world):
    calls, want = world
    for m in range(3):
        assert _own_frontend(calls, m, srand=SEEDS[m]) == want[m], "member %d" % m


def test_per_call_mode_of_a_seeded_frontend_equals_its_fused_mode(world):
    calls, want = world
    assert _own_frontend(calls, 1, seed=SEEDS[1], fused=False) == want[1]


def _group(calls, depth, **form):
    from vision_slam_frontend_amd import frontend
    group = frontend.FrontendGroup(W, H, tg.FS, nfeatures=NF, best_percents=tg.BPS, frame_life=LIFE, debug_images=True,
                                   debug_colour_seeds=SEEDS, **form)
    try:
        group.set_pipelined(True)
        group.set_queue(depth, min(depth, 8), 0)
        for c in calls:
            if c[0] == "odom":
                group.observe_odometry(c[1], c[2], tg.Q, c[3])
            else:
                group.observe_image(c[1], c[2], c[3], c[4])
        got = [_pictures(m, files=bool(form)) for m in group.members]
        stats = group.queue_stats()
    finally:
        group.close()
    return got, stats


@pytest.mark.parametrize("depth", [1, 4, 32])
def test_group_members_equal_seeded_frontends(world, depth):
    calls, want = world
    got, stats = _group(calls, depth)
    for m in range(3):
        assert got[m] == want[m], "member %d's debug images differ from a Frontend of its own" % m
    assert stats["streams"] == 3 and stats["seeded_colour_frames"] == stats["frames"] > 0


@pytest.mark.parametrize("form", [{"debug_jpeg_quality": 90}, {"debug_png": True}], ids=["jpeg", "png"])
def test_group_file_forms(world, form):
    calls, _ = world
    want = [_own_frontend(calls, m, seed=SEEDS[m], **form) for m in range(3)]
    assert all(w[0][0] and w[1][0] and w[1][1] == ("png" if "debug_png" in form else "jpeg") for w in want)
    got, _ = _group(calls, 4, **form)
    assert got == want


def test_a_group_with_debug_images_and_no_seeds_is_refused():
    from vision_slam_frontend_amd import capi, frontend
    with pytest.raises(capi.VsfError) as e:
        frontend.FrontendGroup(W, H, tg.FS, nfeatures=NF, frame_life=LIFE, debug_images=True)
    assert e.value.status == capi.VSF_ERR_UNSUPPORTED
