"""slam::Frontend and slam::FrontendGroup with FrontendConfig::mask_left_ / mask_right_ (Frontend(..., masks=(left, right))):
the masks belong to the context, so per-call, synchronous and pipelined mode book the same SLAMProblem -- and it is the masked
problem: the kept frames are those of tests/orb_mask_ref.py's extraction followed by the oracle's stereo filter, and none of
their keypoints lies in the zero region of the left mask."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import orb_mask_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, NF, LIFE = 320, 240, 600, 3
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
Q = np.array([1, 0, 0, 0], np.float32)
MASKS = ref.masks(W, H)
PAIR = (MASKS["half_plane"], MASKS["rectangle_two_borders"])  # the other eye's housing in the left image, the hood in the right one


def _frames(n=6, seed_shift=0):
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(W, H, n_objects=400, seed=synth.BASE_SEED + seed_shift)
    return [(sc.render(f, 0), sc.render(f, 1)) for f in range(n)]


def _kept_frames(oracle, frames, F, pair):
    """The frames the window holds at the end: (frame id, filtered left keypoints, descriptors), from the reference."""
    thr = np.float32(10000.0)
    kept = []
    for fid, (left, right) in enumerate(frames):
        kl, dl, _ = ref.reference(left, pair[0], NF)
        kr, dr, _ = ref.reference(right, pair[1], NF)
        m = oracle.get_matches(dl, dr)
        keep, _, thr_new, _ = oracle.remove_ambig_stereo(kl, kr, m, F, float(thr))
        thr = np.float32(thr_new)
        kept.append((fid, kl[m["queryIdx"][keep]], dl[m["queryIdx"][keep]]))
    return kept[-LIFE:]


def _drive(fe, frames):
    fe.observe_odometry([0, 0, 0], Q, 0.0)
    for f, (l, r) in enumerate(frames):
        fe.observe_odometry([0.3 * (f + 1), 0, 0], Q, 1.0 + f)
        assert fe.observe_image(l, r) is True
    return dict(wire=fe.serialize_problem(), frames=[fe.frame(i) for i in range(LIFE)])


def _outside_zero_region(kp, mask):
    """A keypoint of level l sits at its level pixel times the level's scale: its own level-0 pixel for l = 0, and within one
    level pixel (ceil(scale) level-0 pixels, + 1 for the rounding of the product) of a non-zero level-0 pixel above --
    a 255 of level l needs every contributing pixel of the level below to be 255, down to level 0."""
    for k in kp:
        scale = float(k["size"]) / 31.0
        m = 0 if k["octave"] == 0 else int(np.ceil(scale)) + 1
        x, y = int(round(float(k["x"]))), int(round(float(k["y"])))
        if not mask[max(y - m, 0):y + m + 1, max(x - m, 0):x + m + 1].any():
            return False
    return True


def test_frontend_modes_book_the_same_masked_problem(oracle):
    from vision_slam_frontend_amd import frontend
    frames = _frames()
    runs = []
    for fused, pipelined in ((False, False), (True, False), (True, True)):  # per call, synchronous, pipelined
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE, masks=PAIR)
        try:
            fe.set_fused(fused)
            fe.set_pipelined(pipelined)
            runs.append(_drive(fe, frames))
        finally:
            fe.close()
    per_call, sync, piped = runs
    assert len(sync["wire"]) > 3000  # (six nodes of a few dozen features each)
    assert per_call["wire"] == sync["wire"] == piped["wire"]
    # ... and it is the masked problem
    for (fid, kl2, dl2), (gid, gk, gd) in zip(_kept_frames(oracle, frames, F_RECT, PAIR), sync["frames"]):
        assert gid == fid and gk.tobytes() == kl2.tobytes() and len(kl2) > 20
        np.testing.assert_array_equal(gd, dl2)
        assert _outside_zero_region(gk, PAIR[0])
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE)  # the default: no masks
    try:
        plain = _drive(fe, frames)
        assert plain["wire"] != sync["wire"]
        assert not all(_outside_zero_region(k, PAIR[0]) for _, k, _ in plain["frames"])
        # masks set on an object that has its context: the frames that follow are masked
        fe.set_masks(*PAIR)
        fe.observe_odometry([3.0, 0, 0], Q, 20.0)
        assert fe.observe_image(*frames[0]) is True
        fid, k, _ = fe.frame(LIFE - 1)
        assert fid == len(frames) and _outside_zero_region(k, PAIR[0])
    finally:
        fe.close()


def test_a_mask_of_another_size_is_refused():
    from vision_slam_frontend_amd import capi, frontend
    with pytest.raises(capi.VsfError) as e:
        frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, masks=(np.full((H, W + 1), 255, np.uint8), None))
    assert e.value.status == capi.VSF_ERR_INVALID_ARG


def test_group_members_carry_their_own_pair(oracle):
    from vision_slam_frontend_amd import frontend
    seqs = [_frames(5, 0), _frames(5, 17), _frames(5, 31)]
    FS = [F_RECT, F_SHIFT, F_RECT]
    pairs = [PAIR, (None, MASKS["half_plane"]), None]
    want = []
    for m in range(3):
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=FS[m], frame_life=LIFE, masks=pairs[m])
        try:
            want.append(_drive(fe, seqs[m]))
        finally:
            fe.close()
    for pipelined in (False, True):
        group = frontend.FrontendGroup(W, H, FS, nfeatures=NF, frame_life=LIFE, masks=pairs)
        try:
            group.set_pipelined(pipelined)
            if pipelined:
                group.set_queue(8, 4, 0)
            for m in range(3):
                group.observe_odometry(m, [0, 0, 0], Q, 0.0)
            for f in range(5):
                for m in (2, 1, 0) if f & 1 else (0, 1, 2):
                    group.observe_odometry(m, [0.3 * (f + 1), 0, 0], Q, 1.0 + f)
                    assert group.observe_image(m, *seqs[m][f]) is True
            got = [group.serialize_problem(m) for m in range(3)]
        finally:
            group.close()
        for m in range(3):
            assert got[m] == want[m]["wire"], "member %d differs from a Frontend of its own (pipelined %d)" % (m, pipelined)
    assert want[0]["wire"] != want[2]["wire"]
