"""slam::Frontend and slam::FrontendGroup with FrontendConfig::orb_score_type_ = FAST_SCORE: the mode belongs to the context,
so per-call, synchronous and pipelined mode book the same SLAMProblem -- and it is the FAST_SCORE problem: the kept frames
are those of tests/orb_score_ref.py's extraction followed by the oracle's stereo filter, not the HARRIS mode's."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import orb_score_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, NF, LIFE = 320, 240, 600, 3
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
Q = np.array([1, 0, 0, 0], np.float32)
FAST_SCORE = 1


def _frames(n=7, seed_shift=0):
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(W, H, n_objects=400, seed=synth.BASE_SEED + seed_shift)
    frames = [(sc.render(f, 0), sc.render(f, 1)) for f in range(n)]
    frames[2] = (frames[2][0], np.full_like(frames[2][1], 128))  # no stereo match in frame 2
    return frames


def _kept_frames(oracle, frames, F):
    """The frames the window holds at the end: (frame id, filtered left keypoints, descriptors), from the reference."""
    thr = np.float32(10000.0)
    kept = []
    for fid, (left, right) in enumerate(frames):
        kl, dl, _ = ref.reference(left, NF)
        kr, dr, _ = ref.reference(right, NF)
        m = oracle.get_matches(dl, dr)
        keep, _, thr_new, _ = oracle.remove_ambig_stereo(kl, kr, m, F, float(thr))
        thr = np.float32(thr_new)
        kept.append((fid, kl[m["queryIdx"][keep]], dl[m["queryIdx"][keep]]))
    return kept[-LIFE:]


def _drive(fe, frames, pipelined):
    fe.observe_odometry([0, 0, 0], Q, 0.0)
    for f, (l, r) in enumerate(frames):
        fe.observe_odometry([0.3 * (f + 1), 0, 0], Q, 1.0 + f)
        assert fe.observe_image(l, r) is True
        if pipelined and f % 3 == 2:  # the odometry gate holds a frame back while others are still on the GPU
            fe.observe_odometry([0.3 * (f + 1), 0, 0], Q, 1.5 + f)
            assert fe.observe_image(l, r) is False
    return dict(wire=fe.serialize_problem(), nodes=fe.nodes(), factors=fe.vision_factors(),
                frames=[fe.frame(i) for i in range(LIFE)])


def test_frontend_modes_book_the_same_fast_score_problem(oracle):
    from vision_slam_frontend_amd import frontend
    frames = _frames()
    runs = []
    for fused, pipelined in ((False, False), (True, False), (True, True)):  # per call, synchronous, pipelined
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE, score_type=FAST_SCORE)
        try:
            fe.set_fused(fused)
            fe.set_pipelined(pipelined)
            runs.append(_drive(fe, frames, pipelined))
        finally:
            fe.close()
    per_call, sync, piped = runs
    assert len(sync["nodes"]) == 7 and len(sync["wire"]) > 10000
    assert per_call["wire"] == sync["wire"] == piped["wire"]
    for other in (per_call, piped):
        for (ia, ka, da), (ib, kb, db) in zip(sync["frames"], other["frames"]):
            assert ia == ib and ka.tobytes() == kb.tobytes()
            np.testing.assert_array_equal(da, db)
        assert len(other["factors"]) == len(sync["factors"]) == 0 + 1 + 2 + 3 + 3 + 3 + 3
        for (a0, a1, ap), (b0, b1, bp) in zip(sync["factors"], other["factors"]):
            assert (a0, a1) == (b0, b1)
            np.testing.assert_array_equal(ap, bp)
    # ... and it is the FAST_SCORE problem
    for (fid, kl2, dl2), (gid, gk, gd) in zip(_kept_frames(oracle, frames, F_RECT), sync["frames"]):
        assert gid == fid and gk.tobytes() == kl2.tobytes() and len(kl2) > 20
        np.testing.assert_array_equal(gd, dl2)
        assert set(np.unique(gk["response"])) <= set(np.arange(256, dtype=np.float32))
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE)  # the default: HARRIS_SCORE
    try:
        harris = _drive(fe, frames, False)
    finally:
        fe.close()
    assert harris["wire"] != sync["wire"]
    assert not set(np.unique(harris["frames"][0][1]["response"])) <= set(np.arange(256, dtype=np.float32))


def test_group_of_two_members_in_fast_score_mode(oracle):
    from vision_slam_frontend_amd import frontend
    seqs = [_frames(6, 0), _frames(6, 17)]
    FS = [F_RECT, F_SHIFT]
    want = []
    for m in range(2):
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=FS[m], frame_life=LIFE, score_type=FAST_SCORE)
        try:
            want.append(_drive(fe, seqs[m], False))
        finally:
            fe.close()
    group = frontend.FrontendGroup(W, H, FS, nfeatures=NF, frame_life=LIFE, score_type=FAST_SCORE)
    try:
        group.set_pipelined(True)
        group.set_queue(8, 4, 0)
        for m in range(2):
            group.observe_odometry(m, [0, 0, 0], Q, 0.0)
        for f in range(6):
            for m in (1, 0) if f & 1 else (0, 1):
                group.observe_odometry(m, [0.3 * (f + 1), 0, 0], Q, 1.0 + f)
                assert group.observe_image(m, *seqs[m][f]) is True
        got = [group.serialize_problem(m) for m in range(2)]
        kept = [[group.members[m].frame(i) for i in range(LIFE)] for m in range(2)]
    finally:
        group.close()
    assert got[0] != got[1]
    for m in range(2):
        assert got[m] == want[m]["wire"], "member %d differs from a FAST_SCORE Frontend of its own" % m
        for (fid, kl2, dl2), (gid, gk, gd) in zip(_kept_frames(oracle, seqs[m], FS[m]), kept[m]):
            assert gid == fid and gk.tobytes() == kl2.tobytes()
            np.testing.assert_array_equal(gd, dl2)


def test_a_score_type_no_context_takes_is_refused():
    """The class hands orb_score_type_ to vsf_create as it is: a value outside {HARRIS_SCORE, FAST_SCORE} is the context's
    VSF_ERR_UNSUPPORTED, not a Frontend in some other mode."""
    from vision_slam_frontend_amd import capi, frontend
    with pytest.raises(capi.VsfError) as e:
        frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, score_type=2)
    assert e.value.status == capi.VSF_ERR_UNSUPPORTED
