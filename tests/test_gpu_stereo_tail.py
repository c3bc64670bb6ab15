"""The floating-point tail of ObserveImage on the device -- RemoveAmbigStereo (k_frontend.hip: stereo_residual_kernel,
stereo_one_frame_kernel, the threshold chain, the filter) and Calculate3DPoints + UndistortFeaturePoints (k_points.hip:
vision_features_kernel) -- under a fundamental matrix that can see a transposed F, swapped views or the other summation
order (tests/stereo_tail_ref.py F_DENSE: tests/test_oracle_stereo_tail.py proves that on the CPU), on crafted inputs, and
against float64 definitions.

B  every ObserveImage path under F_DENSE against the ORACLE, bit for bit on the integer results and the threshold bits:
   the synchronous call (a batch of one: stereo_one_frame_kernel) in both residual orders, the queue (batches of one and
   of several), the C++ Frontend queued and synchronous; every sequence holds a frame without stereo matches (quirk Q3).
C  vsf_remove_ambig_stereo_batch_dev on crafted cv::KeyPoint / cv::DMatch records: 0, 1, 63, 64, 65, 255, 256, 257, 4097
   and 10 000 matches in one batch with many queries on one train row; thresholds tied to a residual (kept) and one ulp
   below it (dropped), on the first frame and through the chain; capacities 16000 (residuals in LDS, the one-launch lone
   frame) and 16004 (the sum from global memory, the three-launch lone frame); residuals and means against float64.
D  vsf_vision_features_batch_dev on crafted geometry (near, mid, far, behind, at infinity, noisy, corners, outside,
   centre, axes) with 6 and 4 rows, frames of 0, 1, 63, 64, 65 features and one at capacity, some with fewer matches than
   keypoints (quirk Q5): point3d within the derived float64 triangulation bound, pixel equal to cvUndistortPoints restated
   in float64, and the oracle's 1e-5 beside them."""
import numpy as np
import pytest

import stereo_tail_ref as R
from stereo_tail_ref import F_DENSE, F_RECT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NF, LIFE = 700, 3
POINT_RTOL, PIXEL_ATOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _frames(n):
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(320, 240, n_objects=400)
    frames = [(sc.render(f, 0), sc.render(f, 1)) for f in range(n)]
    frames[2] = (frames[2][0], np.full_like(frames[2][1], 128))  # no stereo match: frame 3 is filtered against NaN (Q3)
    return frames


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes() or (np.isnan(a) and np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------- B ----

@pytest.mark.parametrize("F_name,order", [("F_DENSE", 0), ("F_DENSE", 1), ("F_DENSE_DEV", 0)])
def test_B_observe_stereo_under_a_dense_f_follows_the_oracle(oracle, F_name, order):
    """B, synchronous vsf_observe_stereo (a batch of one: stereo_one_frame_kernel) in residual order `order`."""
    from test_gpu_observe import _follow_reference_sequence
    ctx, _, sizes = _follow_reference_sequence(oracle, _frames(6), 320, 240, NF, LIFE, F=getattr(R, F_name), order=order)
    ctx.close()
    assert sizes[2] == 0 and sizes[3] == 0 and min(sizes[4:]) > 10, sizes


@pytest.mark.parametrize("order", [0, 1])
def test_B_queue_under_a_dense_f_follows_the_oracle(oracle, capi, order):
    """B, vsf_observe_submit / collect at depth 6: lone frames and bursts, so that batches of one and of several leave; the
    results against the oracle (not against the synchronous call)."""
    from test_gpu_observe import _follow_reference_sequence
    from vision_slam_frontend_amd import frontend
    import ctypes as C
    frames = _frames(10)
    calib = frontend.default_calibration().set("fundamental", F_DENSE)
    bp = float(np.float32(0.3))
    results = []
    with capi.Context(capi.default_params(320, 240, max_images=8, nfeatures=NF, residual_order=order)) as ctx:
        ctx.observe_configure(6, 0, 0)
        i = 0
        for burst in (1, 4, 1, 4):
            tickets = [ctx.observe_submit(l, r, calib, best_percent=bp, frame_life=LIFE) for l, r in frames[i:i + burst]]
            results += [ctx.observe_collect(t, frame_life=LIFE) for t in tickets]
            i += burst
        stats = (C.c_int64 * 11)()
        assert capi.lib().vsf_observe_stats(ctx._h, stats, 11) == capi.VSF_OK
    assert stats[0] == len(frames) and stats[2] >= 2 and stats[1] < len(frames), list(stats)  # some batch of several
    ctx, _, sizes = _follow_reference_sequence(oracle, frames, 320, 240, NF, LIFE, F=F_DENSE, order=order, results=results)
    ctx.close()
    assert sizes[2] == 0 and sizes[3] == 0 and min(sizes[4:]) > 10, sizes


def test_B_frontend_under_a_dense_f_follows_the_model(oracle):
    """B, slam::Frontend(fundamental=F_DENSE), synchronous and with its queue: thresholds, vision factors, kept frames and
    node features against tests/test_gpu_frontend.py's model of the reference on the oracle."""
    from test_gpu_frontend import NF as FNF, _model
    from vision_slam_frontend_amd import frontend
    frames = _frames(7)
    factors, frame_list, kept = _model(oracle, frames, frame_life=3, calib=frontend.default_calibration(), F=F_DENSE)
    q = np.array([1, 0, 0, 0], np.float32)
    for pipelined in (False, True):
        fe = frontend.Frontend(320, 240, nfeatures=FNF, fundamental=F_DENSE, frame_life=3)
        fe.set_pipelined(pipelined)
        if pipelined:
            fe.set_queue(8, 4, 0)
        fe.observe_odometry([0, 0, 0], q, 0.0)
        thr = []
        for f, (l, r) in enumerate(frames):
            fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 1.0 + f)
            assert fe.observe_image(l, r) is True
            if not pipelined:
                thr.append(np.float32(fe.stereo_ambig_constraint))
        if not pipelined:
            assert all(_same_bits(a, k[2]) for a, k in zip(thr, kept)), (thr, [k[2] for k in kept])
        assert _same_bits(fe.stereo_ambig_constraint, kept[-1][2])
        got = fe.vision_factors()
        assert len(got) == len(factors)
        for (ga, gb, gp), (ea, eb, ep) in zip(got, factors):
            assert (ga, gb) == (ea, eb)
            np.testing.assert_array_equal(gp, ep)
        for i, (fid, kl2, dl2) in enumerate(frame_list):
            gid, gk, gd = fe.frame(i)
            assert gid == fid and gk.tobytes() == kl2.tobytes()
            np.testing.assert_array_equal(gd, dl2)
        for f, node in enumerate(fe.nodes()):
            feat, want = node["features"], kept[f][3]
            assert len(feat) == len(kept[f][0])
            if len(feat) == 0:
                continue
            assert np.abs(feat[:, 1:3].astype(np.float64) - want["pixel"]).max() <= PIXEL_ATOL
            g, w = feat[:, 3:6].astype(np.float64), want["point3d"].astype(np.float64)
            fin = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), fin)
            assert (np.abs(g[fin] - w[fin]) / np.maximum(np.abs(w[fin]), 1e-30)).max() <= POINT_RTOL
        assert [len(n["features"]) for n in fe.nodes()][2:4] == [0, 0] and len(fe.nodes()[4]["features"]) > 10
        fe.close()


# ---------------------------------------------------------------------------------------------------------------- C ----

R_KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                       ("octave", "<i4"), ("class_id", "<i4")])
R_DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def _kp(x, y):
    k = np.zeros(len(x), R_KEYPOINT)
    k["x"], k["y"], k["size"], k["response"] = x, y, 31.0, 1e-3
    return k


def _crafted_frame(rng, nm, nkp=None):
    """nm matches on nkp keypoints per side: right row i is left row i seen ~20 px to the left with ~1.5 px of vertical
    error; a third of the matches point many queries at a few train rows (repeated trainIdx)."""
    nkp = max(nm, 1) if nkp is None else nkp
    x, y = rng.uniform(0, 960, nkp), rng.uniform(0, 600, nkp)
    kl = _kp(x, y)
    kr = _kp(x - rng.uniform(2, 40, nkp), y + rng.normal(0, 1.5, nkp))
    m = np.zeros(nm, R_DMATCH)
    m["queryIdx"] = rng.permutation(nkp)[:nm] if nm <= nkp else rng.integers(0, nkp, nm)
    m["trainIdx"] = m["queryIdx"]
    rep = rng.random(nm) < 1 / 3
    m["trainIdx"][rep] = rng.integers(0, min(nkp, 5), rep.sum())
    m["distance"] = rng.integers(0, 60, nm)
    return kl, kr, m


class _Batch:
    """Crafted frames in a context of capacity K: kp [2B][K], desc [2B][K][32], matches [B][K], nm [B] on the device."""

    def __init__(self, capi, frames, K_override=0, order=0, nfeatures=NF):
        self.frames, self.B = frames, len(frames)
        over = dict(max_keypoints=K_override) if K_override else {}
        self.ctx = capi.Context(capi.default_params(320, 240, max_images=2 * self.B, nfeatures=nfeatures, residual_order=order,
                                                    **over))
        K = self.K = self.ctx.params.max_keypoints
        B = self.B
        kp = np.zeros((2 * B, K), R_KEYPOINT)
        desc = np.random.default_rng(1).integers(0, 256, (2 * B, K, 32), dtype=np.uint8)
        mm = np.zeros((B, K), R_DMATCH)
        nm = np.zeros(B, np.int32)
        for f, (kl, kr, m) in enumerate(frames):
            assert len(kl) <= K and len(kr) <= K and len(m) <= K
            kp[2 * f, :len(kl)], kp[2 * f + 1, :len(kr)], mm[f, :len(m)], nm[f] = kl, kr, m, len(m)
        self.desc = desc
        dev = torch.device("cuda", 0)
        u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        self.t = dict(kp=u8(kp), desc=u8(desc), m=u8(mm), nm=torch.from_numpy(nm).to(dev))
        z = lambda *s, dtype=torch.uint8: torch.zeros(s, dtype=dtype, device=dev)  # noqa: E731
        self.out = dict(means=z(B, dtype=torch.float32), thr=z(B + 1, dtype=torch.float32), kp2=z(2 * B, K, 28),
                        desc2=z(2 * B, K, 32), counts2=z(2 * B, dtype=torch.int32))
        torch.cuda.synchronize()

    def run(self, capi, F, thr_in, override=None):
        t, o = self.t, self.out
        ov = 0
        if override is not None:
            self._ov = torch.from_numpy(np.asarray(override, np.float32)).cuda()
            torch.cuda.synchronize()
            ov = self._ov.data_ptr()
        self.ctx.remove_ambig_stereo_batch_dev(t["kp"].data_ptr(), t["desc"].data_ptr(), t["m"].data_ptr(), t["nm"].data_ptr(),
                                               self.B, F, float(thr_in), ov, o["means"].data_ptr(), o["thr"].data_ptr(),
                                               o["kp2"].data_ptr(), o["desc2"].data_ptr(), o["counts2"].data_ptr())
        assert self.ctx.sync() == capi.VSF_OK
        K, B = self.K, self.B
        return dict(means=o["means"].cpu().numpy(), thr=o["thr"].cpu().numpy(), counts2=o["counts2"].cpu().numpy(),
                    kp2=o["kp2"].cpu().numpy().reshape(2 * B, K * 28).view(R_KEYPOINT),
                    desc2=o["desc2"].cpu().numpy())

    def close(self):
        self.ctx.close()


def _check_against_oracle(oracle, batch, got, F, thr_in, order=0, override=None):
    """Threshold bits, mean + 2 bits, kept keypoints and descriptors of both views per frame; each oracle residual within
    the float64 bound (stereo_tail_ref.residuals64) and each device mean within mean_bound.  Returns the oracle's chain."""
    cur = np.float32(thr_in)
    chain = []
    oracle.set_residual_order(order)
    try:
        for f, (kl, kr, m) in enumerate(batch.frames):
            if override is not None:  # (the override path writes no threshold array)
                th = np.float32(override[f])
            else:
                th = cur
                assert _same_bits(got["thr"][f], th), "frame %d: threshold" % f
            keep, res, nxt, kept = oracle.remove_ambig_stereo(kl, kr, m, F, float(th))
            if len(m) == 0:
                assert np.isnan(got["means"][f]) and np.isnan(nxt)
            else:
                assert _same_bits(np.float32(got["means"][f] + np.float32(2.0)), nxt), "frame %d: mean" % f
                want, bound = R.residuals64(kl, kr, m, F)
                assert (np.abs(res.astype(np.float64) - want) <= bound).all(), "frame %d: residual vs float64" % f
                m64, mb = R.mean_bound(res)
                assert abs(float(got["means"][f]) - m64) <= mb, "frame %d: mean vs float64" % f
            assert got["counts2"][2 * f] == got["counts2"][2 * f + 1] == kept, "frame %d: kept" % f
            q, t = m["queryIdx"][keep], m["trainIdx"][keep]
            assert got["kp2"][2 * f, :kept].tobytes() == kl[q].tobytes(), "frame %d: left keypoints" % f
            assert got["kp2"][2 * f + 1, :kept].tobytes() == kr[t].tobytes(), "frame %d: right keypoints" % f
            np.testing.assert_array_equal(got["desc2"][2 * f, :kept], batch.desc[2 * f][q])
            np.testing.assert_array_equal(got["desc2"][2 * f + 1, :kept], batch.desc[2 * f + 1][t])
            chain.append((keep, res, np.float32(nxt)))
            cur = np.float32(nxt)
    finally:
        oracle.set_residual_order(0)
    if override is None:
        assert _same_bits(got["thr"][batch.B], cur)
    return chain


MATCH_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 10000]


@pytest.mark.parametrize("order", [0, 1])
def test_C_match_counts_at_lane_and_workgroup_edges(oracle, capi, order):
    """C: 0, 1, 63, 64, 65, 255, 256, 257, 4097 and 10 000 matches in ONE batch under F_DENSE (frame 1 is filtered against
    the NaN of frame 0, quirk Q3), then the same frames with per-frame thresholds (the override path)."""
    rng = np.random.default_rng(100 + order)
    frames = [_crafted_frame(rng, n) for n in MATCH_COUNTS]
    b = _Batch(capi, frames, order=order, nfeatures=10000)
    try:
        got = b.run(capi, F_DENSE, 10000.0)
        chain = _check_against_oracle(oracle, b, got, F_DENSE, 10000.0, order)
        assert got["counts2"][2] == 0 and np.isnan(got["thr"][1])  # (NaN threshold after the empty frame)
        kept = [int(k.sum()) for k, _, _ in chain]
        assert all(0 < k < n for k, n in zip(kept[3:], MATCH_COUNTS[3:])), kept  # filtering bites on every later frame
        over = [np.float32(np.median(r)) if len(r) else np.float32(1.0) for _, r, _ in chain]
        got = b.run(capi, F_DENSE, 10000.0, override=over)
        _check_against_oracle(oracle, b, got, F_DENSE, 10000.0, order, override=over)
    finally:
        b.close()


def test_C_threshold_ties_keep_and_one_ulp_below_drops(oracle, capi):
    """C: `residual <= threshold`.  First frame: thr_in equal to one match's residual (same float bits) keeps it,
    nextafter(thr, -inf) drops it (F_DENSE).  Through the chain (F_RECT, where a residual |y_r - y_l| with y_l = 0 is exactly
    y_r): frame k + 1 holds a match whose residual IS mean_k + 2 (kept) and one a float above it (dropped), twice."""
    rng = np.random.default_rng(7)
    f0 = _crafted_frame(rng, 300)
    oracle.set_residual_order(0)
    _, res0, _, _ = oracle.remove_ambig_stereo(*f0, F_DENSE, 10000.0)
    j = int(np.argsort(res0)[150])
    tie = np.float32(res0[j])
    b = _Batch(capi, [f0, _crafted_frame(rng, 100)], nfeatures=400)
    try:
        for thr_in, kept_j in ((tie, True), (np.nextafter(tie, np.float32(-np.inf)), False)):
            got = b.run(capi, F_DENSE, thr_in)
            chain = _check_against_oracle(oracle, b, got, F_DENSE, thr_in)
            assert bool(chain[0][0][j]) is kept_j
    finally:
        b.close()
    # through the chain, on F_RECT: craft frame k + 1 from the oracle's threshold after frame k
    frames = [_crafted_frame(rng, 200)]
    for _ in range(2):
        thr = np.float32(10000.0)
        for fr in frames:
            _, _, nxt, _ = oracle.remove_ambig_stereo(*fr, F_RECT, float(thr))
            thr = np.float32(nxt)
        kl, kr, m = _crafted_frame(rng, 150, nkp=160)
        kl["y"][150], kr["y"][150] = 0.0, thr                                   # residual == threshold: kept
        kl["y"][151], kr["y"][151] = 0.0, np.nextafter(thr, np.float32(np.inf))  # one float above: dropped
        m["queryIdx"][:2], m["trainIdx"][:2] = [150, 151], [150, 151]
        frames.append((kl, kr, m))
    b = _Batch(capi, frames, nfeatures=400)
    try:
        got = b.run(capi, F_RECT, 10000.0)
        chain = _check_against_oracle(oracle, b, got, F_RECT, 10000.0)
        for k in (1, 2):
            assert chain[k][0][0] and not chain[k][0][1], "frame %d" % k
            assert _same_bits(got["thr"][k], frames[k][1]["y"][150])
    finally:
        b.close()


def test_C_capacity_at_the_lds_boundary(oracle, capi):
    """C: capacities 16000 (residuals kept in LDS; a lone frame in one launch) and 16004 (the mean summed from global
    memory; a lone frame in three launches), through vsf_remove_ambig_stereo_batch_dev with 16000 matches in a frame and
    through vsf_observe_stereo under F_DENSE: bit-identical to each other and to the oracle."""
    from test_gpu_observe import _follow_reference_sequence, _same_observation
    from vision_slam_frontend_amd import frontend
    rng = np.random.default_rng(16000)
    frames = [_crafted_frame(rng, n) for n in (16000, 0, 5000, 257)]
    outs = []
    for K in (16000, 16004):
        b = _Batch(capi, frames, K_override=K)
        try:
            assert b.K == K
            got = b.run(capi, F_DENSE, 10000.0)
            _check_against_oracle(oracle, b, got, F_DENSE, 10000.0)
            outs.append(got)
            one = _Batch(capi, frames[:1], K_override=K)  # a batch of one
            try:
                _check_against_oracle(oracle, one, one.run(capi, F_DENSE, 10000.0), F_DENSE, 10000.0)
            finally:
                one.close()
        finally:
            b.close()
    a, c = outs
    for k in ("means", "thr", "counts2"):
        assert a[k].tobytes() == c[k].tobytes(), k
    seq = _frames(5)
    calib = frontend.default_calibration().set("fundamental", F_DENSE)
    runs = []
    for K in (16000, 16004):
        with capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=NF, max_keypoints=K)) as ctx:
            runs.append([ctx.observe_stereo(l, r, calib, best_percent=float(np.float32(0.3)), frame_life=LIFE) for l, r in seq])
    for g, w in zip(runs[1], runs[0]):
        _same_observation(w, g)
    ctx, _, sizes = _follow_reference_sequence(oracle, seq, 320, 240, NF, LIFE, F=F_DENSE, max_keypoints=16004,
                                               results=runs[1])
    ctx.close()
    assert sizes[3] == 0 and sizes[4] > 10


# ---------------------------------------------------------------------------------------------------------------- D ----

def _vision_frames(rng, calib, K):
    """Frames of (left kp, left desc, right kp, right desc) for vision_features_batch_dev: sizes 0, 1, 63, 64, 65 and K; right
    row k is left row perm[k] of a crafted correspondence, or (some frames) an unmatched random row -- fewer matches than
    keypoints, quirk Q5."""
    P1, P2, K1 = calib.get("projection_left"), calib.get("projection_right"), calib.get("camera_matrix_left")
    x1, x2, lab = R.point_classes(P1.reshape(3, 4), P2.reshape(3, 4), K1.reshape(3, 3))
    out = []
    for n, unmatched in ((0, 0), (1, 0), (63, 5), (64, 0), (65, 9), (K, 11)):
        idx = np.r_[np.arange(len(x1)), rng.integers(0, len(x1), max(n - len(x1), 0))][:n] if n else np.zeros(0, int)
        idx = rng.permutation(idx) if n else idx
        perm = rng.permutation(n)
        if unmatched:
            perm[rng.choice(n, unmatched, replace=False)] = -1
        dl, dr = R.descriptors_for(rng, n, perm, n)
        kl = _kp(x1[idx, 0], x1[idx, 1])
        src = np.where(perm >= 0, perm, 0)
        kr = _kp(x2[idx[src], 0] if n else np.zeros(0), x2[idx[src], 1] if n else np.zeros(0))
        if unmatched:
            kr["x"][perm < 0], kr["y"][perm < 0] = rng.uniform(0, 960, unmatched), rng.uniform(0, 600, unmatched)
        out.append((kl, dl, kr, dr, lab[idx]))
    return out


@pytest.mark.parametrize("rows", [6, 4])
def test_D_points_and_pixels_against_float64(oracle, capi, rows, record_property):
    from vision_slam_frontend_amd import frontend
    calib = frontend.default_calibration()
    calib.triangulate_rows = rows
    Kcap = 128
    rng = np.random.default_rng(rows)
    frames = _vision_frames(rng, calib, Kcap)
    B = len(frames)
    dev = torch.device("cuda", 0)
    with capi.Context(capi.default_params(320, 240, max_images=2 * B, nfeatures=64, max_keypoints=Kcap)) as ctx:
        K = ctx.params.max_keypoints
        assert K == Kcap
        kp = np.zeros((2 * B, K), R_KEYPOINT)
        desc = np.zeros((2 * B, K, 32), np.uint8)
        counts = np.zeros(2 * B, np.int32)
        for f, (kl, dl, kr, dr, _) in enumerate(frames):
            n = len(kl)
            kp[2 * f, :n], kp[2 * f + 1, :n], desc[2 * f, :n], desc[2 * f + 1, :n] = kl, kr, dl, dr
            counts[2 * f] = counts[2 * f + 1] = n
        t_kp = torch.from_numpy(kp.view(np.uint8).reshape(-1)).to(dev)
        t_desc = torch.from_numpy(desc.reshape(-1)).to(dev)
        t_counts = torch.from_numpy(counts).to(dev)
        feat = torch.zeros((B, K, 28), dtype=torch.uint8, device=dev)
        nfeat = torch.zeros(B, dtype=torch.int32, device=dev)
        npts = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.vision_features_batch_dev(calib, t_kp.data_ptr(), t_desc.data_ptr(), t_counts.data_ptr(), B, feat.data_ptr(),
                                      nfeat.data_ptr(), npts.data_ptr())
        assert ctx.sync() == capi.VSF_OK
        feat = feat.cpu().numpy().reshape(B, K * 28).view(capi.VISION_FEATURE_DTYPE)
        nfeat, npts = nfeat.cpu().numpy(), npts.cpu().numpy()
    P1, P2 = calib.get("projection_left").reshape(3, 4), calib.get("projection_right").reshape(3, 4)
    K1, dist = calib.get("camera_matrix_left").reshape(3, 3), calib.get("distortion_left")
    worst, short = 0.0, 0
    seen = set()
    for f, (kl, dl, kr, dr, lab) in enumerate(frames):
        n = len(kl)
        m = oracle.sort_and_trim(oracle.get_matches(dr, dl), 1.0)  # right -> left, sorted (cc:129-132)
        got = feat[f, :n]
        assert nfeat[f] == n and npts[f] == len(m), "frame %d" % f
        short += len(m) < n
        np.testing.assert_array_equal(got["feature_idx"], np.arange(n, dtype=np.uint64))
        # pixel: cvUndistortPoints restated in float64, at most 1 ulp (bit equality expected)
        assert R.ulp_distance(got["pixel"], R.undistort64(np.c_[kl["x"], kl["y"]], K1, dist)).max(initial=0) <= 1
        # point3d: the float64 SVD of the same DLT rows, within the derived bound; zero beyond the match list (Q5)
        li, ri = m["trainIdx"], m["queryIdx"]
        ref = R.triangulate64(P1, P2, np.c_[kl["x"], kl["y"]][li], np.c_[kr["x"], kr["y"]][ri], rows)
        worst = max(worst, R.triangulation_excess(ref, got["point3d"][:len(m)]))
        assert not got["point3d"][len(m):].any()
        seen.update(lab[li])
        # ... and the oracle's restatement of cv::triangulatePoints, 1e-5 relative
        want, want_pts = oracle.vision_features(kl, dl, kr, dr, P1, P2, K1, dist, rows=rows)
        assert want_pts == len(m)
        g, w = got["point3d"].astype(np.float64), want["point3d"].astype(np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin)
        assert (np.abs(g[fin] - w[fin]) / np.maximum(np.abs(w[fin]), 1e-30)).max(initial=0.0) <= POINT_RTOL
    record_property("triangulation_worst_excess", worst)
    assert worst <= 1.0
    assert short >= 3 and seen >= {"near", "mid", "far", "behind", "infinity", "noisy", "corner", "outside", "axis"}
