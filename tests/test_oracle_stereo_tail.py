"""The floating-point tail of ObserveImage on the CPU: the fixtures and bounds that tests/test_gpu_stereo_tail.py holds the
HIP kernels to, proved here on the oracle.

A  F_DENSE (tests/stereo_tail_ref.py) is dense, neither symmetric nor antisymmetric, and on the synthetic frames the GPU
   tests use it tells apart what F_RECT cannot: a transposed F, left and right swapped, the other residual_order.
C  RemoveAmbigStereo's residuals against |l^T F r| in float64 within the derived rounding bound, the ordered mean within
   its bound; the bound is sharp enough to reject a transposed F.
D  Calculate3DPoints / UndistortFeaturePoints on crafted geometry (near, mid, far, behind, at infinity, noisy, corners,
   outside, centre, axes) against numpy float64 definitions; the triangulation bound rejects three mutated references
   (DLT built in float32, 4 rows where 6 are asked for, left and right views swapped)."""
import numpy as np
import pytest

import stereo_tail_ref as R
from test_oracle_points import _reference_calibration

NF = 700


@pytest.fixture(scope="module")
def frames_orb(oracle):
    """The frames of tests/test_gpu_stereo_tail.py's sequences through the oracle: (kl, kr, matches) per frame."""
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(320, 240, n_objects=400)
    out = []
    for f in range(5):
        ol, orr = oracle.Orb(nfeatures=NF), oracle.Orb(nfeatures=NF)
        ol.run(sc.render(f, 0))
        orr.run(sc.render(f, 1))
        kl, dl = ol.result()
        kr, dr = orr.result()
        out.append((kl, kr, oracle.get_matches(dl, dr)))
    return out


def _chain(oracle, frames, F, order=0, swap=False):
    """The threshold chain over `frames`; returns [(keep, residuals, threshold_next)] per frame."""
    thr = np.float32(10000.0)
    out = []
    oracle.set_residual_order(order)
    try:
        for kl, kr, m in frames:
            if swap:
                ms = m.copy()
                ms["queryIdx"], ms["trainIdx"] = m["trainIdx"], m["queryIdx"]
                keep, res, nxt, _ = oracle.remove_ambig_stereo(kr, kl, ms, F, float(thr))
            else:
                keep, res, nxt, _ = oracle.remove_ambig_stereo(kl, kr, m, F, float(thr))
            out.append((keep, res, np.float32(nxt)))
            thr = np.float32(nxt)
    finally:
        oracle.set_residual_order(0)
    return out


def test_f_dense_fixture():
    F = R.F_DENSE
    assert F.dtype == np.float32 and (F != 0).all()
    assert not np.array_equal(F, F.T) and not np.array_equal(F, -F.T)
    assert np.abs(F - F.T).max() > 0.1 and np.abs(F + F.T).max() > 0.1
    # and it is what its docstring says: H_l^T F_RECT H_r from two different near-identity homographies
    assert not np.allclose(R.H_LEFT, R.H_RIGHT)
    for H in (R.H_LEFT, R.H_RIGHT):
        assert np.abs(H - np.eye(3)).max() < 0.7 and np.abs(H[:2, :2] - np.eye(2)).max() < 0.03
    np.testing.assert_array_equal(F, (R.H_LEFT.T @ R.F_RECT.astype(np.float64) @ R.H_RIGHT).astype(np.float32))


@pytest.mark.parametrize("F_name", ["F_DENSE", "F_DENSE_DEV"])
def test_dense_f_sees_transpose_swap_and_summation_order(oracle, frames_orb, F_name):
    """A.2: with F_RECT all three mistakes give the same bits (checked first); with the dense F each one changes the kept
    sets or the threshold bits somewhere in the sequence."""
    def sig(chain):
        return [(keep.tobytes(), thr.tobytes()) for keep, _, thr in chain]

    rect = sig(_chain(oracle, frames_orb, R.F_RECT))
    assert rect == sig(_chain(oracle, frames_orb, R.F_RECT.T)) == sig(_chain(oracle, frames_orb, R.F_RECT, swap=True))
    assert rect == sig(_chain(oracle, frames_orb, R.F_RECT, order=1))
    F = getattr(R, F_name)
    base = sig(_chain(oracle, frames_orb, F))
    for what, other in (("F^T", _chain(oracle, frames_orb, F.T.copy())), ("left/right swapped", _chain(oracle, frames_orb, F, swap=True)),
                        ("residual_order 1", _chain(oracle, frames_orb, F, order=1))):
        differs = sig(other) != base
        assert differs, what


def test_f_dense_keeps_a_realistic_share(oracle, frames_orb):
    """mean + 2 keeps most of the synthetic pair's matches under F_DENSE, as it does under F_RECT, and drops some."""
    chain = _chain(oracle, frames_orb, R.F_DENSE)
    shares = [keep.mean() for keep, _, _ in chain[1:]]
    assert min(shares) > 0.5 and min(shares) < 1.0, shares
    assert chain[0][0].all()  # the first frame: threshold 10000


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("F_name", ["F_RECT", "F_DENSE", "F_DENSE_DEV"])
def test_residuals_and_means_within_the_float64_bound(oracle, frames_orb, F_name, order):
    """C, float64: every oracle residual within residuals64's derived bound of |l^T F r| in float64 (the GPU must equal these
    bit for bit: tests/test_gpu_stereo_tail.py), every frame's mean (threshold - 2) within mean_bound of the float64 mean."""
    F = getattr(R, F_name)
    worst = 0.0
    for (kl, kr, m), (keep, res, thr) in zip(frames_orb, _chain(oracle, frames_orb, F, order)):
        want, bound = R.residuals64(kl, kr, m, F)
        assert (np.abs(res.astype(np.float64) - want) <= bound).all()
        worst = max(worst, float((np.abs(res - want) / np.maximum(bound, 1e-300)).max()))
        m64, mb = R.mean_bound(res)
        # thr = fl(mean + 2): undo the + 2 with its own rounding (u * |thr|)
        assert abs((float(thr) - 2.0) - m64) <= mb + R.U * abs(float(thr))
    if F_name == "F_RECT":
        assert worst == 0.0  # integers and pixel coordinates: every product and sum exact
    else:
        assert 0 < worst <= 1


def test_residual_bound_rejects_a_transposed_f(oracle, frames_orb):
    kl, kr, m = frames_orb[1]
    _, res_t, _, _ = oracle.remove_ambig_stereo(kl, kr, m, R.F_DENSE.T.copy(), 10000.0)
    want, bound = R.residuals64(kl, kr, m, R.F_DENSE)
    assert (np.abs(res_t - want) > bound).mean() > 0.9


def _calib():
    K, P1, P2, dist = _reference_calibration()
    return K, P1, P2, dist


@pytest.mark.parametrize("rows", [6, 4])
def test_triangulation_of_crafted_geometry_within_the_float64_bound(oracle, rows):
    """D, on the oracle: every point class within triangulation_bound of the numpy float64 SVD; the finite pattern agrees."""
    K, P1, P2, _ = _calib()
    x1, x2, lab = R.point_classes(P1, P2, K)
    ref = R.triangulate64(P1, P2, x1, x2, rows)
    Y = oracle.triangulate_points(P1, P2, x1, x2, rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        got = Y[:, :3] / Y[:, 3:]
    assert R.triangulation_excess(ref, got) <= 1.0
    # every class is determined by its system (the bound is finite), the points at infinity included
    assert np.isfinite(R.triangulation_bound(ref)).all()
    assert (np.abs(ref["v"][lab == "infinity", 3]) < 1e-5).all()
    assert (ref["p"][lab == "behind", 2] < 0).all()


def test_noisy_points_separate_the_4_and_6_row_answers():
    K, P1, P2, _ = _calib()
    x1, x2, lab = R.point_classes(P1, P2, K)
    s = lab == "noisy"
    p6, p4 = R.triangulate64(P1, P2, x1[s], x2[s], 6)["p"], R.triangulate64(P1, P2, x1[s], x2[s], 4)["p"]
    assert np.abs(p6 - p4).max() > 1e-2


@pytest.mark.parametrize("rows", [6, 4])
def test_triangulation_bound_rejects_mutated_references(rows):
    """The bound is sharp: each of three wrong references lies outside it on the crafted points."""
    K, P1, P2, _ = _calib()
    x1, x2, _ = R.point_classes(P1, P2, K)
    ref = R.triangulate64(P1, P2, x1, x2, rows)
    mutants = {
        "DLT built in float32": R.triangulate64(P1, P2, x1, x2, rows, build32=True)["p"],
        "other row count": R.triangulate64(P1, P2, x1, x2, 10 - rows)["p"],
        "left and right swapped": R.triangulate64(P1, P2, x2, x1, rows)["p"],
    }
    for what, p in mutants.items():
        try:
            excess = R.triangulation_excess(ref, p)
        except AssertionError:  # (a different finite pattern is a rejection too)
            excess = np.inf
        assert excess > 10, what


def test_undistortion_restated_operation_for_operation(oracle, record_property):
    """D, undistortion: the oracle equals the float64 restatement of cvUndistortPoints bit for bit on every crafted left
    pixel (corners, outside, centre, axes).  How far five iterations are from the fixed point at the corners is reported
    (record_property `corner_unconverged_px`), not asserted: that is the reference's behaviour."""
    K, P1, P2, dist = _calib()
    x1, _, lab = R.point_classes(P1, P2, K)
    got = oracle.undistort_points(x1, K, dist)
    assert R.ulp_distance(got, R.undistort64(x1, K, dist)).max() == 0
    c = lab == "corner"
    gap = np.abs(R.undistort64(x1[c], K, dist, iters=200).astype(np.float64) - got[c]).max()
    record_property("corner_unconverged_px", float(gap))
    print("five undistortion iterations at the image corners: %.3g px from the fixed point" % gap)
    assert np.isfinite(gap)
