"""Float64 definitions of the floating-point tail of ObserveImage, for tests/test_oracle_stereo_tail.py,
tests/test_oracle_points.py and tests/test_gpu_stereo_tail.py:

  RemoveAmbigStereo (slam_frontend.cc:369-394): |l^T F r| per match and the float rounding bound of its two three-term
      dot products; the bound of the ordered float mean.
  Calculate3DPoints (cc:117-173): the DLT system of cv::triangulatePoints, solved by numpy's float64 SVD, narrowed to float
      and divided in float as cc:159-165 does; the bound a correct implementation must meet against it.
  UndistortFeaturePoints (cc:323-351): cvUndistortPoints' five fixed-point iterations restated operation for operation.

Plus the fixtures that can see mistakes a rectified F hides: F_DENSE, crafted geometry and crafted descriptors."""
import numpy as np

U = 2.0 ** -24   # float32 unit roundoff
EPS64 = 2.0 ** -52

F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)  # l^T F r = y_r - y_l on a rectified pair
# the dense F of tests/test_gpu_frontend_dev.py::test_residuals_dense_fundamental_both_orders
F_DENSE_DEV = np.array([[2.31e-08, -1.17e-05, 3.45e-03], [1.22e-05, 9.8e-08, -0.11], [-4.1e-03, 0.108, 1.0]], np.float32)


def _homography(deg, scale, shear, shift, persp):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    A = np.array([[c, -s], [s, c]]) @ np.array([[scale, shear], [0.0, 1.0 / scale]])
    H = np.eye(3)
    H[:2, :2] = A
    H[:2, 2] = shift
    H[2, :2] = persp
    return H


# Two different near-identity homographies (a few tenths of a degree, ~1 % scale and shear, sub-pixel shifts and a tiny
# perspective row, which makes every entry of F nonzero): the synthetic rectified pair still roughly satisfies
# l^T F_DENSE r = 0, so mean + 2 keeps a realistic share, but F_DENSE != +-F_DENSE^T and no product is exact.
H_LEFT = _homography(0.3, 1.008, 0.01, (0.3, -0.4), (2e-6, -3e-6))
H_RIGHT = _homography(-0.2, 0.993, -0.012, (-0.2, 0.25), (-1.5e-6, 2.5e-6))
F_DENSE = (H_LEFT.T @ F_RECT.astype(np.float64) @ H_RIGHT).astype(np.float32)


# ---- RemoveAmbigStereo ----

def residuals64(kl, kr, matches, F):
    """|l^T F r| of every match in float64 from the float32 inputs (keypoints and F widened), and the bound on the float32
    computation.  Derivation: each three-term dot product fl(a0 b0 + a1 b1 + a2 b2), summed in EITHER order
    (vsf_params::residual_order), is within gamma_3 * sum |a_i b_i| of the exact value (one product rounding, two
    additions; gamma_k = k u / (1 - k u)).  Stage 1, t_j = (l^T F)_j, so |t^_j - t_j| <= gamma_3 T_j with
    T_j = sum_i |l_i F_ij|, and |t^_j| <= (1 + gamma_3) T_j.  Stage 2 adds gamma_3 sum_j |t^_j r_j| for its own rounding
    plus sum_j |t^_j - t_j| |r_j| carried in: in all  gamma_3 (2 + gamma_3) S,  S = sum_j |r_j| T_j.  fabs is exact."""
    F64 = np.asarray(F, np.float32).astype(np.float64).reshape(3, 3)
    q, t = matches["queryIdx"], matches["trainIdx"]
    l = np.c_[kl["x"][q].astype(np.float64), kl["y"][q].astype(np.float64), np.ones(len(q))]
    r = np.c_[kr["x"][t].astype(np.float64), kr["y"][t].astype(np.float64), np.ones(len(t))]
    res = np.abs(np.einsum("ni,ij,nj->n", l, F64, r))
    S = np.einsum("ni,ij,nj->n", np.abs(l), np.abs(F64), np.abs(r))
    g3 = 3 * U / (1 - 3 * U)
    return res, g3 * (2 + g3) * S


def mean_bound(res32):
    """|fl-mean - float64 mean| of float32 residuals summed one by one in match order, then divided by n in float:
    the sum is within gamma_n * sum |r| of the exact one (n - 1 additions, n <= 2^24 is exact as a float), the division adds
    u |mean|.  So |mean32 - mean64| <= gamma_n * sum |r| / n + u |mean64| (1 + gamma_n)."""
    n = len(res32)
    gn = n * U / (1 - n * U)
    r = np.asarray(res32, np.float64)
    m = r.sum() / n
    return m, gn * np.abs(r).sum() / n + U * abs(m) * (1 + gn)


# ---- Calculate3DPoints ----

def dlt_system(P1, P2, x1, x2, rows, build32=False):
    """The rows x 4 system cvTriangulatePoints builds per point: x*P[2]-P[0], y*P[2]-P[1] (, x*P[1]-y*P[0] for OpenCV
    <= 3.4.1's six rows) for each view, from the float32 inputs widened to double.  build32: the same rows computed in
    float32 arithmetic (a mutation the bound must reject)."""
    dt = np.float32 if build32 else np.float64
    per = rows // 2
    n = len(x1)
    A = np.zeros((n, rows, 4), dt)
    for j, (P, x) in enumerate(((P1, x1), (P2, x2))):
        P = np.asarray(P, np.float32).reshape(3, 4).astype(dt)
        x = np.asarray(x, np.float32).reshape(-1, 2).astype(dt)
        X, Y = x[:, 0:1], x[:, 1:2]
        A[:, j * per + 0] = X * P[2] - P[0]
        A[:, j * per + 1] = Y * P[2] - P[1]
        if per == 3:
            A[:, j * per + 2] = X * P[1] - Y * P[0]
    return A.astype(np.float64)


def triangulate64(P1, P2, x1, x2, rows, build32=False):
    """numpy float64 SVD of the DLT rows; v = right singular vector of the smallest singular value (unit); the point
    (x, y, z) = float(v_k) / float(w) in float, as cc:159-165 divides the float 4 x n output.  Returns a dict with
    `p` (n, 3) float32, `v` (n, 4) float64, `sv` (n, 4)."""
    A = dlt_system(P1, P2, x1, x2, rows, build32)
    if len(A) == 0:
        return dict(p=np.zeros((0, 3), np.float32), v=np.zeros((0, 4)), sv=np.zeros((0, 4)))
    _, sv, Vt = np.linalg.svd(A)
    v = Vt[:, 3, :]
    v32 = v.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = v32[:, :3] / v32[:, 3:]
    return dict(p=p.astype(np.float32), v=v, sv=sv)


SVD_C = 64  # the constant of the SVD term below (see triangulation_bound)


def triangulation_bound(ref):
    """Per-coordinate bound on |p_got - p_ref| for an implementation that solves the same float64 system to float64
    accuracy and narrows and divides as cc:159-165 does.
    Derivation.  A backward-stable SVD (LAPACK's, or OpenCV's one-sided Jacobi that stops when every pair of columns is
    orthogonal to 10 DBL_EPSILON) returns the singular vector of the smallest singular value to within
        E = C * 2^-52 * sigma_1 / (sigma_3 - sigma_4)
    per component (the first-order perturbation of an invariant subspace: backward error ~eps sigma_1 over the gap to the
    nearest other singular value; C = SVD_C = 64 covers the Jacobi stopping test, the rounding of ~6 sweeps of rotations
    and the same again for the float64 reference).  For the ratio q_k = v_k / w of unit-vector components, a perturbation
    of at most E in every component moves q_k by at most  E (1 + |q_k|) / (|w| - E)  (no bound when E >= |w|: the point
    is not determined by the system).  Then float narrowing of v_k and w and the float division round q_k three times on
    each side: 3 u (|p_ref| + |p_got|) -- taken as 4 u for the second-order terms.  So
        |p_got - p_ref| <= E (1 + |p_ref|) / (|w| - E) + 4 u (|p_ref| + |p_got|)."""
    v, sv = ref["v"], ref["sv"]
    gap = sv[:, 2] - sv[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        E = np.where(gap > 0, SVD_C * EPS64 * sv[:, 0] / gap, np.inf)
        w = np.abs(v[:, 3])
        scale = np.where(w > E, E / np.maximum(w - E, 1e-300), np.inf)
        return scale[:, None] * (1 + np.abs(ref["p"].astype(np.float64)))


def triangulation_excess(ref, got):
    """max over points and coordinates of |got - ref| / bound (<= 1: within the bound); the finite pattern must agree.
    Points whose system does not determine them (infinite bound) only have to agree in finiteness."""
    p, g = ref["p"].astype(np.float64), np.asarray(got, np.float32).astype(np.float64)
    assert np.array_equal(np.isfinite(p), np.isfinite(g)), "finite in the reference where not on the other side"
    fin = np.isfinite(p) & np.isfinite(triangulation_bound(ref))
    if not fin.any():
        return 0.0
    b = triangulation_bound(ref)[fin] + 4 * U * (np.abs(p[fin]) + np.abs(g[fin])) + 1e-37
    return float((np.abs(g[fin] - p[fin]) / b).max())


# ---- UndistortFeaturePoints ----

def undistort64(pts, K, dist, iters=5):
    """cvUndistortPoints(src, dst, K, dist, R = NULL, P = K) in numpy float64, operation for operation (imgproc/src/
    undistort.cpp): coefficients widened from float, x = (x - cx) * (1 / fx), `iters` fixed-point iterations with
    icdist = 1 / (1 + ((k3 r2 + k1) r2 + k0) r2) (the rational numerator is 1 for five coefficients),
    deltaX = 2 p1 x y + p2 (r2 + 2 x x), deltaY = p1 (r2 + 2 y y) + 2 p2 x y, then K applied as
    (K00 x + K01 y + K02) * (1 / (K20 x + K21 y + K22)) and narrowed to float."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    A = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    k0, k1, k2, k3, k4 = np.asarray(dist, np.float32).astype(np.float64)
    fx, fy, cx, cy = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    x = (pts[:, 0].astype(np.float64) - cx) * (1.0 / fx)
    y = (pts[:, 1].astype(np.float64) - cy) * (1.0 / fy)
    x0, y0 = x.copy(), y.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + ((k4 * r2 + k1) * r2 + k0) * r2)
        dx = 2 * k2 * x * y + k3 * (r2 + 2 * x * x)
        dy = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = A[0, 0] * x + A[0, 1] * y + A[0, 2]
    yy = A[1, 0] * x + A[1, 1] * y + A[1, 2]
    ww = 1.0 / (A[2, 0] * x + A[2, 1] * y + A[2, 2])
    return np.c_[xx * ww, yy * ww].astype(np.float32)


def ulp_distance(a, b):
    """|a - b| in float32 units in the last place, per element (both finite)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


# ---- crafted geometry ----

IMAGE_W, IMAGE_H = 960, 600  # the reference calibration's principal point (482.8, 298.0) sits near this image's centre


def _backproject(K, uv, z):
    K = np.asarray(K, np.float64).reshape(3, 3)
    h = np.c_[uv, np.ones(len(uv))] @ np.linalg.inv(K).T
    return np.c_[h * z[:, None], np.ones(len(uv))]


def _project(P, X):
    x = (np.asarray(P, np.float64).reshape(3, 4) @ X.T).T
    return x[:, :2] / x[:, 2:]


def point_classes(P1, P2, K1, seed=0):
    """Left / right float32 pixels of crafted correspondences, and a label per point:
    near (z 0.3-2 m), mid (to 50 m), far (to 5 km), behind the camera, directions at infinity (x = P [d, 0], w ~ 0),
    noisy (+-0.5 px on both views and up to 20 px of vertical mismatch on the right: the 4-row and 6-row answers differ),
    left pixels at the image corners, just outside the image, exactly at (cx, cy) and on the axes through it."""
    rng = np.random.default_rng(seed)
    K1 = np.asarray(K1, np.float64).reshape(3, 3)
    cx, cy = K1[0, 2], K1[1, 2]
    L, R, lab = [], [], []

    def add(X, name, noise=0.0, vmis=0.0):
        x1, x2 = _project(P1, X), _project(P2, X)
        if noise:
            x1 = x1 + rng.uniform(-noise, noise, x1.shape)
            x2 = x2 + rng.uniform(-noise, noise, x2.shape)
        if vmis:
            x2[:, 1] += rng.uniform(-vmis, vmis, len(x2))
        L.append(x1.astype(np.float32))
        R.append(x2.astype(np.float32))
        lab.extend([name] * len(X))

    def inside(n):
        return np.c_[rng.uniform(20, IMAGE_W - 20, n), rng.uniform(20, IMAGE_H - 20, n)]

    add(_backproject(K1, inside(12), rng.uniform(0.3, 2, 12)), "near")
    add(_backproject(K1, inside(12), rng.uniform(2, 50, 12)), "mid")
    add(_backproject(K1, inside(10), np.exp(rng.uniform(np.log(50), np.log(5000), 10))), "far")
    add(_backproject(K1, inside(6), -rng.uniform(0.5, 20, 6)), "behind")
    d = _backproject(K1, inside(6), np.ones(6))
    d[:, 3] = 0.0
    add(d, "infinity")
    add(_backproject(K1, inside(12), rng.uniform(0.5, 30, 12)), "noisy", noise=0.5, vmis=20.0)
    corners = np.array([[0, 0], [IMAGE_W - 1, 0], [0, IMAGE_H - 1], [IMAGE_W - 1, IMAGE_H - 1]], np.float64)
    add(_backproject(K1, corners, rng.uniform(1, 20, 4)), "corner")
    outside = np.array([[-0.5, -0.5], [IMAGE_W + 0.5, IMAGE_H + 0.5], [-0.5, cy], [cx, IMAGE_H + 0.5]])
    add(_backproject(K1, outside, rng.uniform(1, 20, 4)), "outside")
    axes = np.array([[cx, cy], [cx, 17.0], [cx, IMAGE_H - 17.0], [23.0, cy], [IMAGE_W - 23.0, cy]])
    add(_backproject(K1, axes, rng.uniform(1, 20, 5)), "axis")
    x1, x2 = np.concatenate(L), np.concatenate(R)
    # (cx, cy) itself must reach the kernels as the float the calibration holds
    i = lab.index("axis")
    x1[i] = np.float32([cx, cy])
    return x1, x2, np.array(lab)


def descriptors_for(rng, n_left, right_of_left, n_right):
    """Left descriptors, random; right row k = left row right_of_left[k] with 1-8 bits flipped, or (-1) a random row; every
    other pair of rows at least 90 bits apart, so the ratio test (0.6) passes exactly the chosen pairs."""
    while True:
        dl = rng.integers(0, 256, (n_left, 32), dtype=np.uint8)
        dr = rng.integers(0, 256, (n_right, 32), dtype=np.uint8)
        for k, li in enumerate(right_of_left):
            if li >= 0:
                dr[k] = dl[li]
                for b in rng.choice(256, int(rng.integers(1, 9)), replace=False):
                    dr[k, b // 8] ^= np.uint8(1 << (b % 8))
        d = np.unpackbits(dr[:, None, :] ^ dl[None, :, :], axis=2).sum(2) if n_left and n_right else np.zeros((n_right, n_left))
        far = np.ones_like(d, bool)
        for k, li in enumerate(right_of_left):
            if li >= 0:
                far[k, li] = False
        if not (d[far] >= 90).all():
            continue
        if n_left < 2:
            return dl, dr
        dd = np.unpackbits(dl[:, None, :] ^ dl[None, :, :], axis=2).sum(2) + 256 * np.eye(n_left, dtype=np.int64)
        if dd.min() >= 90:
            return dl, dr
