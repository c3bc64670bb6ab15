"""The matcher's distance plane and its plain reference (no GPU, no oracle): what tests/test_match_plane.py proves right
and tests/test_gpu_match_plane.py holds k_match.hip to.

The plane.  thermo(lo, n) is the 256-bit descriptor with bits [lo, lo + n) set.  Against the two train rows
T_m = [thermo(0, 0), thermo(0, m)] the query thermo(m, d1) has the Hamming distances (d1, d1 + m) exactly, so the query
sets of m = 0..256 walk every point of 0 <= d1 <= d2 <= 256 once: 33 153 points, among them every pair on which
`dist1 < (double)ratio * dist2` (Frontend::GetMatches, slam_frontend.cc:521-538) could turn -- random and real
descriptors reach none of the 51 points where 0.6f and decimal 0.6 part.  m = 0 is the pure index tie (two equal train
rows: [0, 1]); the swapped sets put the far row first ([1, 0] for m > 0).

The reference.  Distances are sums of np.unpackbits(q ^ t); the two nearest come from np.lexsort((index, distance)),
batchDistance's rule "smaller distance, then lower train index" said outright; the ratio test is done in exact rationals
with the ratio taken from the float's own as_integer_ratio() -- never from vsf_params' ratio_num / ratio_shift, which are
code under test."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
INT_MAX = int(np.iinfo(np.int32).max)
NBITS = 256
PLANE_POINTS = (NBITS + 1) * (NBITS + 2) // 2  # 33 153

# name -> the float the caller hands to vsf_params_set_ratio
ACCEPTED = {
    "0.6f": np.float32(0.6), "0.75": np.float32(0.75), "0.5": np.float32(0.5), "1.0": np.float32(1.0),
    "1.5": np.float32(1.5), "0.8f": np.float32(0.8), "0.9f": np.float32(0.9), "0.1f": np.float32(0.1),
    "float32(1/3)": np.float32(1.0) / np.float32(3.0), "2**-31": np.float32(2.0 ** -31), "255.5": np.float32(255.5),
}
# kept points of the plane per ratio, from the exact-rational compare (conditions on the reference, not measurements)
KEPT = {"0.6f": 19891, "0.75": 24768, "0.5": 16512, "1.0": 32896, "1.5": 33152, "0.8f": 26470, "0.9f": 29721,
        "0.1f": 3431, "float32(1/3)": 11136, "2**-31": 256, "255.5": 33152}
# what vsf_params_set_ratio refuses: not in (0, 256), not finite, or more than 31 fractional bits
REFUSED = {"0": 0.0, "negative": -0.5, "256": 256.0, "nan": float("nan"), "inf": float("inf"),
           "0.001f": float(np.float32(0.001)), "1e-9f": float(np.float32(1e-9))}


def thermo(lo: int, n: int) -> np.ndarray:
    """256 bits with [lo, lo + n) set, bit i in byte i // 8 at 1 << (i % 8)."""
    assert 0 <= lo and 0 <= n and lo + n <= NBITS
    bits = np.zeros(NBITS, np.uint8)
    bits[lo:lo + n] = 1
    return np.packbits(bits, bitorder="little")


def train_set(m: int, swapped: bool = False) -> np.ndarray:
    t = np.stack([thermo(0, 0), thermo(0, m)])
    return t[::-1].copy() if swapped else t


def query_set(m: int) -> np.ndarray:
    """Row d1 is at (d1, d1 + m) from train_set(m), d1 = 0..256 - m."""
    return np.stack([thermo(m, d1) for d1 in range(NBITS - m + 1)])


def hamming(q: np.ndarray, t: np.ndarray) -> np.ndarray:
    """[nq, nt] int64 Hamming distances: sums of the bits of q ^ t (equal train rows -- the fillers of a large set -- are
    unpacked once)."""
    q, t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
    if len(q) == 0 or len(t) == 0:
        return np.zeros((len(q), len(t)), np.int64)
    rows, inverse = np.unique(t, axis=0, return_inverse=True)
    out = np.zeros((len(q), len(rows)), np.int64)
    step = max(1, (1 << 25) // (len(rows) * NBITS))  # ~32 MB of unpacked bits at a time
    for i in range(0, len(q), step):
        x = q[i:i + step, None, :] ^ rows[None, :, :]
        out[i:i + step] = np.unpackbits(x, axis=-1).sum(axis=-1, dtype=np.int64)
    return out[:, inverse.reshape(-1)]


def knn2(q: np.ndarray, t: np.ndarray):
    """knnMatch(k = 2): (idx [nq, 2], dist [nq, 2]) int32, ordered by (distance, train index); a neighbour that does not
    exist is index -1 at distance INT32_MAX (include/vsf.h)."""
    d = hamming(q, t)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), INT_MAX, np.int32)
    if nq and nt:
        index = np.broadcast_to(np.arange(nt, dtype=np.int64), d.shape)
        order = np.lexsort((index, d), axis=-1)[:, :2]  # last key is the primary one
        k = order.shape[1]
        idx[:, :k] = order
        dist[:, :k] = np.take_along_axis(d, order, axis=-1)
    return idx, dist


def ratio_exact(r) -> Fraction:
    """The reference's nn_match_ratio: a float widened to double, as the rational it is."""
    return Fraction(*float(np.float32(r)).as_integer_ratio())


def keep_exact(d1: int, d2: int, r) -> bool:
    return Fraction(int(d1)) < ratio_exact(r) * int(d2)


@lru_cache(maxsize=None)
def _keep_table(r: float) -> np.ndarray:
    ratio = Fraction(*r.as_integer_ratio())
    keep = np.zeros((NBITS + 1, NBITS + 1), bool)
    for d1 in range(NBITS + 1):
        for d2 in range(d1, NBITS + 1):
            keep[d1, d2] = Fraction(d1) < ratio * d2
    keep.setflags(write=False)
    return keep


def keep_table(r) -> np.ndarray:
    """keep_exact over the plane: [d1, d2] bool, False below the diagonal (d1 > d2 does not occur)."""
    return _keep_table(float(np.float32(r)))


def on_plane(n: int = NBITS) -> np.ndarray:
    """[d1, d2] bool: the points 0 <= d1 <= d2 <= n."""
    return np.triu(np.ones((NBITS + 1, NBITS + 1), bool)) & (np.arange(NBITS + 1) <= n)[None, :]


def matches_from_knn2(idx: np.ndarray, dist: np.ndarray, nt: int, r) -> np.ndarray:
    """The ratio test on a 2-NN answer: DMATCH records in ascending query index; fewer than two train rows give none
    (quirk Q6: the reference reads matches[i][1] out of bounds there)."""
    if nt < 2 or len(idx) == 0:
        return np.zeros(0, DMATCH_DTYPE)
    keep = keep_table(r)[dist[:, 0], dist[:, 1]]
    out = np.zeros(int(keep.sum()), DMATCH_DTYPE)
    out["queryIdx"] = np.flatnonzero(keep)
    out["trainIdx"] = idx[keep, 0]
    out["distance"] = dist[keep, 0].astype(np.float32)
    return out


def get_matches(q: np.ndarray, t: np.ndarray, r) -> np.ndarray:
    """Frontend::GetMatches(q, t, r), plainly."""
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    idx, dist = knn2(q, t)
    return matches_from_knn2(idx, dist, len(t), r)
