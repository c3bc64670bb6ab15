"""tests/match_plane.py is right and has teeth: the thermometer sets cover the distance plane 0 <= d1 <= d2 <= 256 exactly,
the exact-rational ratio test keeps the stated number of points per ratio, the reference's double compare agrees with it
everywhere (what entitles ratio_compact_kernel to integers), the near-miss compares are each told apart, the CPU oracle
answers the same byte for byte, and vsf_params_set_ratio turns every accepted float into that rational and refuses the
rest without touching the struct."""
import ctypes
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import match_plane as mp

ROOT = Path(__file__).resolve().parent.parent
RATIOS = list(mp.ACCEPTED)
D1 = np.arange(mp.NBITS + 1)[:, None]
D2 = np.arange(mp.NBITS + 1)[None, :]
PLANE = mp.on_plane()


def test_thermo_packs_little_endian():
    assert mp.thermo(0, 0).tolist() == [0] * 32 and mp.thermo(0, 256).tolist() == [255] * 32
    assert mp.thermo(0, 1).tolist() == [1] + [0] * 31 and mp.thermo(7, 2).tolist() == [0x80, 0x01] + [0] * 30
    assert mp.thermo(255, 1).tolist() == [0] * 31 + [0x80]


def test_construction_covers_the_plane_exactly_once():
    seen = np.zeros((mp.NBITS + 1, mp.NBITS + 1), np.int64)
    wrong = 0
    for m in range(mp.NBITS + 1):
        q, t = mp.query_set(m), mp.train_set(m)
        d = mp.hamming(q, t)
        want = np.stack([np.arange(len(q)), np.arange(len(q)) + m], axis=1)
        wrong += int((d != want).sum()) + int((mp.hamming(q, mp.train_set(m, swapped=True)) != want[:, ::-1]).sum())
        np.add.at(seen, (d[:, 0], d[:, 1]), 1)
    assert wrong == 0
    assert int(seen.sum()) == mp.PLANE_POINTS == 33153
    assert np.array_equal(seen == 1, PLANE) and not seen[~PLANE].any()  # every point, each exactly once


def test_plain_knn2_states_the_tie_rule():
    for m in (0, 1, 100, 256):
        q = mp.query_set(m)
        idx, dist = mp.knn2(q, mp.train_set(m))
        assert (idx == [0, 1]).all()  # m == 0: two equal rows, the lower index first
        assert np.array_equal(dist, np.stack([np.arange(len(q)), np.arange(len(q)) + m], axis=1))
        idx, dist_s = mp.knn2(q, mp.train_set(m, swapped=True))
        assert (idx == ([0, 1] if m == 0 else [1, 0])).all() and np.array_equal(dist_s, dist)
    idx, dist = mp.knn2(mp.query_set(250), mp.train_set(250)[:1])
    assert (idx == [0, -1]).all() and (dist[:, 1] == mp.INT_MAX).all()
    idx, dist = mp.knn2(mp.query_set(250), np.zeros((0, 32), np.uint8))
    assert (idx == -1).all() and (dist == mp.INT_MAX).all()
    assert len(mp.get_matches(mp.query_set(250), mp.train_set(250)[:1], 0.6)) == 0  # quirk Q6


@pytest.mark.parametrize("name", RATIOS)
def test_kept_counts(name):
    keep = mp.keep_table(mp.ACCEPTED[name])
    assert not keep[~PLANE].any()
    assert int(keep.sum()) == mp.KEPT[name]
    for d1, d2 in ((0, 0), (3, 5), (150, 250), (255, 256), (256, 256)):  # the table is keep_exact, point by point
        assert keep[d1, d2] == mp.keep_exact(d1, d2, mp.ACCEPTED[name])


def test_named_points():
    k = mp.keep_table(mp.ACCEPTED["0.6f"])
    assert k[3, 5] and k[6, 10] and k[150, 250] and not k[4, 6] and not k[151, 250]  # 3 < (double)0.6f * 5 is TRUE
    assert Fraction(150) < mp.ratio_exact(np.float32(0.6)) * 250 < Fraction(150) + Fraction(1, 100000)  # 150.000006
    assert not mp.keep_table(mp.ACCEPTED["1.0"])[np.arange(257), np.arange(257)].any()  # the 257 ties are dropped
    for name in ("1.5", "255.5"):  # only (0, 0) is dropped
        assert np.argwhere(PLANE & ~mp.keep_table(mp.ACCEPTED[name])).tolist() == [[0, 0]]
    k = mp.keep_table(mp.ACCEPTED["2**-31"])  # exactly the 256 points d1 == 0 < d2
    assert k[0, 1:].all() and int(k.sum()) == 256


@pytest.mark.parametrize("name", RATIOS)
def test_double_compare_is_the_exact_compare(name):
    """d1 < (double)r * d2 as the reference computes it (one rounded double product) against the rational compare."""
    r = float(np.float32(mp.ACCEPTED[name]))
    dbl = (D1.astype(np.float64) < r * D2.astype(np.float64)) & PLANE
    assert int((dbl != mp.keep_table(r)).sum()) == 0


# Points of the plane at which each near-miss of the compare answers differently from the exact one (counted from the
# reference; 0.6f: `<=` differs only at (0, 0), no other point has d1 * 2^23 == 5033165 * d2 with d2 <= 256).
LE_CATCHES = {"0.6f": 1, "0.75": 65, "0.5": 129, "1.0": 257, "1.5": 1, "0.8f": 1, "0.9f": 1, "0.1f": 1,
              "float32(1/3)": 1, "2**-31": 1, "255.5": 1}
F32_CATCHES = {"0.6f": 33, "0.8f": 51, "0.1f": 25, "float32(1/3)": 85}


@pytest.mark.parametrize("name", RATIOS)
def test_mutant_less_equal_is_rejected(name):
    num, den = float(np.float32(mp.ACCEPTED[name])).as_integer_ratio()
    le = np.array([[d1 <= d2 and d1 * den <= num * d2 for d2 in range(257)] for d1 in range(257)])
    diff = le != mp.keep_table(mp.ACCEPTED[name])
    assert int(diff.sum()) == LE_CATCHES[name] and diff[0, 0]


@pytest.mark.parametrize("name,decimal,first", [("0.6f", 0.6, [3, 5]), ("0.8f", 0.8, [4, 5])])
def test_mutant_decimal_ratio_is_rejected(name, decimal, first):
    dec = (D1.astype(np.float64) < decimal * D2.astype(np.float64)) & PLANE
    where = np.argwhere(dec != mp.keep_table(mp.ACCEPTED[name]))
    assert len(where) == 51 and where[0].tolist() == first
    assert (where[:, 0] * first[1] == where[:, 1] * first[0]).all()  # all on the line d1 / d2 == 3 / 5 (4 / 5)
    assert not dec[tuple(where.T)].any()  # the float is above the decimal: it keeps them, the decimal drops them


@pytest.mark.parametrize("name", sorted(F32_CATCHES))
def test_mutant_float32_product_is_rejected(name):
    r = np.float32(mp.ACCEPTED[name])
    f32 = (D1.astype(np.float32) < r * D2.astype(np.float32)) & PLANE
    assert (r * D2.astype(np.float32)).dtype == np.float32
    assert int((f32 != mp.keep_table(r)).sum()) == F32_CATCHES[name]


@pytest.fixture(scope="module")
def plane_knn2():
    """The plain 2-NN of every set of the plane: {(m, swapped): (q, t, idx, dist)}."""
    out = {}
    for m in range(mp.NBITS + 1):
        q = mp.query_set(m)
        for swapped in (False, True):
            t = mp.train_set(m, swapped)
            out[m, swapped] = (q, t) + mp.knn2(q, t)
    return out


def test_oracle_knn2_equals_plain(oracle, plane_knn2):
    for (m, swapped), (q, t, idx, dist) in plane_knn2.items():
        oi, od = oracle.knn2_hamming(q, t)
        assert np.array_equal(oi, idx) and np.array_equal(od, dist), (m, swapped)
        assert oi.dtype == idx.dtype and od.dtype == dist.dtype


@pytest.mark.parametrize("name", RATIOS)
def test_oracle_get_matches_equals_plain(oracle, plane_knn2, name):
    r = float(np.float32(mp.ACCEPTED[name]))
    assert oracle.DMATCH_DTYPE == mp.DMATCH_DTYPE
    kept = 0
    for (m, swapped), (q, t, idx, dist) in plane_knn2.items():
        want = mp.matches_from_knn2(idx, dist, len(t), r)
        got = oracle.get_matches(q, t, ratio=r)
        assert got.tobytes() == want.tobytes(), (name, m, swapped)
        kept += len(want)
    assert kept == 2 * mp.KEPT[name]


def test_plain_get_matches_is_knn2_then_ratio(plane_knn2):
    q, t, idx, dist = plane_knn2[100, True]
    m = mp.get_matches(q, t, np.float32(0.6))
    assert m.tobytes() == mp.matches_from_knn2(idx, dist, 2, np.float32(0.6)).tobytes()
    assert m["queryIdx"].tolist() == list(range(151)) and (m["trainIdx"] == 1).all() and (m["imgIdx"] == 0).all()
    assert m["distance"].tolist() == [float(d) for d in range(151)]  # (150, 250) is the last kept, (151, 251) is not


# ---- vsf_params_set_ratio: pure host code, needs only the library to load ----
@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from vision_slam_frontend_amd import capi
    if not capi.LIB_PATH.exists():
        g.build()
    return capi


@pytest.mark.parametrize("name", RATIOS)
def test_set_ratio_is_the_floats_own_rational(capi, name):
    r = float(np.float32(mp.ACCEPTED[name]))
    p = capi.default_params(640, 480)
    p.ratio_num, p.ratio_shift = 12345, 7
    assert capi.lib().vsf_params_set_ratio(ctypes.byref(p), ctypes.c_float(r)) == capi.VSF_OK
    assert Fraction(p.ratio_num, 2 ** p.ratio_shift) == Fraction(r) == mp.ratio_exact(r)
    assert p.ratio_num % 2 == 1 or p.ratio_shift == 0  # lowest terms
    assert p.ratio_shift <= 31
    # the kernel's compare on these two integers is the exact compare on the whole plane
    ints = ((D1.astype(object) << int(p.ratio_shift)) < int(p.ratio_num) * D2.astype(object)) & PLANE
    assert np.array_equal(ints.astype(bool), mp.keep_table(r))
    assert int(p.ratio_num) * 256 < 2 ** 64 and 256 << int(p.ratio_shift) < 2 ** 64  # both sides fit the kernel's uint64
    q = capi.default_params(640, 480, nn_match_ratio=r)
    assert (q.ratio_num, q.ratio_shift) == (p.ratio_num, p.ratio_shift)


def test_set_ratio_known_pairs(capi):
    got = {}
    for name in ("0.6f", "0.75", "1.0", "1.5", "2**-31", "255.5"):
        p = capi.default_params(640, 480, nn_match_ratio=float(mp.ACCEPTED[name]))
        got[name] = (p.ratio_num, p.ratio_shift)
    assert got == {"0.6f": (5033165, 23), "0.75": (3, 2), "1.0": (1, 0), "1.5": (3, 1), "2**-31": (1, 31),
                   "255.5": (511, 1)}


@pytest.mark.parametrize("name", list(mp.REFUSED))
def test_set_ratio_refuses_and_leaves_the_struct_alone(capi, name):
    p = capi.default_params(640, 480, nn_match_ratio=0.75)
    before = bytes(p)
    st = capi.lib().vsf_params_set_ratio(ctypes.byref(p), ctypes.c_float(mp.REFUSED[name]))
    assert st == capi.VSF_ERR_INVALID_ARG
    assert (p.ratio_num, p.ratio_shift) == (3, 2) and bytes(p) == before
    with pytest.raises(capi.VsfError):
        capi.default_params(640, 480, nn_match_ratio=mp.REFUSED[name])


def test_refused_floats_are_refused_for_the_stated_reason():
    """0.001f and 1e-9f lie in (0, 256) and are finite: what refuses them is the 31-bit limit on the fraction."""
    for name in ("0.001f", "1e-9f"):
        r = mp.REFUSED[name]
        assert 0 < r < 256 and Fraction(r).denominator > 2 ** 31
    assert Fraction(float(mp.ACCEPTED["2**-31"])).denominator == 2 ** 31  # the last shift that is accepted
