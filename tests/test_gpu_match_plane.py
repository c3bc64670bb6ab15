"""k_match.hip held to tests/match_plane.py: every point of the distance plane 0 <= d1 <= d2 <= 256 through knn2 and the
ratio test at eleven ratios (one context each), the same through the host-pointer calls, the two designed rows at the
positions of a 10 300-row train set where tiles, lane halves, split chunks and 4096-row key ranges meet, and constructed
keep patterns through ratio_compact_kernel's compaction.  The reference is the plain one (unpackbits, lexsort, exact
rationals: proved right in tests/test_match_plane.py), the CPU oracle beside it where that is one more line."""
import numpy as np
import pytest

import match_plane as mp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RATIOS = list(mp.ACCEPTED)
SENT = -7     # fill of idx2 / dist2 / nmatches
SENT_B = 0xA5  # fill of every byte of the match records
F06 = mp.ACCEPTED["0.6f"]


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def plane():
    """Every set of the plane and its plain 2-NN, computed once: {(m, swapped): (q, t, idx, dist)}."""
    out = {}
    for m in range(mp.NBITS + 1):
        q = mp.query_set(m)
        for swapped in (False, True):
            t = mp.train_set(m, swapped)
            out[m, swapped] = (q, t) + mp.knn2(q, t)
    return out


def _context(capi, ratio, K=0):
    """A small context (the matcher needs no image): max_keypoints, the sets' row capacity, is nfeatures + 256 = 320
    unless given."""
    return capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=64, max_keypoints=K,
                                            nn_match_ratio=float(np.float32(ratio))))


def _pack(K, sets):
    desc = np.zeros((len(sets), K, 32), np.uint8)
    for i, s in enumerate(sets):
        desc[i, :len(s)] = s
    return desc, np.asarray([len(s) for s in sets], np.int32)


def _match_batch(capi, ctx, desc, counts, q, t):
    """One vsf_match_batch_dev launch into sentinel-filled outputs: (idx2, dist2, match bytes, nmatches) on the host."""
    dev = torch.device("cuda", 0)
    K, n = ctx.params.max_keypoints, len(q)
    assert desc.shape[1:] == (K, 32)
    d_desc, d_counts = torch.from_numpy(desc).to(dev), torch.from_numpy(counts).to(dev)
    d_q, d_t = torch.from_numpy(np.asarray(q, np.int32)).to(dev), torch.from_numpy(np.asarray(t, np.int32)).to(dev)
    out = (torch.full((n, K, 2), SENT, dtype=torch.int32, device=dev),
           torch.full((n, K, 2), SENT, dtype=torch.int32, device=dev),
           torch.full((n, K, 16), SENT_B, dtype=torch.uint8, device=dev),
           torch.full((n,), SENT, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ctx.match_batch_dev(d_desc.data_ptr(), d_counts.data_ptr(), K * 32, d_q.data_ptr(), d_t.data_ptr(), n,
                        *(x.data_ptr() for x in out))
    assert ctx.sync() == capi.VSF_OK
    return [x.cpu().numpy() for x in out]


def _check_pair(got, pr, nq, idx, dist, want, what, unsplit=True):
    """Pair `pr` of a batch against the plain 2-NN (None: not compared) and the plain matches; nothing written past either
    (a launch that splits the train sets clears all of dist2 first: only the unsplit form leaves rows past a set alone)."""
    g_idx, g_dist, g_m, g_n = got
    if idx is not None:
        np.testing.assert_array_equal(g_idx[pr, :nq], idx, err_msg="%s idx2" % what)
        np.testing.assert_array_equal(g_dist[pr, :nq], dist, err_msg="%s dist2" % what)
    assert (g_idx[pr, nq:] == SENT).all(), "%s: idx2 rows past the set written" % what
    assert not unsplit or (g_dist[pr, nq:] == SENT).all(), "%s: dist2 rows past the set written" % what
    assert int(g_n[pr]) == len(want), "%s nmatches %d, want %d" % (what, g_n[pr], len(want))
    rec = g_m[pr, :len(want)].reshape(-1).view(mp.DMATCH_DTYPE)
    if rec.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(rec != want)[0])
        raise AssertionError("%s match %d: %s, want %s" % (what, bad, rec[bad], want[bad]))
    assert (g_m[pr, len(want):] == SENT_B).all(), "%s: records written behind nmatches" % what


# ---- a. the whole plane in one launch per ratio ----
@pytest.mark.parametrize("name", RATIOS)
def test_whole_plane_one_launch(capi, plane, name):
    """Sets 0..256: the query sets; 257 + m: T_m; 514 + m: T_m swapped.  Pairs m and 257 + m match query set m against the
    straight and the swapped T_m: 514 pairs, the plane twice, in one launch (unsplit: the sets are one tile)."""
    r = mp.ACCEPTED[name]
    M = mp.NBITS + 1
    with _context(capi, r) as ctx:
        K = ctx.params.max_keypoints
        assert K >= M
        desc, counts = _pack(K, [plane[m, False][0] for m in range(M)] + [plane[m, False][1] for m in range(M)] +
                             [plane[m, True][1] for m in range(M)])
        q = np.concatenate([np.arange(M), np.arange(M)])
        t = np.concatenate([M + np.arange(M), 2 * M + np.arange(M)])
        got = _match_batch(capi, ctx, desc, counts, q, t)
    kept = {}
    for pr in range(2 * M):
        m, swapped = pr % M, pr >= M
        _, _, idx, dist = plane[m, swapped]
        want = mp.matches_from_knn2(idx, dist, 2, r)
        _check_pair(got, pr, M - m, idx, dist, want, "%s m=%d%s" % (name, m, " swapped" if swapped else ""))
        rec = got[2][pr, :len(want)].reshape(-1).view(mp.DMATCH_DTYPE)
        assert (rec["trainIdx"] == (0 if m == 0 or not swapped else 1)).all()  # the near row; m == 0: the lower index
        kept[pr] = {(int(d1), int(d1) + m) for d1 in rec["queryIdx"]}
    for half in (range(M), range(M, 2 * M)):  # straight, swapped: each the whole plane
        points = set().union(*(kept[pr] for pr in half))
        assert len(points) == sum(len(kept[pr]) for pr in half) == mp.KEPT[name]
        if name == "0.6f":
            assert {(3, 5), (6, 10), (150, 250)} <= points and (4, 6) not in points and (0, 0) not in points
        if name == "1.0":
            assert not any((d, d) in points for d in range(M)) and len(points) == mp.PLANE_POINTS - M
        if name in ("1.5", "255.5"):
            assert (0, 0) not in points and len(points) == mp.PLANE_POINTS - 1
        if name == "2**-31":
            assert points == {(0, d2) for d2 in range(1, M)}


# ---- b. the same through the host-pointer calls ----
@pytest.mark.parametrize("name", RATIOS)
def test_plane_through_host_pointer_calls(capi, oracle, plane, name):
    r = mp.ACCEPTED[name]
    with _context(capi, r) as ctx:
        for m in (0, 1, 2, 31, 32, 33, 100, 128, 255, 256):
            for swapped in (False, True):
                q, t, idx, dist = plane[m, swapped]
                what = "%s m=%d swapped=%d" % (name, m, swapped)
                gi, gd = ctx.knn2_hamming(q, t)
                np.testing.assert_array_equal(gi, idx, err_msg=what)
                np.testing.assert_array_equal(gd, dist, err_msg=what)
                got = ctx.get_matches(q, t)
                assert got.tobytes() == mp.matches_from_knn2(idx, dist, 2, r).tobytes(), what
                assert got.tobytes() == oracle.get_matches(q, t, ratio=float(np.float32(r))).tobytes(), what
        # one train row: a lone neighbour, and no matches (quirk Q6)
        q, t = plane[100, False][0], plane[100, False][1][1:]
        gi, gd = ctx.knn2_hamming(q, t)
        assert (gi == [0, -1]).all() and np.array_equal(gd[:, 0], np.arange(len(q)) + 100) and (gd[:, 1] == mp.INT_MAX).all()
        assert len(ctx.get_matches(q, t)) == 0
        # the query set of one m in ragged pieces, an empty one among them, against T_m in one call
        for m in (2, 100):  # m = 2 holds (3, 5); m = 100 holds (150, 250)
            q, t, idx, dist = plane[m, False]
            cuts = [0, 1, 1, 4, 64, 65, 151, len(q)]
            pieces = [q[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
            got = ctx.get_matches_multi(pieces, t)
            assert len(got) == len(pieces)
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                want = mp.matches_from_knn2(idx[a:b], dist[a:b], 2, r)
                assert got[i].tobytes() == want.tobytes(), "%s m=%d piece %d" % (name, m, i)
            assert sum(len(g) for g in got) == len(mp.matches_from_knn2(idx, dist, 2, r))


# ---- c. positions in a large train set ----
N_BIG = 10300  # 321 full tiles and one of 28 rows; beyond two 4096-row key ranges
# (index of the one designed row, index of the other): same tile and lane half (row & 4 equal), same tile and different
# halves, adjacent tiles, either side of a 128-row boundary, of a 512-row split chunk (what one pair of 10 300 rows is cut
# into), of both 4096-row key ranges, the first row, the last row of the partial tile, and far apart.
POSITIONS = [(0, 3), (0, 4), (3, 4), (31, 32), (127, 128), (511, 512), (4095, 4096), (8191, 8192), (0, 10299),
             (8192, 10299), (32, 4096), (128, 8191)]
SINGLES = [0, 4, 4096, 10299]
BAND_M = [0, 2, 4, 20, 100, 1, 33]  # m = 0: the designed rows are equal, the lower index wins across every boundary
BAND_D1 = 41                        # d1 <= 40, m <= 100: d2 <= 140, every filler (256 - d1 >= 216) strictly farther
SINGLE_D1 = list(range(BAND_D1)) + [95, 96, 97, 127, 128, 129, 256]  # one designed row: d2 = 256 - d1 is a filler's


def _big_train(near, far, m):
    t = np.tile(mp.thermo(0, mp.NBITS), (N_BIG, 1))
    t[near] = mp.thermo(0, 0)
    if far is not None:
        t[far] = mp.thermo(0, m)
    return t


@pytest.fixture(scope="module")
def big_sets():
    """[(what, queries, train, plain idx, plain dist)]: the designed rows at POSITIONS in both orders, then SINGLES."""
    band = {m: np.stack([mp.thermo(m, d1) for d1 in range(BAND_D1)]) for m in BAND_M}
    single_q = np.stack([mp.thermo(0, d1) for d1 in SINGLE_D1])
    out = []
    for i, (a, b) in enumerate(POSITIONS):
        m = BAND_M[i % len(BAND_M)]
        for near, far in ((a, b), (b, a)):
            t = _big_train(near, far, m)
            idx, dist = mp.knn2(band[m], t)
            if m > 0:  # the construction: (d1, d1 + m) at the designed rows, nearest first
                assert (idx == [near, far]).all() and np.array_equal(dist[:, 1] - dist[:, 0], np.full(BAND_D1, m))
            else:
                assert (idx == [min(a, b), max(a, b)]).all() and np.array_equal(dist[:, 0], dist[:, 1])
            out.append(("rows %d/%d m=%d" % (near, far, m), band[m], t, idx, dist))
    for pos in SINGLES:
        t = _big_train(pos, None, 0)
        idx, dist = mp.knn2(single_q, t)
        low = 1 if pos == 0 else 0  # the lowest-index filler
        assert (idx[:BAND_D1] == [pos, low]).all() and np.array_equal(dist[:BAND_D1, 1], 256 - np.arange(BAND_D1))
        out.append(("lone row %d" % pos, single_q, t, idx, dist))
    return out


def test_positions_in_a_large_train_set_split_form(capi, oracle, big_sets):
    """One pair at a time through the host-pointer calls: the train set is split over workgroups (512-row chunks here)
    and the chunks' packed keys merge by 64-bit CAS."""
    with _context(capi, F06) as ctx:
        for i, (what, q, t, idx, dist) in enumerate(big_sets):
            gi, gd = ctx.knn2_hamming(q, t)
            np.testing.assert_array_equal(gi, idx, err_msg=what)
            np.testing.assert_array_equal(gd, dist, err_msg=what)
            got = ctx.get_matches(q, t)
            assert got.tobytes() == mp.matches_from_knn2(idx, dist, len(t), F06).tobytes(), what
            if i % 6 == 0:
                oi, od = oracle.knn2_hamming(q, t)
                assert np.array_equal(oi, idx) and np.array_equal(od, dist), what
                assert got.tobytes() == oracle.get_matches(q, t).tobytes(), what


def test_designed_rows_either_side_of_a_128_row_split_chunk(capi):
    """1024 queries against 512 train rows: the one pair is cut four ways, into chunks of exactly 128 rows (the smallest
    the split makes).  The designed rows sit on both sides of each chunk boundary, in both orders, equal rows included."""
    rng = np.random.default_rng(128)
    with _context(capi, F06) as ctx:
        for m in (0, 2, 100):
            q = np.stack([mp.thermo(m, int(d1)) for d1 in rng.integers(0, BAND_D1, 1024)])
            for a, b in ((127, 128), (255, 256), (383, 384), (0, 511), (128, 383)):
                for near, far in ((a, b), (b, a)):
                    t = _big_train(near, far, m)[:512]
                    idx, dist = mp.knn2(q, t)
                    what = "rows %d/%d m=%d" % (near, far, m)
                    gi, gd = ctx.knn2_hamming(q, t)
                    np.testing.assert_array_equal(gi, idx, err_msg=what)
                    np.testing.assert_array_equal(gd, dist, err_msg=what)
                    assert ctx.get_matches(q, t).tobytes() == mp.matches_from_knn2(idx, dist, 512, F06).tobytes(), what


def test_positions_in_a_large_train_set_unsplit_form(capi, big_sets):
    """The same sets in one launch of 144 pairs: enough workgroups, so each walks a whole train set, 4096 rows per key
    range."""
    n_pairs = 144
    queries = {}  # the distinct query sets, by identity
    for _, q, _, _, _ in big_sets:
        queries.setdefault(id(q), q)
    q_slot = {k: i for i, k in enumerate(queries)}
    with _context(capi, F06, K=N_BIG + 4) as ctx:
        K = ctx.params.max_keypoints
        assert K >= N_BIG
        desc, counts = _pack(K, list(queries.values()) + [s[2] for s in big_sets])
        which = np.arange(n_pairs) % len(big_sets)
        q = np.asarray([q_slot[id(big_sets[w][1])] for w in which])
        t = len(queries) + which
        got = _match_batch(capi, ctx, desc, counts, q, t)
    for pr in range(n_pairs):
        what, qs, ts, idx, dist = big_sets[which[pr]]
        _check_pair(got, pr, len(qs), idx, dist, mp.matches_from_knn2(idx, dist, len(ts), F06), "pair %d %s" % (pr, what))


# ---- d. keep patterns for the compaction ----
KEEP_NQ = [1, 63, 64, 65, 255, 256, 257, 513, 1000]


def _keep_patterns(nq):
    rng = np.random.default_rng(nq)
    i = np.arange(nq)
    pats = {"none": np.zeros(nq, bool), "all": np.ones(nq, bool), "alternating": i % 2 == 0,
            "alternating from 1": i % 2 == 1, "64 kept 64 dropped": (i // 64) % 2 == 0,
            "64 dropped 64 kept": (i // 64) % 2 == 1, "random": rng.random(nq) < 0.5, "sparse": rng.random(nq) < 0.02}
    for s in sorted({0, 63, 64, 255, 256, 257, nq - 1}):
        if s < nq:
            pats["only %d" % s] = i == s
    return pats


@pytest.fixture(scope="module")
def keep_cases():
    """[(what, keep pattern, queries)] against T_100: a kept query is at (150, 250), ON the boundary (150 < 0.6f x 250 =
    150.000006), a dropped one at (151, 251)."""
    kept_q, dropped_q = mp.thermo(100, 150), mp.thermo(100, 151)
    assert mp.keep_exact(150, 250, F06) and not mp.keep_exact(151, 251, F06)
    return [("nq=%d %s" % (nq, name), keep, np.where(keep[:, None], kept_q, dropped_q))
            for nq in KEEP_NQ for name, keep in _keep_patterns(nq).items()]


def _keep_want(keep):
    want = np.zeros(int(keep.sum()), mp.DMATCH_DTYPE)
    want["queryIdx"], want["trainIdx"], want["distance"] = np.flatnonzero(keep), 0, 150.0
    return want


def test_compaction_keep_patterns_one_launch(capi, keep_cases):
    t100 = mp.train_set(100)
    with _context(capi, F06, K=1024) as ctx:
        desc, counts = _pack(ctx.params.max_keypoints, [c[2] for c in keep_cases] + [t100])
        n = len(keep_cases)
        got = _match_batch(capi, ctx, desc, counts, np.arange(n), np.full(n, n))
    for pr, (what, keep, q) in enumerate(keep_cases):
        want = mp.get_matches(q, t100, F06) if pr % 8 == 0 else _keep_want(keep)
        assert want.tobytes() == _keep_want(keep).tobytes()  # the plain reference says what the pattern says
        _check_pair(got, pr, len(q), None, None, want, what, unsplit=False)  # (107 pairs of 8 query tiles: split in two)
        assert (got[1][pr, :len(q), 0] == np.where(keep, 150, 151)).all() and (got[0][pr, :len(q)] == [0, 1]).all(), what
        rec = got[2][pr, :len(want)].reshape(-1).view(mp.DMATCH_DTYPE)
        assert (np.diff(rec["queryIdx"]) > 0).all(), what  # ascending query index


def test_compaction_keep_patterns_host_pointer_calls(capi, keep_cases):
    t100 = mp.train_set(100)
    with _context(capi, F06) as ctx:
        big = [c for c in keep_cases if len(c[1]) >= 257]
        for what, keep, q in big:
            assert ctx.get_matches(q, t100).tobytes() == _keep_want(keep).tobytes(), what
        got = ctx.get_matches_multi([c[2] for c in big], t100)
        for (what, keep, q), g in zip(big, got):
            assert g.tobytes() == _keep_want(keep).tobytes(), what
