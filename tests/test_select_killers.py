"""The selection's depth-limit paths, from the oracle alone (no GPU): the case list of tests/select_cases.py reaches the
regimes it claims, in every form of the selection kernel.  tests/test_gpu_select_forms.py runs the same list on the device.

The regimes (k_select.hip): R1 reg_introselect (range <= 64), R2 wave_introselect (65..256), R3 one lane in
par_introselect (> 256) -- each on an LDS-resident and on an HBM-resident array, and for stage 1 after the HBM -> LDS
hand-over as well."""
import numpy as np
import pytest

import select_cases as sc
from vision_slam_frontend_amd.capi import SELECT_FORMS

FORMS = "ABCD"


def test_adversary_meets_the_depth_limit_where_the_cpu_test_of_the_header_does(oracle):
    """killer_for_nth against the host std::nth_element: the ranges at which depth == 0 is met (tests/cpp/test_select.cc
    drives vsf_select.h with the same adversary); the nth it was made for does not matter away from n - 2."""
    want = {40: 21, 64: 41, 70: 47, 80: 57, 100: 77, 130: 103, 200: 173, 256: 225, 257: 226, 300: 269, 1000: 965,
            3100: 3057, 9300: 9249, 13000: 12949}
    for n, rng in want.items():
        keys = oracle.killer_for_nth(n, n // 2)
        assert sorted(np.unique(keys).astype(int).tolist())[0] == 0 and keys.max() == n - 1
        for nth in (n // 2, n // 7, 1):
            ranges, fb = oracle.nth_trace(keys, nth)
            assert fb == rng, (n, nth, fb)
            assert len(ranges) == 2 * (n.bit_length() - 1) and ranges[0] == n  # every pass the depth allows was a bad one
    keys = oracle.killer_for_nth(200, 198)
    assert oracle.nth_trace(keys, 198)[1] == -1  # (near n - 2 the selection ends before the depth does)


def test_trace_on_plain_inputs(oracle):
    rng = np.random.default_rng(3)
    ranges, fb = oracle.nth_trace(rng.uniform(-1, 1, 5000).astype(np.float32), 700)
    assert fb == -1 and ranges[0] == 5000 and all(a > b for a, b in zip(ranges, ranges[1:])) and ranges[-1] > 3
    ranges, fb = oracle.nth_trace(np.zeros(3, np.float32), 1)
    assert ranges == [] and fb == -1
    # the organ pipe of the old hook's test: the only one of its inputs that meets the limit, on its last 7 elements
    for k in (1, 2):
        ranges, fb = oracle.nth_trace(sc.organ(6000), k)
        assert fb == 7 and len(ranges) == 24
    assert oracle.nth_trace(sc.organ(6000), 6000 // 7)[1] == 689


def test_embedded_killer_first_pass_leaves_the_killer(oracle):
    for stage in (1, 2):
        keys, nth = sc.embedded_killer(oracle, stage, 3100, 290, 145)
        ranges, fb = oracle.nth_trace(keys, nth)
        assert ranges[:3] == [3100, 290, 289] and len(ranges) == 22 and fb == 290 - 1 - 2 * 20


@pytest.mark.parametrize("form", FORMS)
def test_case_list_reaches_what_it_claims(oracle, form):
    reached, many = set(), 0
    for c in sc.killer_cases(form, oracle):
        n = len(c.keys)
        if c.stage == 1:
            assert c.keys.min() >= 0 and c.keys.max() <= 255 and np.array_equal(c.keys, np.floor(c.keys))
        assert 0 < min(c.n_points) and max(c.n_points) < n
        for k in c.n_points:
            p = sc.path_of(form, c.stage, c.keys, k, oracle)
            got = sc.Cell(c.stage, p.residency, p.staged, p.regime)
            assert got == c.cell, (form, c.name, k, p)
            reached.add(got)
            if c.many:
                assert p.wg_passes >= 6, (c.name, p)
                many += 1
            if p.residency == "hbm" and p.regime == "R3" and not p.staged:
                assert k <= 16, "one lane on an HBM array: keep the heap small (%s)" % c.name
    assert reached >= sc.required_cells(form), sc.required_cells(form) - reached
    assert many >= 1


@pytest.mark.parametrize("form", FORMS)
def test_hand_over_happens_where_the_range_first_fits(oracle, form):
    """n slightly above ENTRIES: the range fits after one pass (E + 1), after two (E + 3), and after a dozen; an array
    that is still above ENTRIES when its depth runs out never moves."""
    E = SELECT_FORMS[form][1]
    for n, at in ((E + 1, 1), (E + 3, 2)):
        keys = sc.as_stage_keys(1, oracle.killer_for_nth(n, n // 2), "sat")
        p = sc.path_of(form, 1, keys, n // 2, oracle)
        assert p.migrates_at == at and p.staged and p.regime == "R3" and 256 < p.fallback <= E
    late = [sc.path_of(form, 1, c.keys, c.n_points[0], oracle) for c in sc.killer_cases(form, oracle)
            if c.stage == 1 and c.cell.staged and c.cell.regime == "R3"]
    assert max(p.migrates_at for p in late) >= 12
    keys = sc.as_stage_keys(1, oracle.killer_for_nth(E + 130, 5), "sat")
    p = sc.path_of(form, 1, keys, 5, oracle)
    assert p.migrates_at is None and p.fallback > E
    # stage 2 never moves, whatever its size
    assert sc.path_of(form, 2, sc.as_stage_keys(2, oracle.killer_for_nth(E + 1, 3)), 3, oracle).migrates_at is None


def test_issue_sizes_9300_and_13000_do_not_fit_their_forms(oracle):
    """Forms C and A hold 9 216 and 12 288 entries; the killers of 9 300 and 13 000 elements meet the limit at 9 249 and
    12 949, above them: no hand-over.  They run as never-staged R3 cases; the staged ones start at 9 250 and 12 330."""
    for form, n in (("C", 9300), ("A", 13000)):
        keys = sc.as_stage_keys(1, oracle.killer_for_nth(n, 5), "sat")
        p = sc.path_of(form, 1, keys, 5, oracle)
        assert p.migrates_at is None and p.regime == "R3" and p.fallback > SELECT_FORMS[form][1]
    p = sc.path_of("B", 1, sc.as_stage_keys(1, oracle.killer_for_nth(3100, 1550), "sat"), 1550, oracle)
    assert p.migrates_at == 15 and p.fallback == 3057


def test_what_the_adversary_mod_256_reaches(oracle):
    """Stage 1 compares one byte.  Up to 256 elements the adversary's values ARE bytes.  Beyond, taken mod 256, they
    stop being a killer (only 300 still meets the limit); saturated at 255 they stay one, because the bad passes only
    ever compare against the few dozen smallest values."""
    for n, want in sc.MOD256_REACH.items():
        keys = oracle.killer_for_nth(n, n // 2)
        for nth in (n // 2, 5):
            assert oracle.nth_trace(sc.as_stage_keys(1, keys, "mod"), nth)[1] == want, (n, nth)
            assert oracle.nth_trace(sc.as_stage_keys(1, keys, "sat"), nth) == oracle.nth_trace(keys, nth)


@pytest.mark.parametrize("form", FORMS)
def test_no_range_lies_beyond_the_mask_scratch(form):
    """par_introselect and the partition hand a range of more than maxw * 64 elements to one lane.  No form has such a
    range: the LDS masks cover ENTRIES >= n elements, the HBM masks ceil(level_cap / 64) words with level_cap >= n."""
    nt, entries, stage2 = SELECT_FORMS[form]
    maxw = {"A": 192, "B": 64, "C": 144, "D": 64}[form]
    assert entries // 64 <= maxw and (entries // 64) * 64 >= entries and stage2 <= entries
    for level_cap in (513, 1537, entries + 1, 2 * entries + 37, 70000):
        hbm_w = (level_cap + 63) // 64
        assert hbm_w * 64 >= level_cap and 6 * hbm_w + 2 <= level_cap  # (hbm_masks: always true where an array is in HBM)


def test_matrix_shapes():
    for form in FORMS:
        E = SELECT_FORMS[form][1]
        s = sc.matrix_sizes(form)
        assert {1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, E - 1, E, E + 1, 2 * E + 37} == set(s)
    assert sc.matrix_n_points(700) == [0, 1, 2, 14, 100, 350, 699, 700, 705]
