"""Inputs for the selection kernel's test hook (Context.debug_retain_best_form) and, from the oracle's trace of
std::nth_element alone, the path the device takes on them -- shared by tests/test_select_killers.py (CPU: the case list
reaches what it claims) and tests/test_gpu_select_forms.py (GPU: every case against oracle.retain_best).

The device (k_select.hip) restates std::__introselect pass for pass, so the sequence of ranges (last - first) is the
host's.  What differs is WHO runs a pass and WHERE the array lives:

  residency   stage 1 (32-bit candidates, one score byte compared): LDS when n <= ENTRIES of the form, else HBM;
              stage 2 ((Harris float, id) pairs): LDS when n <= 512, else HBM.
  migration   an HBM-resident stage-1 array moves into the idle LDS array at the first pass whose range is
              256 < range <= ENTRIES (with depth left); stage 2 has no such hand-over.
  regime      where the depth limit (2 * floor(log2 n) passes) is met, if it is met: range <= 64 in the register loop of
              one wave (R1), 65..256 in the single-wave loop (R2), above 256 on one lane of the workgroup loop (R3).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from vision_slam_frontend_amd.capi import SELECT_FORMS

WAVE_CUTOFF, REG_CUTOFF, STAGE2_ENTRIES = 256, 64, 512

# what a case reaches: residency "lds" | "hbm"; staged: the fallback happens after the HBM -> LDS hand-over;
# regime "R1" | "R2" | "R3"; many: at least 6 workgroup passes before the range came down to one wave
Cell = namedtuple("Cell", "stage residency staged regime")
Case = namedtuple("Case", "name stage keys n_points cell many")
Path = namedtuple("Path", "residency migrates_at staged regime fallback wg_passes")


def lds_entries(form: str, stage: int) -> int:
    return SELECT_FORMS[form][1] if stage == 1 else SELECT_FORMS[form][2]


def path_of(form: str, stage: int, keys: np.ndarray, n_points: int, oracle) -> Path | None:
    """The device's path through retainBest(keys, n_points) in this form and stage; None when no selection runs."""
    n = len(keys)
    if not 0 < n_points < n:
        return None
    ranges, fallback = oracle.nth_trace(keys, n_points)
    residency = "lds" if n <= lds_entries(form, stage) else "hbm"
    migrates_at = None
    if stage == 1 and residency == "hbm":
        for i, r in enumerate(ranges):  # (every traced pass has depth left)
            if r <= WAVE_CUTOFF:
                break
            if r <= SELECT_FORMS[form][1]:
                migrates_at = i
                break
    regime = None
    if fallback >= 0:
        assert fallback > 3
        regime = "R1" if fallback <= REG_CUTOFF else "R2" if fallback <= WAVE_CUTOFF else "R3"
    wg_passes = sum(1 for r in ranges if r > WAVE_CUTOFF)
    return Path(residency, migrates_at, migrates_at is not None and fallback >= 0, regime, fallback, wg_passes)


# ---- key material -------------------------------------------------------------------------------------------------
def as_stage_keys(stage: int, values: np.ndarray, how: str = "sat") -> np.ndarray:
    """Stage 2 compares floats: the values as they are.  Stage 1 compares one byte: the values mod 256 ("mod"), or
    saturated at 255 ("sat"), or scaled into 0..255 keeping their order ("scale")."""
    v = np.asarray(values, np.float64)
    if stage == 2:
        return v.astype(np.float32)
    if how == "mod":
        b = np.mod(v, 256)
    elif how == "sat":
        b = np.minimum(v, 255)
    else:
        b = np.floor(v * 256.0 / max(float(v.max()) + 1.0, 256.0)) if len(v) else v
    assert len(b) == 0 or (b.min() >= 0 and b.max() <= 255)
    return b.astype(np.float32)


def organ(n: int) -> np.ndarray:
    return np.minimum(np.arange(n), n - 1 - np.arange(n)).astype(np.float32)


def embedded_killer(oracle, stage: int, n: int, m: int, nth_in: int):
    """(keys, nth): n elements whose FIRST pass is a good one that leaves exactly an m-element killer as the range, so
    that the depth limit is met far below n.  Layout: n - m high fillers (all equal), a pivot value P in between at the
    middle position, and the killer's m (lower) values at the end: the median of a[1], a[n/2], a[n-1] is P, no element
    moves, the cut is n - m, and nth >= cut continues on the killer alone with 2 * floor(log2 n) - 1 passes left -- which
    is the depth the adversary played against.  For stage 1 the killer's values are saturated at 253 (P = 254, fillers
    255): only the few dozen smallest values are ever pivots, and saturation keeps their order."""
    assert 8 <= m < n // 2 - 1 and 0 <= nth_in < m
    depth = 2 * (int(n).bit_length() - 1) - 1
    k = oracle.killer_for_nth(m, nth_in, depth).astype(np.float64)
    if stage == 1:
        k, hi, p = np.minimum(k, 253), 255.0, 254.0
    else:
        hi, p = float(m + 1), float(m)
    x = np.full(n, hi, np.float32)
    x[n - m:] = k
    x[n // 2] = p
    return x, n - m + nth_in


def killer_cases(form: str, oracle):
    """The cases that are MEANT to reach a depth-limit regime, with the cell each claims.  n_points: the list to run."""
    E = SELECT_FORMS[form][1]
    cases = []

    def plain(stage, n, nth, how, residency, staged, regime, others=()):
        k = as_stage_keys(stage, oracle.killer_for_nth(n, nth), how)
        cases.append(Case("killer%d@%d/%s" % (n, nth, how), stage, k, [nth, *others],
                          Cell(stage, residency, staged, regime), False))

    def embedded(stage, n, m, residency, staged, regime):
        k, nth = embedded_killer(oracle, stage, n, m, m // 2)
        cases.append(Case("embedded%d/%d" % (m, n), stage, k, [nth, n - m + 3], Cell(stage, residency, staged, regime), False))

    for stage in (1, 2):
        # one wave from the start (n <= 256): R1 and R2; the byte keys of stage 1 are the adversary's own values here
        for n in (40, 64, 70, 80):
            plain(stage, n, n // 2, "mod", "lds", False, "R1", (1, n // 7))
        for n in (100, 130, 200, 256):
            plain(stage, n, n // 2, "mod", "lds", False, "R2", (1, n // 7))
    # 257: one workgroup pass, then R2;  300: R3 on an LDS array (269 < 512: stage 2 as well)
    for stage in (1, 2):
        plain(stage, 257, 128, "sat", "lds", False, "R2", (36,))
        plain(stage, 300, 150, "mod" if stage == 1 else "sat", "lds", False, "R3", (2, 42))
    plain(2, 512, 256, "sat", "lds", False, "R3", (3,))
    plain(1, E, E // 2, "sat", "lds", False, "R3", (5,))
    plain(1, E - 1, 7, "sat", "lds", False, "R3")
    # HBM-resident, fallback on the HBM array itself (one lane: n_points small, so the heap stays small)
    plain(2, 513, 5, "sat", "hbm", False, "R3", (2,))
    plain(2, 1000, 5, "sat", "hbm", False, "R3", (9,))
    plain(2, E + 1, 3, "sat", "hbm", False, "R3")
    plain(1, E + 130, 5, "sat", "hbm", False, "R3", (2,))  # still above ENTRIES when the depth runs out: never staged
    plain(1, 2 * E + 37, 4, "sat", "hbm", False, "R3")
    if form in "AC":
        plain(1, {"A": 13000, "C": 9300}[form], 5, "sat", "hbm", False, "R3", (2,))
    embedded(2, 600, 200, "hbm", False, "R2")
    embedded(2, 600, 90, "hbm", False, "R1")
    embedded(1, E + 28, 250, "hbm", False, "R2")  # from above ENTRIES straight to one wave: staged through the wave scratch
    embedded(1, E + 28, 100, "hbm", False, "R1")
    # ... and after the hand-over to LDS: the range first fits after a pass or two (E + 1, E + 3), or after a dozen
    # (the trace decides: B's 3 100 fits after 15 passes; 9 300 and 13 000 never come down to C's 9 216 and A's 12 288
    # entries within their 26 passes -- fallback ranges 9 249 and 12 949 -- so C and A start nearer, and those two sizes
    # join the never-staged cases above)
    start = {"A": 12330, "B": 3100, "C": 9250, "D": 1564}[form]
    for n in (E + 1, E + 3, start):
        plain(1, n, n // 2, "sat", "hbm", True, "R3", (5, n // 7))
    embedded(1, E + 28, 290, "hbm", True, "R2")
    embedded(1, 2 * E + 37, 288, "hbm", True, "R2")
    # R1 after many good workgroup passes: the organ pipe runs out of depth on its last few elements
    cases.append(Case("organ6000", 2, organ(6000), [1, 2], Cell(2, "hbm", False, "R1"), True))
    return cases


# The adversary's values taken mod 256, beyond 256 elements: the wrap-around makes ties of values the bad passes need
# apart, and the killer stops being one.  What the trace says these reach (fallback range, or -1), at nth = n // 2 and 5:
MOD256_REACH = {300: 269, 1000: -1, 3100: -1, 9300: -1, 13000: -1}


def mod256_cases(oracle):
    """The same inputs as cases WITHOUT a claim (cell None): they run on the device for what they are."""
    return [Case("killer%d@%d/mod" % (n, n // 2), 1, as_stage_keys(1, oracle.killer_for_nth(n, n // 2), "mod"),
                 [n // 2, 5], None, False) for n in MOD256_REACH if n > 300]


def required_cells(form: str):
    """What the case list has to reach in every form (tests/test_select_killers.py asserts it from the trace)."""
    req = set()
    for stage in (1, 2):
        for regime in ("R1", "R2", "R3"):
            req.add(Cell(stage, "lds", False, regime))
            req.add(Cell(stage, "hbm", False, regime))
    req.add(Cell(1, "hbm", True, "R2"))
    req.add(Cell(1, "hbm", True, "R3"))
    return req


# ---- the plain matrix ---------------------------------------------------------------------------------------------
def matrix_sizes(form: str):
    E = SELECT_FORMS[form][1]
    return [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, E - 1, E, E + 1, 2 * E + 37]


def matrix_n_points(n: int):
    return sorted({0, 1, 2, n // 50, n // 7, n // 2, n - 1, n, n + 5})


def matrix_keys(stage: int, n: int, oracle):
    """(name, keys) for one size: the key families of the issue; stage 1 gets them as bytes."""
    rng = np.random.default_rng(1000 * stage + n)
    out = [("uniform", rng.integers(0, 256, n).astype(np.float32) if stage == 1
            else rng.uniform(-1, 1, n).astype(np.float32)),
           ("ties", rng.integers(20, 61, n).astype(np.float32)),
           ("heavy_ties", rng.integers(20, 23, n).astype(np.float32)),
           ("equal", np.full(n, 7, np.float32)),
           ("sorted", as_stage_keys(stage, np.arange(n), "scale")),
           ("reverse", as_stage_keys(stage, np.arange(n)[::-1], "scale")),
           ("organ", as_stage_keys(stage, organ(n), "scale"))]
    return out
