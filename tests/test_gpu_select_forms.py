"""retainBest in the forms production runs (Context.debug_retain_best_form: the selection kernel's four instances, both
stages, the production memory plan), element for element against libstdc++'s nth_element + partition (oracle.retain_best).

Two lists: the plain matrix (sizes around every threshold of the code x n_points x key families), and the cases that
meet the depth limit (tests/select_cases.py; tests/test_select_killers.py shows on the CPU that they reach what they
claim).  Before the device is touched each case asserts, from the oracle's trace, where its array lives, whether it is
handed over to LDS and in which regime it meets the limit; the module ends with a check that every cell of that table ran.

Measured on an MI355X: see NOTES.md ("selection forms")."""
import numpy as np
import pytest

import select_cases as sc
from vision_slam_frontend_amd.capi import SELECT_FORMS

pytestmark = pytest.mark.gpu

FORMS = "ABCD"
_REF = {}     # (stage, case name, n, n_points) -> (key bits, ids): computed once, shared by the forms
_RAN = {}     # form -> cells reached on the device
_MOVED = {}   # (form, n) -> passes after which stage-1 matrix cases were handed over to LDS


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    capi.lib()
    c = capi.Context(capi.default_params(320, 240, max_images=1, nfeatures=100))
    yield c
    c.close()


def _reference(oracle, stage, name, keys, k):
    key = (stage, name, len(keys), k)
    if key not in _REF:
        rk, rid = oracle.retain_best(keys, k)
        _REF[key] = (rk.astype(np.uint32) if stage == 1 else rk.view(np.uint32), rid)
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _check(ctx, oracle, form, stage, name, keys, k, level_cap=None):
    what = "form %s stage %d %s n=%d n_points=%d" % (form, stage, name, len(keys), k)
    rk, rid = _reference(oracle, stage, name, keys, k)
    gk, gid, intact = ctx.debug_retain_best_form(form, stage, keys, k, level_cap=level_cap)
    assert len(gid) == len(rid), what
    np.testing.assert_array_equal(gid, rid, err_msg=what)
    np.testing.assert_array_equal(gk, rk, err_msg=what)
    assert intact, "the entries behind the array were written: " + what


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("form", FORMS)
def test_form_matches_libstdcxx_on_the_matrix(ctx, oracle, form, stage):
    entries = sc.lds_entries(form, stage)
    checked = 0
    for n in sc.matrix_sizes(form):
        for name, keys in sc.matrix_keys(stage, n, oracle):
            # the level's slices: roomy, exactly as long as the array ("ties"), or much longer ("equal")
            level_cap = n if name == "ties" else 3 * n + 100 if name == "equal" else None
            for k in sc.matrix_n_points(n):
                p = sc.path_of(form, stage, keys, k, oracle)
                if p is not None:  # (else a no-op or an empty result: no selection runs)
                    assert p.residency == ("lds" if n <= entries else "hbm")
                    assert p.migrates_at is None or (stage == 1 and n > entries and p.migrates_at >= 1)
                    if p.migrates_at is not None:
                        _MOVED.setdefault((form, n), set()).add(p.migrates_at)
                _check(ctx, oracle, form, stage, name, keys, k, level_cap)
                checked += 1
    assert checked > 900
    if stage == 1:  # the hand-over was exercised by ordinary inputs too, after one HBM pass and after several
        E = SELECT_FORMS[form][1]
        assert 1 in _MOVED[(form, E + 1)] and max(_MOVED[(form, 2 * E + 37)]) >= 2


def _run_killers(ctx, oracle, form):
    if form in _RAN:
        return _RAN[form]
    reached = set()
    for c in sc.killer_cases(form, oracle) + sc.mod256_cases(oracle):
        for k in c.n_points:
            p = sc.path_of(form, c.stage, c.keys, k, oracle)
            cell = sc.Cell(c.stage, p.residency, p.staged, p.regime)
            if c.cell is not None:
                assert cell == c.cell, (form, c.name, k, p)  # before the device is touched
            _check(ctx, oracle, form, c.stage, c.name, c.keys, k)
            reached.add(cell)
    _RAN[form] = reached
    return reached


@pytest.mark.parametrize("form", FORMS)
def test_form_matches_libstdcxx_at_the_depth_limit(ctx, oracle, form):
    """The killers with the n_points they were made for and with others, the embedded killers (limit met far below n, on
    an HBM array, through the wave scratch or after the hand-over) and the organ pipe (limit met on the last 7 elements)."""
    assert _run_killers(ctx, oracle, form)


def test_every_cell_of_the_table_ran_on_the_device(ctx, oracle):
    for form in FORMS:
        reached = _run_killers(ctx, oracle, form)  # (already run above: this only reads the record)
        missing = sc.required_cells(form) - reached
        assert not missing, (form, missing)
