"""The debug images' drawing restatement (tests/draw_ref.py) against pixel sets derived by hand from OpenCV 3.2's
drawing.cpp, and the device kernel's closed-form line (csrc/k_draw.hip) against LineIterator's iteration for every
|dx|, |dy| <= 300.  CPU only."""
import numpy as np
import pytest

import draw_ref as D


def test_cv_round_is_half_to_even():
    vals = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.4999, 2.5001, 639.5, 640.5]
    assert [D.cv_round(v) for v in vals] == [0, 2, 2, 0, -2, -2, 2, 3, 640, 640]


def test_radius5_ring():
    # Circle(): (dx, dy) runs (5, 0), (4, 1), (4, 2), (4, 3) and stops at (3, 4); eight points per step
    offs = {(5, 0), (-5, 0), (0, 5), (0, -5)}
    for a, b in ((4, 1), (4, 2), (4, 3)):
        for sa in (1, -1):
            for sb in (1, -1):
                offs |= {(sa * a, sb * b), (sa * b, sb * a)}
    assert len(offs) == 28
    got = D.circle_points(20, 20, 5, 64, 64)
    assert set(got) == {(20 + x, 20 + y) for x, y in offs}
    # the same ring at a corner keeps what lies inside: x, y >= 0
    corner = {(5, 0), (0, 5), (4, 1), (1, 4), (4, 2), (2, 4), (4, 3), (3, 4)}
    assert set(D.circle_points(0, 0, 5, 10, 10)) == corner
    assert D.circle_points(-20, 3, 5, 10, 10) == []
    assert set(D.circle_points(3, 3, 0, 10, 10)) == {(3, 3)}


OCTANTS = {  # from (10, 10); derived step by step from LineIterator (err = dx - 2dy, +2dx on a minor step, -2dy always)
    (15, 12): [(10, 10), (11, 10), (12, 11), (13, 11), (14, 12), (15, 12)],
    (12, 15): [(10, 10), (10, 11), (11, 12), (11, 13), (12, 14), (12, 15)],
    # left_to_right: the walk starts at the left end, so this is not the mirror image of the one above
    (8, 15): [(8, 15), (8, 14), (9, 13), (9, 12), (10, 11), (10, 10)],
    (5, 12): [(5, 12), (6, 12), (7, 11), (8, 11), (9, 10), (10, 10)],
    (5, 8): [(5, 8), (6, 8), (7, 9), (8, 9), (9, 10), (10, 10)],
    (8, 5): [(8, 5), (8, 6), (9, 7), (9, 8), (10, 9), (10, 10)],
    (12, 5): [(10, 10), (10, 9), (11, 8), (11, 7), (12, 6), (12, 5)],
    (15, 8): [(10, 10), (11, 10), (12, 9), (13, 9), (14, 8), (15, 8)],
}


@pytest.mark.parametrize("end", sorted(OCTANTS))
def test_line_octants(end):
    assert D.line_points(10, 10, end[0], end[1], 32, 32) == OCTANTS[end]


def test_line_axes_and_diagonals():
    assert D.line_points(2, 3, 6, 3, 10, 10) == [(x, 3) for x in range(2, 7)]
    assert D.line_points(6, 3, 2, 3, 10, 10) == [(x, 3) for x in range(2, 7)]
    assert D.line_points(3, 6, 3, 2, 10, 10) == [(3, y) for y in range(6, 1, -1)]
    assert D.line_points(0, 0, 4, 4, 10, 10) == [(k, k) for k in range(5)]
    assert D.line_points(4, 0, 0, 4, 10, 10) == [(k, 4 - k) for k in range(5)]
    assert D.line_points(7, 7, 7, 7, 10, 10) == [(7, 7)]


def test_line_endpoints_outside():
    # both ends beyond the sides: clipLine moves them onto x = 0 and x = 9
    assert D.line_points(-5, 5, 14, 5, 10, 10) == [(x, 5) for x in range(10)]
    # across two corners: y = 0 and y = 9 first
    assert D.line_points(-3, -3, 12, 12, 10, 10) == [(k, k) for k in range(10)]
    # clipLine truncates toward zero: y1 += (int)(4 * 3 / 9.) = 1, so the walk starts at (0, 2), not on the true line
    assert D.line_points(-4, 1, 5, 4, 10, 10) == [(0, 2), (1, 2), (2, 3), (3, 3), (4, 4), (5, 4)]
    # both ends left of the image: nothing
    assert D.line_points(-5, -5, -1, 20, 10, 10) == []
    assert D.line_points(-5, 20, 30, 25, 10, 10) == []


def test_render_last_writer_wins():
    g = np.full((8, 8), 7, np.uint8)
    ops = [(D.LINE, 0, 3, 7, 3, (1, 2, 3)), (D.LINE, 3, 0, 3, 7, (4, 5, 6))]
    c = D.render(g, None, ops)
    assert tuple(c[3, 3]) == (4, 5, 6) and tuple(c[3, 0]) == (1, 2, 3) and tuple(c[0, 0]) == (7, 7, 7)
    c2 = D.render(g, g, ops[::-1])
    assert c2.shape == (8, 16, 3) and tuple(c2[3, 3]) == (1, 2, 3)


def _iterate_all(dx, dy, steps):
    """LineIterator (left_to_right, 8-connected) vectorised over many lines from (0, 0): positions after 0..steps-1 steps."""
    s = np.where(dx < 0, -1, 0)
    x0 = np.where(s < 0, dx, 0)
    y0 = np.where(s < 0, dy, 0)
    adx = (dx ^ s) - s
    dyl = (dy ^ s) - s
    s2 = np.where(dyl < 0, -1, 0)
    ady = (dyl ^ s2) - s2
    ystep = np.where(s2 < 0, -1, 1)
    swap = ady > adx
    major, minor = np.where(swap, ady, adx), np.where(swap, adx, ady)
    err = major - 2 * minor
    # major step: x + 1, or y +- 1 when swapped; minor step: the other
    mx, my = np.where(swap, 0, 1), np.where(swap, ystep, 0)
    nx, ny = np.where(swap, 1, 0), np.where(swap, 0, ystep)
    x, y = x0.copy(), y0.copy()
    xs, ys = [x.copy()], [y.copy()]
    for _ in range(steps - 1):
        neg = err < 0
        err = err - 2 * minor + np.where(neg, 2 * major, 0)
        x = x + mx + np.where(neg, nx, 0)
        y = y + my + np.where(neg, ny, 0)
        xs.append(x.copy())
        ys.append(y.copy())
    return np.stack(xs, 1), np.stack(ys, 1), x0, y0, major, minor, swap, ystep


def test_closed_form_minor_offset_exhaustive():
    r = np.arange(-300, 301, dtype=np.int64)
    k = np.arange(301, dtype=np.int64)[None, :]
    rng = np.random.default_rng(5)
    for block in range(0, len(r), 40):  # (40 x 601 lines at a time: ~60 MB per array)
        dx, dy = [a.reshape(-1) for a in np.meshgrid(r[block:block + 40], r, indexing="ij")]
        xs, ys, x0, y0, major, minor, swap, ystep = _iterate_all(dx, dy, 301)
        m = D.line_minor(major[:, None], minor[:, None], k)
        kx = np.where(swap[:, None], x0[:, None] + m, x0[:, None] + k)
        ky = np.where(swap[:, None], y0[:, None] + ystep[:, None] * k, y0[:, None] + ystep[:, None] * m)
        valid = k <= major[:, None]
        assert np.array_equal(np.where(valid, kx, 0), np.where(valid, xs, 0))
        assert np.array_equal(np.where(valid, ky, 0), np.where(valid, ys, 0))
        # the walk ends on the far endpoint
        end = np.arange(len(dx)), major
        assert np.array_equal(xs[end], np.where(dx < 0, 0, dx)) and np.array_equal(ys[end], np.where(dx < 0, 0, dy))
        # and the vectorised iteration is the scalar restatement's, on a sample
        for i in rng.choice(len(dx), 20, replace=False):
            want = D.line_points(300, 300, 300 + int(dx[i]), 300 + int(dy[i]), 601, 601)
            got = [(300 + int(xs[i, j]), 300 + int(ys[i, j])) for j in range(int(major[i]) + 1)]
            assert got == want
