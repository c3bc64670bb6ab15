"""Restatement of what the reference's debug images are drawn with (slam_frontend.cc:74-115), in plain Python: OpenCV 3.2
imgproc/src/drawing.cpp at thickness 1, LINE_8, shift 0, 8-bit 3-channel canvases.  Unpinned, like the rest of the
oracle: each routine follows the named OpenCV routine statement for statement, and tests/test_draw_ref.py checks it
against pixel sets derived by hand.

  cv_round      cvRound(float): round half to even (SSE2 cvtss2si in the default rounding mode)
  circle_points Circle() (drawing.cpp): the integer midpoint circle; its `inside` branch and its clipped branch both
                write exactly the points that lie inside the image
  clip_line     clipLine(Size2l, Point2l&, Point2l&)
  line_points   Line() -> LineIterator(img, pt1, pt2, 8, left_to_right = true), clipLine first when an end is outside
  line_minor    the device kernel's closed form of LineIterator's minor offset (csrc/k_draw.hip)
  render        GRAY2BGR of one image or two side by side (cv::hconcat), then the operations in order: later ones
                overwrite earlier ones
"""
from __future__ import annotations

import numpy as np

CIRCLE, LINE = 0, 1


def cv_round(v) -> int:
    return int(np.rint(np.float32(v)))


def circle_points(cx: int, cy: int, radius: int, width: int, height: int):
    """The pixels Circle(img, center, radius, color, fill = 0) writes, in write order (repeats included)."""
    out = []
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        y11, y12, y21, y22 = cy - dy, cy + dy, cy - dx, cy + dx
        x11, x12, x21, x22 = cx - dx, cx + dx, cx - dy, cx + dy
        for x, y in ((x11, y11), (x11, y12), (x12, y11), (x12, y12), (x21, y21), (x21, y22), (x22, y21), (x22, y22)):
            if 0 <= x < width and 0 <= y < height:
                out.append((x, y))
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return out


def _trunc(v: float) -> int:  # (int64) of a double: toward zero
    return int(v)


def clip_line(width: int, height: int, x1: int, y1: int, x2: int, y2: int):
    """clipLine: (inside, x1, y1, x2, y2)."""
    right, bottom = width - 1, height - 1
    if width <= 0 or height <= 0:
        return False, x1, y1, x2, y2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _trunc(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _trunc(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _trunc(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _trunc(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def line_points(x1: int, y1: int, x2: int, y2: int, width: int, height: int):
    """The pixels Line(img, pt1, pt2, color, 8) writes, in iteration order: LineIterator with pointers restated as (x, y)
    steps (bt_pix = one pixel along x, istep = one row along y)."""
    if not (0 <= x1 < width and 0 <= x2 < width and 0 <= y1 < height and 0 <= y2 < height):
        inside, x1, y1, x2, y2 = clip_line(width, height, x1, y1, x2, y2)
        if not inside:
            return []
    dx, dy = x2 - x1, y2 - y1
    s = -1 if dx < 0 else 0
    # left_to_right
    dx = (dx ^ s) - s
    dy = (dy ^ s) - s
    x1 ^= (x1 ^ x2) & s
    y1 ^= (y1 ^ y2) & s
    bt_pix, istep = (1, 0), (0, 1)
    s = -1 if dy < 0 else 0
    dy = (dy ^ s) - s
    if s:
        istep = (0, -1)
    if dy > dx:  # the conditional swaps
        dx, dy = dy, dx
        bt_pix, istep = istep, bt_pix
    err = dx - (dy + dy)
    plus_delta, minus_delta = dx + dx, -(dy + dy)
    plus_step, minus_step = istep, bt_pix
    count = dx + 1
    x, y = x1, y1
    out = []
    for _ in range(count):
        out.append((x, y))
        if err < 0:  # mask = err < 0 ? -1 : 0
            err += minus_delta + plus_delta
            x, y = x + minus_step[0] + plus_step[0], y + minus_step[1] + plus_step[1]
        else:
            err += minus_delta
            x, y = x + minus_step[0], y + minus_step[1]
    return out


def line_minor(major, minor, k):
    """Minor-axis offset after k major steps (0 <= minor <= major), as the device kernel computes it."""
    major, minor, k = np.asarray(major, np.int64), np.asarray(minor, np.int64), np.asarray(k, np.int64)
    return np.where(major > 0, (2 * minor * k + major - 1) // np.maximum(2 * major, 1), 0)


def render(src0: np.ndarray, src1, ops) -> np.ndarray:
    """GRAY2BGR canvas of src0 (| src1) with ops drawn in order; ops: (kind, x0, y0, x1, y1, (b, g, r))."""
    grey = src0 if src1 is None else np.concatenate([src0, src1], axis=1)
    canvas = np.repeat(grey[:, :, None], 3, axis=2).copy()
    h, w = grey.shape
    for kind, x0, y0, x1, y1, bgr in ops:
        if kind == CIRCLE:
            pts = circle_points(x0, y0, x1, w, h) if 0 <= x1 <= 65535 else []
        else:
            pts = line_points(x0, y0, x1, y1, w, h)
        for x, y in pts:
            canvas[y, x] = bgr[:3]
    return canvas


def stereo_ops(left_kp, right_kp, pairs, width: int, colours):
    """CreateStereoDebugImage's operations (cc:84-96): pairs are (right index, left index) in order, colours one (b, g, r)
    per pair."""
    ops = []
    for (ri, li), col in zip(pairs, colours):
        l, r = left_kp[int(li)], right_kp[int(ri)]
        lx, ly = cv_round(l["x"]), cv_round(l["y"])
        rx, ry = cv_round(np.float32(r["x"]) + np.float32(width)), cv_round(r["y"])
        ops += [(CIRCLE, lx, ly, 5, 0, (0, 0, 255)), (CIRCLE, rx, ry, 5, 0, (0, 0, 255)), (LINE, lx, ly, rx, ry, tuple(col))]
    return ops


def match_ops(past_kp, curr_kp, pairs):
    """CreateMatchDebugImage's operations (cc:105-113): pairs are (past index, current index) in order."""
    ops = []
    for pi, ci in pairs:
        a, b = past_kp[int(pi)], curr_kp[int(ci)]
        ax, ay = cv_round(a["x"]), cv_round(a["y"])
        ops += [(CIRCLE, ax, ay, 5, 0, (0, 0, 255)), (LINE, ax, ay, cv_round(b["x"]), cv_round(b["y"]), (0, 255, 0))]
    return ops


def rand_colours(rand, n: int):
    """cv::Scalar(rand() % 255, rand() % 255, rand() % 255) n times, the arguments evaluated right to left (GCC): the first
    draw is channel 2.  Unpinned: C++ leaves the order unspecified."""
    out = []
    for _ in range(n):
        c2 = rand() % 255
        c1 = rand() % 255
        c0 = rand() % 255
        out.append((c0, c1, c2))
    return out
