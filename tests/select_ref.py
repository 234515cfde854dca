"""The greedy min-distance selection every detector of the front-end ends in, restated sequentially in plain Python:
walk the candidates in order, skip one whose pixel is blocked, else accept it and block a filled disc round it, stop at
max_corners (feature_tracker.cpp:13-38 with cv::circle's disc; cv::goodFeaturesToTrack's distance pass with the open
Euclidean one).  Independent of oracle/ and of the library: tests/test_select_cases.py holds it to both oracles and to
the cv2 recordings, tests/test_select_edges_gpu.py holds the three selection kernels to it.

The keyword arguments after `out_base` of select() exist for the deliberately WRONG copies that test_select_cases.py
runs over the case families (a case family that no wrong copy disturbs checks nothing): their defaults are the rule.
"""
import numpy as np


def midpoint_halfwidths(r):
    """cv::circle(img, c, r, v, -1): the filled disc's half-width per |dy|, 0..r, by the midpoint recurrence of OpenCV's
    drawing.cpp (each visited (dx, dy) draws the spans of rows +-dy, half-width dx, and of rows +-dx, half-width dy)"""
    hw = [-1] * (r + 1)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def euclid_halfwidths(d, closed=False):
    """the open Euclidean disc dx*dx + dy*dy < d*d (closed: <=, a wrong copy) as half-widths per |dy|; the list ends
    with the last row that has a pixel"""
    d2 = float(d) * float(d)
    hw = []
    dy = 0
    while True:
        w = -1
        dx = 0
        while (dx * dx + dy * dy <= d2) if closed else (dx * dx + dy * dy < d2):
            w = dx
            dx += 1
        if w < 0:
            return hw
        hw.append(w)
        dy += 1


def halfwidths(kind, d):
    """kind 'circle': cv::circle of the integer radius d; 'euclid': the open disc of min_distance d"""
    if kind == "circle":
        return midpoint_halfwidths(int(d))
    assert kind == "euclid", kind
    return euclid_halfwidths(d)


def fill_disc(m, W, H, cx, cy, hw, clip=True):
    """m: bytearray of W*H bytes; the disc's rows, clipped to the sensor (clip False, a wrong copy: a row that leaves
    the sensor on one side goes on in the neighbouring row's bytes)"""
    r = len(hw) - 1
    for dy in range(-r, r + 1):
        y = cy + dy
        h = hw[-dy if dy < 0 else dy]
        if y < 0 or y >= H or h < 0:
            continue
        if clip:
            x0, x1 = max(cx - h, 0), min(cx + h, W - 1)
            if x1 < x0:
                continue
            a, b = y * W + x0, y * W + x1 + 1
        else:
            a, b = max(y * W + cx - h, 0), min(y * W + cx + h + 1, W * H)
        m[a:b] = b"\xff" * (b - a)


def select(W, H, xy, payload, hw, mask=None, stamp_pts=None, max_corners=None, out_base=0,
           clip=True, stamp_refused=False, cap_every=1, rounding=np.rint):
    """xy: uint32 x | y << 16; mask: (H, W) u8, 255 = blocked; stamp_pts: (k, 2) float32, rounded to nearest with ties
    to even like cvRound -> (points float32 (n, 2), payloads int32 (n), counts [accepted, out_base + accepted, total]).
    Wrong copies: clip (fill_disc), stamp_refused (a refused candidate blocks its disc too), cap_every (max_corners is
    looked at only before every cap_every-th candidate), rounding (np.trunc)."""
    xy = np.asarray(xy, np.uint32).reshape(-1)
    payload = np.asarray(payload, np.int32).reshape(-1)
    m = bytearray(W * H)
    if mask is not None:
        m[:] = np.where(np.asarray(mask, np.uint8).reshape(H, W) == 255, 255, 0).astype(np.uint8).tobytes()
    if stamp_pts is not None:
        for px, py in np.asarray(stamp_pts, np.float32).reshape(-1, 2):
            fill_disc(m, W, H, int(rounding(px)), int(rounding(py)), hw, clip)
    cap = len(xy) if max_corners is None else int(max_corners)
    pts, idx = [], []
    xs = (xy & 0xffff).tolist()
    ys = (xy >> 16).tolist()
    for i in range(len(xs)):
        if i % cap_every == 0 and len(pts) >= cap:
            break
        x, y = xs[i], ys[i]
        if m[y * W + x]:
            if stamp_refused:
                fill_disc(m, W, H, x, y, hw, clip)
            continue
        pts.append((x, y))
        idx.append(i)
        fill_disc(m, W, H, x, y, hw, clip)
    n = len(pts)
    return (np.array(pts, np.float32).reshape(-1, 2), payload[np.array(idx, np.int64)].astype(np.int32),
            np.array([n, out_base + n, len(xs)], np.int32))


def pack_xy(x, y):
    return (np.asarray(x, np.uint32) | (np.asarray(y, np.uint32) << np.uint32(16))).astype(np.uint32)
