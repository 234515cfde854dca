"""numpy restatement of the plain C++ FAST of the reference's vendored library
(dependences/fast_neon-master: fast_corner_detect_9 / _10, fast_corner_score_10, fast_nonmax_3x3).

Test infrastructure, not product code.  tests/test_fast_ref.py checks it against outputs recorded from
the reference's own compiled functions (tests/golden/fast_ref_*.npz); that is what licenses its use on
inputs the fixtures do not hold.

    score_N(x, y) = max over the 16 start positions s of
                    max( min_{k<N}(p[s+k] - c), min_{k<N}(c - p[s+k]) ) - 1
the largest barrier at which the pixel still passes (c: centre byte, p: the 16 ring bytes).
"""
import numpy as np

# Bresenham circle of radius 3, (dx, dy), in the library's order
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2),
        (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
OUTSIDE = -2  # value of score_map outside the 3-pixel border (real scores are -1..254)


def score_map(img, arc):
    """int16 H x W map of score_arc; OUTSIDE in the 3-pixel border (and everywhere if a side is < 7)"""
    assert arc in (9, 10)
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape
    out = np.full((H, W), OUTSIDE, np.int16)
    if W < 7 or H < 7:
        return out
    c = img[3:H - 3, 3:W - 3].astype(np.int16)
    d = np.stack([img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx].astype(np.int16) - c for dx, dy in RING])
    d = np.concatenate([d, d[:arc]])  # circular
    best = np.full(c.shape, -256, np.int16)
    for s in range(16):
        w = d[s:s + arc]
        np.maximum(best, w.min(0), out=best)
        np.maximum(best, -w.max(0), out=best)
    out[3:H - 3, 3:W - 3] = best - 1
    return out


def detect(img, arc, barrier, smap=None):
    """fast_corner_detect_<arc>: int16 [n, 2] (x, y) in raster order, and their score_<arc> (int32 [n])"""
    if smap is None:
        smap = score_map(img, arc)
    ys, xs = np.nonzero((smap >= barrier) & (smap != OUTSIDE))
    xy = np.stack([xs, ys], 1).astype(np.int16).reshape(-1, 2)
    return xy, smap[ys, xs].astype(np.int32)


def nonmax_3x3(xy, scores, shape):
    """fast_nonmax_3x3: ascending indices of the corners none of whose 8 neighbours is a corner with a
    score greater than or equal to its own"""
    H, W = shape
    m = np.full((H + 2, W + 2), -(1 << 30), np.int64)
    x, y = xy[:, 0].astype(np.int64) + 1, xy[:, 1].astype(np.int64) + 1
    s = np.asarray(scores, np.int64)
    m[y, x] = s
    keep = np.ones(len(s), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= m[y + dy, x + dx] < s
    return np.nonzero(keep)[0].astype(np.int32)


def fast_corners(img, arc=10, barrier=20, nonmax=True):
    """what esvio_fe_fast_corners returns: (xy int16 [n, 2], score int32 [n] or None for arc 9, n_detected)"""
    xy, sc = detect(img, arc, barrier)
    n_det = len(xy)
    if nonmax:
        assert arc == 10
        idx = nonmax_3x3(xy, sc, np.asarray(img).shape)
        xy, sc = xy[idx], sc[idx]
    return xy, (sc if arc == 10 else None), n_det
