"""CPU: tests/kf_ref.py — the sequential reading of the keyframe rules (include/esvio_fe.h "keyframes") — against answers
worked out by hand from the rules' text, none of them taken from the library or from kf_ref itself."""
import os

import numpy as np
import pytest

import kf_ref as K
from esvio_amd import frontend as FE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C9 = [7, 17, 32, 46, 52, 46, 32, 17, 7]
# what an impulse at index 0 of a row weighs at outputs 0..4: r(p) = 0 only for p = 0, so nothing is doubled ...
W_AT_0 = [52, 46, 32, 17, 7]
# ... and at index 1, at outputs 0..5: r(-1) = r(1) = 1, so output o sums the taps that reach 1 and -1: c[5-o] + c[3-o]
W_AT_1 = [46 + 46, 52 + 32, 46 + 17, 32 + 7, 17, 7]


# ---- B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 1, 255])
def test_blur_leaves_a_constant_image_alone(v):
    assert np.array_equal(K.blur(np.full((11, 13), v, np.uint8)), np.full((11, 13), v, np.uint8))


@pytest.mark.parametrize("v", [255, 200, 3])
def test_blur_of_an_interior_impulse_is_the_rounded_tap_product(v):
    img = np.zeros((21, 23), np.uint8)
    img[10, 12] = v
    want = np.zeros((21, 23), np.int64)
    for j in range(9):
        for i in range(9):
            want[10 + j - 4, 12 + i - 4] = (v * C9[j] * C9[i] + 32768) >> 16
    assert np.array_equal(K.blur(img), want)


def _weights(n, at):
    """a row of n pixels: what an impulse at `at` (0, 1, n-2, n-1) weighs at every output"""
    w = np.zeros(n, np.int64)
    tab = W_AT_0 if at in (0, n - 1) else W_AT_1
    for o, c in enumerate(tab):
        w[o if at < 2 else n - 1 - o] = c
    return w


@pytest.mark.parametrize("ay", ["0", "1", "n-2", "n-1", "mid"])
@pytest.mark.parametrize("ax", ["0", "1", "n-2", "n-1", "mid"])
def test_blur_doubles_what_reflect_101_folds_back(ay, ax):
    H, W, v = 17, 19, 255
    pos = lambda a, n: {"0": 0, "1": 1, "n-2": n - 2, "n-1": n - 1, "mid": n // 2}[a]
    y, x = pos(ay, H), pos(ax, W)

    def weights(a, n, p):
        if a != "mid":
            return _weights(n, p)
        w = np.zeros(n, np.int64)
        w[p - 4:p + 5] = C9
        return w
    img = np.zeros((H, W), np.uint8)
    img[y, x] = v
    want = (v * np.outer(weights(ay, H, y), weights(ax, W, x)) + 32768) >> 16
    assert np.array_equal(K.blur(img), want)


def test_blur_commutes_with_the_transpose():
    img = np.random.default_rng(5).integers(0, 256, (23, 31), dtype=np.uint8)
    assert np.array_equal(K.blur(img.T), K.blur(img).T)


# ---- F ------------------------------------------------------------------------------------------------------------
def ring_image(centres, start, length, deltas, size=(15, 17), base=100):
    """base everywhere; for every centre (x, y) the `length` ring pixels from index `start` on (circular) get
    base + deltas[k]"""
    img = np.full(size, base, np.int32)
    for cx, cy in centres:
        for k in range(length):
            dx, dy = K.RING[(start + k) % 16]
            img[cy + dy, cx + dx] = base + deltas[k % len(deltas)]
    return img.astype(np.uint8)


def kept(img, t):
    xy, score, _ = K.fast(img, t)
    return {(int(x), int(y)): int(s) for (x, y), s in zip(xy, score)}


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("start", [0, 5, 12])  # (12: the arc runs over ring index 15 -> 0)
def test_fast_takes_an_arc_of_nine_and_no_arc_of_eight(sign, start):
    c = (8, 7)
    nine = ring_image([c], start, 9, [sign * 50])
    eight = ring_image([c], start, 8, [sign * 50])
    assert kept(nine, 10).get(c) == 49
    assert K.fast_scores(nine, 10)[0][c[1], c[0]]
    assert not K.fast_scores(eight, 10)[0][c[1], c[0]] and c not in kept(eight, 10)
    assert not K.fast_scores(eight, 0)[0][c[1], c[0]]


@pytest.mark.parametrize("sign", [1, -1])
def test_fast_score_is_the_arc_minimum_less_one(sign):
    c = (8, 7)
    img = ring_image([c], 3, 9, [sign * d for d in (60, 41, 37, 90, 55, 38, 37, 100, 64)])
    corner, score = K.fast_scores(img, 20)
    assert corner[7, 8] and score[7, 8] == 36
    assert kept(img, 36).get(c) == 36       # still a corner at barrier 36: 37 > 36
    assert c not in kept(img, 37) and not K.fast_scores(img, 37)[0][7, 8]


def test_fast_longer_arc_scores_its_best_window():
    # 11 bright pixels with differences 10 10 40 40 40 40 40 40 40 40 40: the best window of nine has minimum 40
    img = ring_image([(8, 7)], 0, 11, [10, 10, 40, 40, 40, 40, 40, 40, 40, 40, 40])
    assert K.fast_scores(img, 5)[1][7, 8] == 39


def test_fast_suppresses_two_adjacent_corners_of_equal_score():
    a, b = (7, 7), (8, 7)
    img = ring_image([a, b], 2, 9, [40])
    corner, score = K.fast_scores(img, 20)
    assert corner[7, 7] and corner[7, 8] and score[7, 7] == score[7, 8] == 39
    k = kept(img, 20)
    assert a not in k and b not in k


def test_fast_keeps_corners_at_the_border_of_three_and_none_inside_it():
    W = 17
    for cx in (3, W - 4):
        assert kept(ring_image([(cx, 7)], 0 if cx == 3 else 8, 9, [50]), 10).get((cx, 7)) == 49
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (15, W), dtype=np.uint8)
    for t in (0, 5):
        xy, _, _ = K.fast(img, t)
        assert len(xy) and xy[:, 0].min() >= 3 and xy[:, 0].max() <= W - 4 and xy[:, 1].min() >= 3 and xy[:, 1].max() <= 15 - 4
        assert np.array_equal(xy, xy[np.lexsort((xy[:, 0], xy[:, 1]))])  # raster order


def test_fast_never_keeps_a_corner_of_score_zero():
    img = ring_image([(8, 7)], 0, 9, [1])
    corner, score = K.fast_scores(img, 0)
    assert corner[7, 8] and score[7, 8] == 0 and (8, 7) not in kept(img, 0)


# ---- D ------------------------------------------------------------------------------------------------------------
def ramp(W, H=40):
    return np.tile(np.arange(W, dtype=np.uint8), (H, 1))


def hand_pattern(tests):
    """256 tests, all (0, 0, 0, 0) — equal pixels, bit 0 — except the given ones {i: (x1, y1, x2, y2)}"""
    p = np.zeros((4, 256), np.int32)
    for i, t in tests.items():
        p[:, i] = t
    return tuple(p)


def bits(desc):
    return np.unpackbits(np.asarray(desc, np.uint32).view(np.uint8), bitorder="little")


def test_brief_on_a_ramp_is_x1_below_x2():
    pat = FE.load_brief_pattern(os.path.join(GOLDEN, "brief_pattern.yml"))
    assert all(len(a) == 256 and np.abs(a).max() <= 24 for a in pat)
    d = K.brief(ramp(100, 60), [(50.0, 30.0), (24.0, 24.0), (75.0, 35.0)], pat)
    want = (pat[0] < pat[2]).astype(np.uint8)
    for k in range(3):
        assert np.array_equal(bits(d[k]), want)
    # bit i sits in word i >> 5 at bit i & 31
    for i in (0, 31, 32, 200, 255):
        assert ((int(d[0, i >> 5]) >> (i & 31)) & 1) == want[i]


def test_brief_float_addition_and_truncation():
    # test 0: x1 = -3 -> p.x + x1 = -0.5 -> (int) 0: inside; X2 = (int)3.5 = 3; 0 < 3: bit 1
    # test 40: the same at p.x + x1 = -1.0: outside: bit 0 (p.x = 2.0 below)
    pat = hand_pattern({0: (-3, 0, 1, 0), 40: (-3, 0, 1, 0)})
    assert bits(K.brief(ramp(30), [(2.5, 5.0)], pat)).nonzero()[0].tolist() == [0, 40]
    assert bits(K.brief(ramp(30), [(2.0, 5.0)], pat)).sum() == 0
    # 0.99999994f + 24 rounds to 25.0f: in a 25-wide image X2 = 25 is outside (bit 0); exactly it would be 24 (bit 1)
    pat = hand_pattern({7: (0, 0, 24, 0)})
    assert np.float32(0.99999994) < 1 and np.float32(0.99999994) + np.float32(24) == np.float32(25)
    assert bits(K.brief(ramp(25), [(np.float32(0.99999994), 5.0)], pat)).sum() == 0
    assert bits(K.brief(ramp(25), [(0.5, 5.0)], pat)).nonzero()[0].tolist() == [7]
    assert bits(K.brief(ramp(26), [(np.float32(0.99999994), 5.0)], pat)).nonzero()[0].tolist() == [7]
    # truncation is toward zero on both sides: y = -0.75 + 0 -> 0, inside
    assert bits(K.brief(ramp(26), [(0.5, -0.75)], pat)).nonzero()[0].tolist() == [7]


def test_brief_outside_and_non_finite_points_give_zero():
    pat = FE.load_brief_pattern(os.path.join(GOLDEN, "brief_pattern.yml"))
    pts = [(-100.0, 20.0), (50.0, 500.0), (np.nan, 20.0), (50.0, np.inf), (-np.inf, np.nan), (40000.0, 20.0), (50.0, -32768.0)]
    assert not K.brief(ramp(100, 60), pts, pat).any()
    assert not K.brief(np.full((60, 100), 9, np.uint8), [(50.0, 30.0)], pat).any()  # equal pixels


# ---- M ------------------------------------------------------------------------------------------------------------
def with_bits(n):
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d, bitorder="little").view("<u4")


@pytest.mark.parametrize("d, idx, dist, status", [(79, 0, 79, 1), (80, 0, 80, 0), (127, 0, 127, 0), (128, -1, 128, 0), (256, -1, 128, 0)])
def test_match_boundaries(d, idx, dist, status):
    got = K.match([np.zeros(8, np.uint32)], [with_bits(d)])
    assert (got[0][0], got[1][0], got[2][0]) == (idx, dist, status)


def test_match_takes_the_first_of_equal_distances_and_nothing_of_an_empty_set():
    T = [with_bits(90), with_bits(30), with_bits(200), np.roll(with_bits(30), 3), with_bits(31)]
    assert [int(K.hamming(np.zeros(8, np.uint32), T)[i]) for i in (1, 3)] == [30, 30]
    got = K.match([np.zeros(8, np.uint32), with_bits(200)], T)
    assert got[0].tolist() == [1, 2] and got[1].tolist() == [30, 0] and got[2].tolist() == [1, 1]
    got = K.match([np.zeros(8, np.uint32)], np.zeros((0, 8), np.uint32))
    assert (got[0][0], got[1][0], got[2][0]) == (-1, 128, 0)


# ---- the pattern file's parser ---------------------------------------------------------------------------------------
def test_pattern_parser():
    x1, y1, x2, y2 = FE.parse_brief_pattern("%YAML:1.0\nx1:\n  - 1\n  - -2\ny1: [3, 4]\nx2:\n  - 5\n  - 6\ny2:\n  - -7\n  - 8\n")
    assert (x1.tolist(), y1.tolist(), x2.tolist(), y2.tolist()) == ([1, -2], [3, 4], [5, 6], [-7, 8])
    for bad in ("x1:\n  - 1\n", "- 1\n", "x1: 7\ny1: []\nx2: []\ny2: []\n", "x1: [1]\ny1: []\nx2: []\ny2: []\n"):
        with pytest.raises(ValueError):
            FE.parse_brief_pattern(bad)
    raw = open(os.path.join(GOLDEN, "brief_pattern.yml"), "rb").read()
    assert len(raw) == 6977
