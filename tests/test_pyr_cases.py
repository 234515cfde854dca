"""The inputs of tests/pyr_cases.py reach the edges they are for — shown from the reference alone, without a GPU:
level sizes, dense surfaces without a flat byte, saturated derivatives and pyrDown ties, every behaviour of CLAHE's clip
step, and the levels whose 24-pixel ring takes a second reflection (where the device's one-reflection helper would
return a negative source index)."""
import numpy as np
import pytest

import pyr_cases as PC

ALL_SIZES = list(PC.FOUR_LEVEL) + list(PC.SMALL)


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_level_sizes(oracle, W, H):
    want = PC.level_sizes(W, H)
    assert oracle.pyr_levels(W, H) + 1 == len(want)
    pyr = PC.expected_pyramid(oracle, np.zeros((H, W), np.uint8))
    assert [(im.shape[1] - 2 * PC.PAD, im.shape[0] - 2 * PC.PAD) for im, _ in pyr] == list(want)
    assert all(dv.shape == im.shape + (2,) for im, dv in pyr)


def test_what_the_four_level_sizes_reach():
    # the fused kernels' tiles are 8 x 4 pixels of level 3
    w3, h3 = PC.FOUR_LEVEL[(169, 169)][3]
    assert (w3 % 8, h3 % 4) == (6, 2) and all(w % 2 and h % 2 for w, h in PC.FOUR_LEVEL[(169, 169)][:3])
    assert PC.FOUR_LEVEL[(192, 176)][3][0] % 8 == 0
    assert 169 % 4 and not 176 % 4  # k_time_surface / k_time_surface4
    # CLAHE: both sides are extended as soon as one is no multiple of 8
    assert PC.clahe_geometry(176, 176)[:2] == (176, 176)
    assert PC.clahe_geometry(176, 169)[:2] == (184, 176) and PC.clahe_geometry(169, 176)[:2] == (176, 184)
    assert PC.clahe_geometry(346, 260)[:2] == (352, 264) and PC.clahe_geometry(352, 264)[:2] == (352, 264)


@pytest.mark.parametrize("W,H", list(PC.FOUR_LEVEL))
def test_dense_surfaces_have_no_flat_byte_and_busy_edges(oracle, W, H):
    fr = PC.dense_frames(W, H)
    assert len(fr) >= 3
    seen = set()
    for k, f in enumerate(fr):
        _, _, _, _, ts = PC.oracle_surfaces(oracle, W, H, f, k)
        for cam in range(2):
            assert not np.isin(ts[cam], (127, 128)).any()
            seen.add(ts[cam].tobytes())
            for im, _ in PC.expected_pyramid(oracle, ts[cam]):
                cur = im[PC.PAD:-PC.PAD, PC.PAD:-PC.PAD]
                for edge in (cur[0], cur[1], cur[-2], cur[-1], cur[:, 0], cur[:, 1], cur[:, -2], cur[:, -1]):
                    assert len(np.unique(edge)) >= 2
    assert len(seen) == 2 * len(fr)  # different frames: a ring left over from another one holds other bytes


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_extremes_saturate_the_derivatives_and_tie_the_rounding(oracle, W, H):
    fr = PC.extremes_frames(W, H)
    top, edge_hit, corner_hit = 0, np.zeros(4, bool), np.zeros(4, bool)
    for f in fr:
        for img in (f.left, f.right):
            dv = oracle.scharr(img).astype(np.int64)
            top = max(top, int(np.abs(dv).max()))
            edge_hit |= [bool(dv[0].any()), bool(dv[-1].any()), bool(dv[:, 0].any()), bool(dv[:, -1].any())]
            # At a corner pixel both derivatives are 0 whatever the image is: reflect-101 makes x - 1 and x + 1 (y - 1 and
            # y + 1) the same pixel.  What a wrong border (replicate, or a reflection about the wrong column) would turn
            # into a non-zero derivative there is a corner pixel that differs from both of its neighbours.
            assert not dv[0, 0].any() and not dv[0, -1].any() and not dv[-1, 0].any() and not dv[-1, -1].any()
            for c, (y, x, ny, nx) in enumerate(((0, 0, 1, 1), (0, -1, 1, -2), (-1, 0, -2, 1), (-1, -1, -2, -2))):
                corner_hit[c] |= img[y, x] != img[y, nx] and img[y, x] != img[ny, x]
    assert top == 16 * 255
    assert edge_hit.all() and corner_hit.all()
    # the ties image: a sum of 128 mod 256 at every level, and the restated sums are the oracle's pyrDown
    ties = [f.left for f in fr if f.name == "extremes/ties"][0]
    cur = ties
    for _ in range(len(PC.level_sizes(W, H)) - 1):
        s = PC.pyr_down_sums(cur)
        assert ((s & 255) == 128).any()
        nxt = oracle.pyr_down(cur)
        assert np.array_equal(nxt, (s + 128) >> 8)
        cur = nxt


def _clahe_inputs(oracle, W, H):
    """{frame name: the images CLAHE gets on the GPU}: the designed pair (trackImage), and at the sizes that have an event
    handle also what the detector renders of the frame's planes and its one event per camera"""
    out = {}
    for k, f in enumerate(PC.frames(oracle, W, H, clahe=True)):
        if f.name.startswith("clahe/"):
            out[f.name] = [f.left, f.right]
            if (W, H) in PC.FOUR_LEVEL:
                out[f.name] += PC.oracle_surfaces(oracle, W, H, f, k)[4]
    return out


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_clahe_frames_reach_every_behaviour_of_the_clip_step(oracle, W, H):
    fr = _clahe_inputs(oracle, W, H)
    want = PC.attainable_clahe_classes(W, H)
    for pick in (slice(0, 2), slice(2, 4)):  # designed, rendered
        imgs = [img for v in fr.values() for img in v[pick]]
        if not imgs:
            continue
        got = set().union(*(PC.clahe_tile_classes(img) for img in imgs))
        assert got >= want, want - got
        if (W, H) in PC.FOUR_LEVEL:
            assert want == set(PC.CLAHE_CLASSES)
            # residuals on both sides of each threshold of `tid % step == 0 && tid / step < residual`
            res = {r for img in imgs for c, r, _ in PC.clahe_tile_stats(img) if c}
            assert {1, 100, 128, 129, 200, 255} <= res
    _, _, tw, th, _ = PC.clahe_geometry(W, H)
    ct = fr["clahe/constant_tiles"][0]
    assert all(len(np.unique(ct[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw])) == 1
               for ty in range(PC.TILES) for tx in range(PC.TILES) if ty * th < H and tx * tw < W)
    # a constant image: smin == smax, scale 0, every byte 0
    eq = oracle.clahe(fr["clahe/constant"][0])
    assert eq.min() == eq.max()
    assert not PC.level0(oracle, "equalize", fr["clahe/constant"][0]).any()


@pytest.mark.parametrize("W,H", list(PC.FOUR_LEVEL))
def test_normalize_restated(oracle, W, H):
    """the numpy restatement of the normalisation (scale and shift in double, rounded to float) is the oracle's on every
    surface an `equalize` handle renders, and the shift's arithmetic is pinned: the left level 0 of clahe/shift changes
    when the shift is computed in float from the rounded scale instead (the frame is searched for that; no other frame
    tells the two apart, and neither can a right surface: see shift_frame)"""
    killed = 0
    for k, f in enumerate(PC.frames(oracle, W, H, clahe=True)):
        for cam, img in enumerate(PC.oracle_surfaces(oracle, W, H, f, k)[4]):
            eq = oracle.clahe(img)
            want = oracle.normalize_minmax(eq)
            assert np.array_equal(PC.normalize_restated(eq), want), f.name
            n = int((PC.normalize_shift_in_float(eq) != want).sum())
            assert n == 0 or (cam == 0 and f.name == "clahe/shift"), (f.name, cam, n)
            killed += n
    assert killed >= 16  # (more than a pixel or two)


@pytest.mark.parametrize("W,H", ALL_SIZES)
def test_the_ring_takes_a_second_reflection_exactly_where_a_side_is_at_most_24(W, H):
    for lw, lh in PC.level_sizes(W, H):
        for n in (lw, lh):
            total = PC.ring_source_index(n)
            once = PC.reflect101_once(np.arange(-PC.PAD, n + PC.PAD), n)
            assert ((total >= 0) & (total < n)).all()
            assert (not np.array_equal(total, once)) == (n <= 24), n
            if n <= 24:
                # the suspect: the outermost columns (rows) past 2 n - 2 get a NEGATIVE source, i.e. the kernel reads a
                # ring byte of the opposite side, which the same launch writes
                bad = np.nonzero(once != total)[0]
                assert len(bad) == 25 - n and bad[0] == PC.PAD + 2 * n - 1 and bad[-1] == n + 2 * PC.PAD - 1
                assert (once[bad] < 0).all() and (once[bad] >= -PC.PAD).all()
                assert np.array_equal(total[bad], -once[bad])  # ... whose right value is the wanted one
            else:
                assert (once >= 0).all()
