"""The ordered per-block emission (block_list_slot in fe_kernels.hip: ballot, per-wave counts, one barrier, prefix over
the earlier waves) at its edges, seen through the one public entry point that returns the compacted list itself:
esvio_fe_fast_corners without non-max hands back k_fast_collect's lists in raster order, with scores; with non-max
the second count (n_detected, the takers before non-max) goes through the same barrier.  Device against the numpy
restatement tests/fast_ref.py (tied to the reference's compiled FAST by tests/test_fast_ref.py), bit for bit:
positions, order, scores, n_out, n_detected, for arc 9 and 10, non-max off and on, image in host and device memory.

The images are built so that, over 256-pixel blocks and 64-pixel waves in raster order, they contain together
  (a) a block with no taker;                       (d) takers in lane 0 and in lane 63 of some wave;
  (b) a block whose only takers sit in its last wave;  (e) a wave with at least 32 takers;
  (c) a block with takers in every wave;           (f) takers in the short last block.
test_images_contain_every_class (no GPU) asserts that from the restatement's output alone.

Sizes: the smallest handle is 42 x 42, so 64 x 44 stands for "whole blocks only" (11 of them; a wave is one row: (e),
and lane 0 is always border: no (d)); 70 x 47 has a short last block of 218 pixels that reaches row H - 4, the last
row FAST looks at ((f); a short block of fewer than 3 W + 4 pixels lies in the border rows and can hold no taker:
70 x 45, kept as the case whose last block is empty).

How the takers are placed: a single bright pixel on a dark ground is a FAST-9 and FAST-10 corner at barrier 20 (all 16
ring pixels darker) and makes no other pixel one.  (e) needs more than the one-in-two such pixels allow in a row whose
first and last three pixels are border: a sawtooth 40, 110, 180, 250 along x in one row — a pixel whose right ring
pixel (x + 3) is darker by more than the barrier keeps a darker arc of 15, so three of four are corners."""
import functools

import numpy as np
import pytest

import fast_ref
from esvio_amd import frontend as FE
from test_fast_gpu import DeviceImage, _check_against, _handle, _ref

BLOCK, WAVE, BARRIER = 256, 64, 20
SIZES = [(64, 44), (70, 45), (70, 47)]
CLASSES = "abcdef"


def _valid(i, W, H):
    return 3 <= i % W < W - 3 and 3 <= i // W < H - 3


def build_image(W, H):
    img = np.zeros((H, W), np.uint8)
    flat = img.reshape(-1)
    P = W * H
    img[5, 3:W - 3] = 40 + 70 * (np.arange(3, W - 3) % 4)  # (e); rows 2..8 see it on their rings
    block = -(-12 * W // BLOCK)  # the first block that starts below row 11
    # (b) one pixel in the block's last wave
    flat[[i for i in range(block * BLOCK + 3 * WAVE, (block + 1) * BLOCK) if _valid(i, W, H)][-1]] = 255
    block += 1
    # (c) one pixel in every wave of the next block (more than three pixels apart in x from each other and from (b)'s:
    # neighbours of equal score fall to the non-max, and two bright pixels on opposite sides of a ring undo a corner)
    for w in range(BLOCK // WAVE):
        flat[[i for i in range(block * BLOCK + w * WAVE, block * BLOCK + (w + 1) * WAVE) if _valid(i, W, H)][13 * w + 5]] = 255
    block += 1
    # (d) the first later wave whose lanes 0 and 63 are both inside the border, if the width has one
    for w in range(block * BLOCK // WAVE, P // WAVE):
        if _valid(w * WAVE, W, H) and _valid(w * WAVE + WAVE - 1, W, H):
            flat[w * WAVE] = flat[w * WAVE + WAVE - 1] = 255
            break
    # (f) the first pixel of the short last block that FAST looks at, if there is one
    if P % BLOCK:
        for i in range(P // BLOCK * BLOCK, P):
            if _valid(i, W, H):
                flat[i] = 255
                break
    return img


@functools.lru_cache(maxsize=None)
def case(W, H):
    """the image and the restatement's (detect_9, detect_10, score_10, non-max survivors): computed once, read-only"""
    img = build_image(W, H)
    ref = _ref(img, BARRIER)
    img.setflags(write=False)
    for a in ref:
        a.setflags(write=False)
    return img, ref


def classes_of(xy, W, H):
    """which of (a)..(f) a list of takers (x, y) shows"""
    P = W * H
    idx = xy[:, 1].astype(np.int64) * W + xy[:, 0].astype(np.int64)
    n_blocks, n_waves = -(-P // BLOCK), -(-P // WAVE)
    per_wave = np.bincount(idx // WAVE, minlength=n_waves)
    per_wave_of_block = np.zeros(n_blocks * (BLOCK // WAVE), np.int64)
    per_wave_of_block[:n_waves] = per_wave
    per_wave_of_block = per_wave_of_block.reshape(n_blocks, BLOCK // WAVE)
    per_block = per_wave_of_block.sum(1)
    lanes = np.zeros((n_waves, WAVE), bool)
    lanes[idx // WAVE, idx % WAVE] = True
    got = set()
    if (per_block == 0).any():
        got.add("a")
    if ((per_wave_of_block[:, :-1].sum(1) == 0) & (per_wave_of_block[:, -1] > 0)).any():
        got.add("b")
    if (per_wave_of_block > 0).all(1).any():
        got.add("c")
    if (lanes[:, 0] & lanes[:, -1]).any():
        got.add("d")
    if (per_wave >= 32).any():
        got.add("e")
    if P % BLOCK and per_block[-1] > 0:
        got.add("f")
    return got


def test_images_contain_every_class():
    """from the restatement's output alone, for the lists each mode of the GPU test compares: detect_9, detect_10 and
    the non-max survivors each show (a)..(f) over the images together; (e) on the image of whole rows per wave, (f) on
    the one whose short last block reaches below the border; the count before non-max differs from the one after"""
    seen = {"detect_9": {}, "detect_10": {}, "nonmax": {}}
    for W, H in SIZES:
        img, (d9, d10, s10, nm) = case(W, H)
        seen["detect_9"][W, H] = classes_of(d9, W, H)
        seen["detect_10"][W, H] = classes_of(d10, W, H)
        seen["nonmax"][W, H] = classes_of(d10[nm], W, H)
        assert 0 < len(nm) < len(d10), (W, H, len(nm), len(d10))
    for mode, by_size in seen.items():
        # (survivors of the 3 x 3 non-max are never neighbours: at most 29 of a row's 58 inner pixels, and with 42 <= W
        # a wave covers at most two rows, which are adjacent — 32 survivors in a wave cannot be; the second count that
        # mode carries through the barrier is detect_10's, which has them)
        assert set().union(*by_size.values()) == set(CLASSES) - ({"e"} if mode == "nonmax" else set()), (mode, by_size)
    for mode in ("detect_9", "detect_10"):
        assert "e" in seen[mode][64, 44] and "f" in seen[mode][70, 47], (mode, seen[mode])
        assert "f" not in seen[mode][70, 45] and "d" in seen[mode][70, 47], (mode, seen[mode])
        assert {"a", "b", "c"} <= seen[mode][64, 44] & seen[mode][70, 47], (mode, seen[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_lists_equal_restatement_at_the_emitters_edges(W, H):
    img, (d9, d10, s10, nm) = case(W, H)
    print((W, H), "n9", len(d9), "n10", len(d10), "nonmax", len(nm), "classes", "".join(sorted(classes_of(d10, W, H))))
    ft = _handle(W, H)
    dev = DeviceImage(img)
    for space, arg in (("host", np.array(img)), ("device", dev.ptr.value)):
        _check_against(ft, img, arg, BARRIER, d9, d10, s10, nm, (W, H, space))
    dev.free()
    ft.close()
