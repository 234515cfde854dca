"""Inputs of the address-stage and hot-pixel tests, shared by the CPU test of the restatement and the GPU test of the
kernels: the sensor, the ROI, the streams and the figures about them that were counted with numpy alone
(tests/test_addr_filter_ref.py asserts each of them before anything is compared)."""
import numpy as np

import ba_filter_cases as K

W, H = K.W, K.H
ROI = (5, 7, 30, 20)                 # inclusive corners (x0, y0, x1, y1)
FULL = (0, 0, W - 1, H - 1)
HOT = (20, 20)                       # K.hot_pixel_events' pixel
STRADDLE = [(31, 0), (32, 0), (21, 1), (22, 1), (41, 41)]   # pixel indices 31, 32, 63, 64 and 1763 (the partial last word)


def pix(xy, w=W):
    return xy[0] + xy[1] * w


def uniform4097():
    return K.uniform_events(4097, W, H, 8 * 4097, seed=4197)


def uniform_wide(n, seed):
    """uniform on 64 x 48, for the second shape"""
    return K.uniform_events(n, 64, 48, 8 * max(n, 1), seed=seed)


def with_outsiders(ev, w, h, every=97):
    """the stream with every `every`-th event moved out of the sensor (x = w or y = h, alternating)"""
    out = ev.copy()
    idx = np.arange(0, len(out), every)
    out["x"][idx[0::2]] = w
    out["y"][idx[1::2]] = h
    return out
