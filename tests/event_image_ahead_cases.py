"""Designed sequences for the event images that follow announced batches (include/esvio_fe.h "event images", mode 2):
stereo batches whose images tell the frames apart.  The sensor of tests/event_image_cases.py is cut into five bands of
nine rows; batch k's left events lie in band k % 5 and its right events in band (k + 2) % 5, so any two batches within
four of each other touch different rows in both cameras: an image delivered a frame (or up to four) early or late
cannot equal the one that was due.  tests/test_event_image_ahead_ref.py checks that."""
import numpy as np

import event_image_cases as K
import event_image_ref as R
from esvio_amd.events import EVENT_DTYPE

W, H = K.W, K.H
N_BATCHES = 9
BANDS, BAND_ROWS = 5, 9
STEP_US = 20_000
NO_RIGHT = 5                                  # the batch with nR = 0
PUB = (1, 0, 1, 1, 0, 0, 1, 0, 1)             # published frames mixed with unpublished ones, singly and in pairs
NONE = np.zeros(0, EVENT_DTYPE)


def band(k):
    return (0, (k % BANDS) * BAND_ROWS, W, (k % BANDS) * BAND_ROWS + BAND_ROWS)


def sequence(seed=0, n=N_BATCHES, first=0):
    """[(left, right, cur_time)]: batch k has 300 .. 4300 left and 300 .. 2300 right events — below and above one event
    per pixel of the cameras that have events, the density at which k_evimg_mark changes its form — with stamps inside
    its own 20 ms"""
    out = []
    for k in range(first, first + n):
        t0 = K.T0_US + k * STEP_US
        nl, nr = 300 + 1000 * (k % 5), 2300 - 500 * (k % 5)
        L = K.uniform(nl, 1000 + 17 * seed + k, t0_us=t0, region=band(k))
        Rt = NONE if k - first == NO_RIGHT else K.uniform(nr, 2000 + 17 * seed + k, t0_us=t0, region=band(k + 2))
        out.append((L, Rt, (t0 + STEP_US - 1) * 1e-6))
    return out


_ref = {}


def reference(seed=0):
    """[(left image, right image, canvas)] of sequence(seed) by the plain loop, computed once per process"""
    if seed not in _ref:
        imgs = []
        for L, Rt, _ in sequence(seed):
            a, b = R.event_image(L, W, H), R.event_image(Rt, W, H)
            for x in (a, b):
                x.setflags(write=False)
            imgs.append((a, b, R.canvas(a, b)))
        _ref[seed] = imgs
    return _ref[seed]
