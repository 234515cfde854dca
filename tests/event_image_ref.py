"""The event images of include/esvio_fe.h ("event images") as the plain loop: detector.cur_event_mat_left/right
(event_detector.cc:145-146, :164-165, :208-209, :226-227) for the events of one call, in stream order."""
import numpy as np

ON, OFF = (255, 0, 0), (0, 0, 255)  # (B, G, R)


def event_image(ev, W, H, base=None, pixels=None):
    """(H, W, 3) uint8 after the events `ev` (EVENT_DTYPE) are applied in stream order to `base` (None: zeros — a track
    call; a stage call passes the image as it is).  pixels: None, or per event the (x, y) the SAE update writes it at,
    (-1, -1) for an event it drops (the motion-compensated overload: the warped pixels)."""
    E = np.zeros((H, W, 3), np.uint8) if base is None else np.array(base, np.uint8, copy=True)
    assert E.shape == (H, W, 3)
    for i in range(len(ev)):
        x, y = (int(ev["x"][i]), int(ev["y"][i])) if pixels is None else (int(pixels[i][0]), int(pixels[i][1]))
        if pixels is None and (x >= W or y >= H):
            continue  # the SAE update skips it
        if x < 0 or y < 0:
            continue  # dropped
        assert x < W and y < H
        E[y, x] = ON if ev["polarity"][i] != 0 else OFF
    return E


def canvas(L, R):
    """hconcat(left, right) (feature_tracker.cpp:1107): (H, 2 W, 3)"""
    assert L.shape == R.shape
    return np.concatenate([L, R], axis=1)
