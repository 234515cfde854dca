"""The filter rule of include/esvio_fe.h with esvio_fe_filter_params (esvio_fe_filter_batch, esvio_fe_track_batch) as
the plain sequential loop its text describes: steps 1-5 with step 3b (the refractory test on the pixel's own previous
stamp) and step 4's second form (min_support 0: no support test).  An int64 plane per camera, -1 = none, Python
integers for the stamps.  Independent of the kernels — no sort, no segments — and of tests/ba_filter_ref.py, which
restates esvio_fe_filter_events alone: the two loops are compared with each other in tests/test_ba_filter2_ref.py."""
import numpy as np

NONE = -1
LIMIT = 1 << 62
NEIGHBOURS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


def fresh_plane(W, H):
    return np.full(W * H, NONE, np.int64)


def filter_events(B, W, H, ev, window_ns, min_support=1, refractory_ns=0, want_parts=False):
    """advances the plane B (in place) by the events `ev` (EVENT_DTYPE records) -> (flags uint8[n], n_rejected);
    want_parts: -> (flags, n_rejected, supported uint8[n], refractory uint8[n]), the two tests' own verdicts"""
    assert 0 <= min_support <= 8 and 0 <= refractory_ns <= LIMIT
    assert min_support == 0 or 1 <= window_ns <= LIMIT
    n = len(ev)
    flags, sup, refr = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    rejected = 0
    xs, ys = ev["x"].tolist(), ev["y"].tolist()
    secs, nsecs = ev["sec"].tolist(), ev["nsec"].tolist()
    for i in range(n):
        x, y = xs[i], ys[i]
        if x >= W or y >= H:                                   # 1.
            rejected += 1
            continue
        t = secs[i] * 10 ** 9 + nsecs[i]                       # 2.
        supported = True
        if min_support > 0:                                    # 3.
            support = 0
            for dx, dy in NEIGHBOURS:
                u, v = x + dx, y + dy
                if 0 <= u < W and 0 <= v < H:
                    b = int(B[u + v * W])
                    if b != NONE and t - b < window_ns:
                        support += 1
            supported = support >= min_support
        own = int(B[x + y * W])                                # 3b.
        refractory = refractory_ns > 0 and own != NONE and t - own < refractory_ns
        flags[i] = supported and not refractory                # 4.
        sup[i], refr[i] = supported, refractory
        B[x + y * W] = t                                       # 5.
    return (flags, rejected, sup, refr) if want_parts else (flags, rejected)
