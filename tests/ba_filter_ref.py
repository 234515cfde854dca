"""The background-activity filter of include/esvio_fe.h (esvio_fe_filter_events) as the plain sequential loop its text
describes: an int64 plane per camera, -1 = none, Python integers for the stamps.  Independent of the kernels — no sort,
no segments: one event after the other."""
import numpy as np

NONE = -1
NEIGHBOURS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


def fresh_plane(W, H):
    return np.full(W * H, NONE, np.int64)


def filter_events(B, W, H, ev, window_ns, min_support=1):
    """advances the plane B (in place) by the events `ev` (EVENT_DTYPE records) -> (flags uint8[n], n_rejected)"""
    assert 1 <= window_ns <= 1 << 62 and 1 <= min_support <= 8
    n = len(ev)
    flags = np.zeros(n, np.uint8)
    rejected = 0
    xs, ys = ev["x"].tolist(), ev["y"].tolist()
    secs, nsecs = ev["sec"].tolist(), ev["nsec"].tolist()
    for i in range(n):
        x, y = xs[i], ys[i]
        if x >= W or y >= H:                       # 1.
            rejected += 1
            continue
        t = secs[i] * 10 ** 9 + nsecs[i]           # 2.
        support = 0
        for dx, dy in NEIGHBOURS:                  # 3.
            u, v = x + dx, y + dy
            if not (0 <= u < W and 0 <= v < H):
                continue
            b = int(B[u + v * W])
            if b != NONE and t - b < window_ns:
                support += 1
        flags[i] = support >= min_support          # 4.
        B[x + y * W] = t                           # 5.
    return flags, rejected


def raw_records(ev):
    """the records as rows of 16 bytes, padding included (numpy's own copies of a structured array drop it)"""
    return np.ascontiguousarray(ev).view(np.uint8).reshape(-1, 16)


def kept_of(ev, flags):
    """the records the call emits — all 16 bytes of each, as rows of bytes — and the last of them (None if none)"""
    kept = raw_records(ev)[flags != 0]
    return kept, (kept[-1] if len(kept) else None)
