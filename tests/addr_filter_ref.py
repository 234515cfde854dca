"""The address stage (step 1a of the filter rule) and hot-pixel learning of include/esvio_fe.h as the plain sequential
loops their text describes.  filter_events is tests/ba_filter2_ref.py's loop with step 1a between its steps 1 and 2;
Hot.learn / Hot.select count and select with Python integers.  Independent of the kernels: no sort, no segments, no
waves."""
import numpy as np

NONE = -1
LIMIT = 1 << 62
NEIGHBOURS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


class Stage:
    """an esvio_fe_address_filter and the camera's pixel mask (a set of pixel indices y*W + x, or None: no mask set)"""

    def __init__(self, roi, polarity=0, flatten=0, use_mask=0, mask=None):
        self.roi, self.polarity, self.flatten, self.use_mask = tuple(roi), polarity, flatten, use_mask
        self.mask = None if mask is None else set(mask)

    def rejects(self, x, y, pol, W):
        x0, y0, x1, y1 = self.roi
        if x < x0 or x > x1 or y < y0 or y > y1:
            return True
        if self.use_mask and self.mask is not None and (x + y * W) in self.mask:
            return True
        on = pol != 0
        return (self.polarity == 1 and not on) or (self.polarity == 2 and on)


def fresh_plane(W, H):
    return np.full(W * H, NONE, np.int64)


def filter_events(B, W, H, ev, window_ns, min_support=1, refractory_ns=0, stage=None):
    """advances the plane B (in place) by the events `ev` (EVENT_DTYPE records) ->
    (flags uint8[n], n_rejected, n rejected by the stage alone)"""
    assert 0 <= min_support <= 8 and 0 <= refractory_ns <= LIMIT
    assert min_support == 0 or 1 <= window_ns <= LIMIT
    n = len(ev)
    flags = np.zeros(n, np.uint8)
    rejected = by_stage = 0
    xs, ys, ps = ev["x"].tolist(), ev["y"].tolist(), ev["polarity"].tolist()
    secs, nsecs = ev["sec"].tolist(), ev["nsec"].tolist()
    for i in range(n):
        x, y = xs[i], ys[i]
        if x >= W or y >= H:                                   # 1.
            rejected += 1
            continue
        if stage is not None and stage.rejects(x, y, ps[i], W):  # 1a.
            rejected += 1
            by_stage += 1
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
        B[x + y * W] = t                                       # 5.
    return flags, rejected, by_stage


def raw_records(ev):
    return np.ascontiguousarray(ev).view(np.uint8).reshape(-1, 16)


def kept_of(ev, flags, stage=None):
    """the records the call emits, all 16 bytes of each as rows (byte 12 flattened), and the last of them (or None)"""
    kept = raw_records(ev)[flags != 0].copy()
    if stage is not None and stage.flatten:
        kept[:, 12] = 1 if stage.flatten == 1 else 0
    return kept, (kept[-1] if len(kept) else None)


def without_stage(ev, stage, W, H):
    """S -> S': the stream without its address-rejected events (out-of-sensor ones stay) and with polarity rewritten"""
    xs, ys, ps = ev["x"].tolist(), ev["y"].tolist(), ev["polarity"].tolist()
    keep = [not (xs[i] < W and ys[i] < H and stage.rejects(xs[i], ys[i], ps[i], W)) for i in range(len(ev))]
    out = raw_records(ev)[np.array(keep, bool)].copy().view(ev.dtype).reshape(-1)  # (whole records: the padding travels)
    if stage.flatten:
        inside = (out["x"] < W) & (out["y"] < H)
        out["polarity"][inside] = 1 if stage.flatten == 1 else 0
    return out


class Hot:
    """one camera's learning state"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.reset()

    def reset(self):
        self.C = [0] * (self.W * self.H)
        self.N, self.t_min, self.t_max = 0, None, None

    def learn(self, ev, bad=None):
        """every in-sensor event counts; bad: indices of events that conversion calls BAD (not counted)"""
        bad = set(bad or ())
        xs, ys = ev["x"].tolist(), ev["y"].tolist()
        secs, nsecs = ev["sec"].tolist(), ev["nsec"].tolist()
        for i in range(len(ev)):
            if i in bad or xs[i] >= self.W or ys[i] >= self.H:
                continue
            t = secs[i] * 10 ** 9 + nsecs[i]
            self.C[xs[i] + ys[i] * self.W] += 1
            self.N += 1
            self.t_min = t if self.t_min is None else min(self.t_min, t)
            self.t_max = t if self.t_max is None else max(self.t_max, t)

    def select(self, max_pixels, min_count=1, min_rate_hz=0, mean_factor=0):
        """-> ([(x, y)], [count], dict(events, span_ns, threshold, above, selected))"""
        P = self.W * self.H
        span = self.t_max - self.t_min if self.N else 0
        T = min_count
        if min_rate_hz:
            T = max(T, -((-min_rate_hz * span) // 10 ** 9))
        if mean_factor:
            T = max(T, -((-mean_factor * self.N) // P))
        hot = [p for p in range(P) if self.C[p] >= T]
        hot.sort(key=lambda p: (-self.C[p], p))
        sel = hot[:max_pixels]
        info = dict(events=self.N, span_ns=span, threshold=T, above=len(hot), selected=len(sel))
        return [(p % self.W, p // self.W) for p in sel], [self.C[p] for p in sel], info
