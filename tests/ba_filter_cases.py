"""Inputs of the background-activity filter tests (esvio_fe_filter_events): the hand-made cases with their answers
derived by hand from the text of include/esvio_fe.h — written out here, produced by no implementation — and the
generators of the random streams.  Shared by the CPU test of the restatement and the GPU test of the kernels."""
import numpy as np

from esvio_amd.events import EVENT_DTYPE

W = H = 42          # the hand-made cases' sensor (the smallest a handle accepts)
WINDOW = 1000       # ... and their window, ns


def records(rows):
    """[(x, y, sec, nsec), ...] -> EVENT_DTYPE records, polarity alternating (the filter ignores it)"""
    ev = np.zeros(len(rows), EVENT_DTYPE)
    for i, (x, y, sec, nsec) in enumerate(rows):
        ev[i]["x"], ev[i]["y"], ev[i]["sec"], ev[i]["nsec"], ev[i]["polarity"] = x, y, sec, nsec, i & 1
    return ev


# name -> (events, min_support, expected flags, expected n_rejected); every case starts from a fresh plane
HAND = {
    # the second event's only stamped neighbour is 999 ns older: 999 < 1000
    "adjacent_inside_window": ([(10, 10, 7, 5000), (11, 10, 7, 5999)], 1, [0, 1], 0),
    # ... exactly window_ns older: 1000 < 1000 is false
    "adjacent_at_window": ([(10, 10, 7, 5000), (11, 10, 7, 6000)], 1, [0, 0], 0),
    # the event's own pixel never counts
    "same_pixel_repeats": ([(5, 5, 0, 100), (5, 5, 0, 200), (5, 5, 0, 300)], 1, [0, 0, 0], 0),
    # the diagonal neighbour, earlier in the stream, is stamped 8.999 ms LATER: a negative difference counts
    "later_stamped_neighbour": ([(20, 20, 3, 9_000_000), (21, 21, 3, 1000)], 1, [0, 1], 0),
    # a stamp of 0 is a stamp (500 - 0 < 1000); a pixel nobody stamped is `none`, not 0: the third event (stamp 10,
    # far from both) has no support
    "stamp_zero_supports": ([(3, 3, 0, 0), (4, 3, 0, 500), (30, 30, 0, 10)], 1, [0, 1, 0], 0),
    # corner (0,0) has 3 neighbours in the sensor: (1,0) finds 0 stamped, (0,1) finds (1,0), (1,1) finds both,
    # (0,0) finds all three
    "corner_support_3": ([(1, 0, 0, 100), (0, 1, 0, 200), (1, 1, 0, 300), (0, 0, 0, 400)], 3, [0, 0, 0, 1], 0),
    "corner_support_4": ([(1, 0, 0, 100), (0, 1, 0, 200), (1, 1, 0, 300), (0, 0, 0, 400)], 4, [0, 0, 0, 0], 0),
    # x = 42 is outside: rejected, flag 0, and it stamps nothing — not pixel (0,11) either, where 42 + 10*42 would
    # land: (1,11), a neighbour of that pixel and of nothing stamped, finds no support.  (11,10) is supported by
    # (10,10) across the rejected event.
    "rejected_between_supporters": ([(10, 10, 0, 100), (42, 10, 0, 150), (11, 10, 0, 200), (1, 11, 0, 250)], 1,
                                    [0, 0, 1, 0], 1),
    # y = 42 likewise; nsec >= 10^9 is taken as it is: 1 s + 0 ns against 0 s + 1_000_000_500 ns is 500 ns older
    "nsec_beyond_a_second": ([(7, 42, 0, 0), (8, 8, 1, 0), (9, 9, 0, 1_000_000_500)], 1, [0, 0, 1], 1),
}


def hand_case(name):
    rows, min_support, flags, rejected = HAND[name]
    return records(rows), min_support, np.array(flags, np.uint8), rejected


def uniform_events(n, w, h, span_us, seed, t0_us=1_000_000_000, patch=None):
    """n events uniform on the w x h sensor (or on its patch x patch corner), stamps uniform over span_us, ascending"""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, EVENT_DTYPE)
    ev["x"] = rng.integers(0, patch or w, n)
    ev["y"] = rng.integers(0, patch or h, n)
    t = np.sort(rng.integers(0, max(span_us, 1), n)) + t0_us
    ev["sec"], ev["nsec"] = t // 1_000_000, (t % 1_000_000) * 1000
    ev["polarity"] = rng.integers(0, 2, n)
    return ev


SWEEP_SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4097)   # the wave's and the sort tile's boundaries


def sweep_events(n):
    """the size sweep: uniform on 42 x 42 (on a 12 x 12 corner patch below 2047 events), stamps uniform over 8 n us"""
    return uniform_events(n, W, H, 8 * n, seed=100 + n, patch=12 if n < 2047 else None)


def hot_pixel_events(n_hot=5000, seed=5):
    """one pixel with n_hot events, interleaved one to one with events of its 8 neighbours (half of them) and of far
    pixels: the hot pixel's segment of the sorted batch is n_hot long.  Stamps step by 0..3 us."""
    rng = np.random.default_rng(seed)
    n = 2 * n_hot
    ev = np.zeros(n, EVENT_DTYPE)
    ev["x"], ev["y"] = 20, 20
    near = rng.random(n_hot) < 0.5
    d = rng.integers(0, 8, n_hot)
    d = d + (d >= 4)  # 0..8 without the centre
    ev["x"][1::2] = np.where(near, 20 + d % 3 - 1, rng.integers(0, 14, n_hot))
    ev["y"][1::2] = np.where(near, 20 + d // 3 - 1, rng.integers(0, 14, n_hot))
    t = np.cumsum(rng.integers(0, 4, n)) + 2_000_000_000
    ev["sec"], ev["nsec"] = t // 1_000_000, (t % 1_000_000) * 1000
    return ev
