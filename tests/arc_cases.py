"""Planted SAE planes that take Arc* (EventDetector::isCorner, event_detector.cc:308-544) to its edges, and the one
independent transcription of its ring loop that the oracle is checked against.  Corner centres are tiled over the plane
on a 9-pixel grid, so the 16 small-ring and 20 large-ring pixels of a centre are its own and a ring can be given any
values: ties, arcs at the 4 / 6 / 10 / 12 and 5 / 8 / 12 / 15 length limits, stamps one ulp apart.  One family of rings
is planted on the polarity-1 plane and another on the polarity-0 plane of the same pages, with an event of either
polarity on every centre.  Seeded numpy, no device code; shared by test_arc_cases.py, which shows without a GPU that the
cases reach the edges they are for, and test_arc_edges_gpu.py, which holds the device's rank form (k_arc_mark,
k_arc_map, k_arc_ev, k_dedup) to the oracle."""
import collections
import operator

import numpy as np

from esvio_amd.events import EVENT_DTYPE, event_times

SMALL = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
         (-3, 0), (-3, 1), (-2, 2), (-1, 3))
LARGE = ((0, 4), (1, 4), (2, 3), (3, 2), (4, 1), (4, 0), (4, -1), (3, -2), (2, -3), (1, -4), (0, -4), (-1, -4),
         (-2, -3), (-3, -2), (-4, -1), (-4, 0), (-4, 1), (-3, 2), (-2, 3), (-1, 4))
LIMITS = {16: (4, 6), 20: (5, 8)}  # kSmallMinThresh / kSmallMaxThresh, kLargeMinThresh / kLargeMaxThresh

GRID = 9           # centre spacing: the large ring reaches 4 pixels out
SIZES = ((346, 260), (173, 131), (256, 64))
MIN_DIST = 3       # the smallest the handle accepts: border limit 4, every grid centre is inside it
NEW, OLD = 5.0, 1.0
EPOCH = 1.7e9      # stamps of a recording that carries wall-clock time


# ------------------------------------------------------------------ the independent transcription
def ring_segment_size(v, kmin, join=operator.ge):
    """the newest segment's size of one ring (event_detector.cc:337-428 / :438-534); `join`: the test that lets a
    frontier pixel into the segment (the reference's is >=)"""
    N = len(v)
    seg = v[0]
    ri = 0
    for i in range(1, N):
        if v[i] > seg:
            seg, ri = v[i], i
    li = (ri - 1 + N) % N
    ri = (ri + 1) % N
    lv, rv = v[li], v[ri]
    lmin, rmin = lv, rv
    size = kmin
    for it in range(1, N):
        if rv > lv:
            if it < kmin:
                seg = min(seg, rmin)
            elif join(rv, seg):
                size = it + 1
                seg = min(seg, rmin)
            ri = (ri + 1) % N
            rv = v[ri]
            rmin = min(rmin, rv)
        else:
            if it < kmin:
                seg = min(seg, lmin)
            elif join(lv, seg):
                size = it + 1
                seg = min(seg, lmin)
            li = (li - 1 + N) % N
            lv = v[li]
            lmin = min(lmin, lv)
    return size


def ring_accepts(size, N, kmin, kmax):
    """:430-435 / :536-541"""
    return size <= kmax or (N - kmax <= size <= N - kmin)


def ring_python(v, join=operator.ge, accepts=ring_accepts):
    """one ring's verdict from its 16 or 20 values in circle order"""
    N = len(v)
    kmin, kmax = LIMITS[N]
    return bool(accepts(ring_segment_size([float(a) for a in v], kmin, join), N, kmin, kmax))


def arc_python(S, x, y):
    """independent transcription of the reference's two ring loops on the plane S, used only to cross-check the oracle"""
    return (ring_python([S[y + dy, x + dx] for dx, dy in SMALL]) and
            ring_python([S[y + dy, x + dx] for dx, dy in LARGE]))


def is_corner_python(L0, L1, S0, S1, ev, thr=0.01, min_dist=MIN_DIST):
    """isCorner for every record of `ev`, transcribed: the pre-check (:315), the border limit (:320-324), the two rings;
    0 for a record outside the sensor (the reference is never handed one)"""
    L, S = (L0, L1), (S0, S1)
    H, W = S0.shape
    b = min_dist + 1
    out = np.zeros(len(ev), np.uint8)
    for i, (x, y, et, p) in enumerate(zip(ev["x"].tolist(), ev["y"].tolist(), event_times(ev).tolist(),
                                          (ev["polarity"] != 0).astype(int).tolist())):
        if x >= W or y >= H:
            continue
        if et > L[p][y, x] + thr or L[1 - p][y, x] > L[p][y, x]:
            continue
        if x < b or x >= W - b or y < b or y >= H - b:
            continue
        out[i] = arc_python(S[p], x, y)
    return out


# ------------------------------------------------------------------ rings
def arc_ring(N, length, start, inside=NEW, outside=OLD):
    """`length` consecutive pixels from `start` hold `inside` (a value or `length` values), the rest `outside`"""
    v = np.empty(N, np.float64)
    v[(start + np.arange(length)) % N] = inside
    v[(start + length + np.arange(N - length)) % N] = outside
    return v


PASSING = {16: arc_ring(16, 5, 2), 20: arc_ring(20, 6, 3)}  # 5 of 16 / 6 of 20 new pixels: the other ring's fixed pattern


def twolevel(N):
    """every arc length 1..N-1 at every rotation: N (N - 1) rings; every rank field is the arc's start once"""
    return [arc_ring(N, a, r) for a in range(1, N) for r in range(N)]


def _two_groups(N, n, seed, inside, outside):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a, r = int(rng.integers(1, N)), int(rng.integers(0, N))
        out.append(arc_ring(N, a, r, rng.choice(inside, a), rng.choice(outside, N - a)))
    return out


def noisy(N, n=320, seed=101):
    """a random arc; stamps inside from three values above the three used outside: ties inside both groups"""
    return _two_groups(N, n, seed + N, (4.0, 4.5, 5.0), (1.0, 1.5, 2.0))


def overlap(N, n=480, seed=202):
    """as noisy, but the lowest inside value equals the highest outside one: the >= of the join test decides"""
    return _two_groups(N, n, seed + N, (2.0, 4.5, 5.0), (1.0, 1.5, 2.0))


def ramps(N, n=320, seed=303):
    """a tent around a random peak, clipped by a plateau on top and a floor below and quantised in steps of 1 to 3 ring
    positions: symmetric ties between the left and the right frontier, several equal maxima (every 16th ring has its
    plateau across indices N-1 and 0)"""
    rng = np.random.default_rng(seed + N)
    out = []
    for k in range(n):
        peak = int(rng.integers(0, N))
        half, floor, q = int(rng.integers(0, 3)), int(rng.integers(1, N // 2 + 1)), int(rng.integers(1, 4))
        if k % 16 == 0:
            peak, half = (0, 1) if k % 32 else (N - 1, 1)  # maxima at N-1, 0 (and 1 / N-2)
        i = np.arange(N)
        d = np.minimum((i - peak) % N, (peak - i) % N)
        out.append(10.0 - np.minimum(np.maximum(d - half, 0), floor) // q)
    return out


def perm(N, n=96, seed=404):
    rng = np.random.default_rng(seed + N)
    return [rng.permutation(N).astype(np.float64) + 1.0 for _ in range(n)]


def ternary(N, n=96, seed=505):
    rng = np.random.default_rng(seed + N)
    return [rng.choice((1.0, 2.0, 3.0), N) for _ in range(n)]


def one_ulp_apart(rings, base=EPOCH):
    """the rings with their distinct values replaced, in order, by consecutive doubles from `base` up"""
    levels = sorted({float(a) for v in rings for a in v})
    chain = [base]
    for _ in levels[1:]:
        chain.append(float(np.nextafter(chain[-1], np.inf)))
    m = dict(zip(levels, chain))
    return [np.array([m[float(a)] for a in v]) for v in rings]


def epoch(N):
    """twolevel and noisy again at 1.7e9 s with the levels one ulp apart: ranks must separate neighbouring doubles"""
    return one_ulp_apart(twolevel(N)) + one_ulp_apart(noisy(N, seed=606))


FAMILIES = dict(twolevel=twolevel, noisy=noisy, overlap=overlap, ramps=ramps, perm=perm, ternary=ternary, epoch=epoch)
COUNTED = ("twolevel", "noisy", "overlap", "ramps")  # the families the shares and the sensitivity counts are taken over
_RINGS = {}


def family(name, N):
    if (name, N) not in _RINGS:
        _RINGS[(name, N)] = FAMILIES[name](N)
    return _RINGS[(name, N)]


def family_time_us(name):
    """the stamp of a family's events: after every stamp of its rings"""
    return 1_700_000_100_000_000 if name == "epoch" else 5_000_000


# ------------------------------------------------------------------ planes and events
def centres(W, H):
    """[(x, y)] of the grid, row by row: 1064 at 346 x 260"""
    return [(x, y) for y in range(4, H - 4, GRID) for x in range(4, W - 4, GRID)]


def records(x, y, t_us, pol):
    """event records; x and y may be anything a uint16 holds (make_events would do, this one takes per-event stamps
    as well)"""
    x = np.atleast_1d(np.asarray(x))
    ev = np.zeros(x.shape[0], EVENT_DTYPE)
    t_us = np.broadcast_to(np.asarray(t_us, np.int64), x.shape)
    ev["x"], ev["y"] = x, np.broadcast_to(np.asarray(y), x.shape)
    ev["sec"] = (t_us // 1_000_000).astype(np.uint32)
    ev["nsec"] = ((t_us % 1_000_000) * 1000).astype(np.uint32)
    ev["polarity"] = np.broadcast_to(np.asarray(pol), x.shape).astype(np.uint8)
    return ev


def join(parts):
    """the records of `parts` in one array (np.concatenate would pack the 16-byte records to 13)"""
    ev = np.zeros(sum(len(p) for p in parts), EVENT_DTYPE)
    k = 0
    for p in parts:
        ev[k:k + len(p)] = p
        k += len(p)
    return ev


def plant(S, x, y, small, large):
    """the two rings of centre (x, y) into the plane S; pixels outside the plane are left out"""
    H, W = S.shape
    for circle, v in ((SMALL, small), (LARGE, large)):
        for (dx, dy), a in zip(circle, v):
            if 0 <= x + dx < W and 0 <= y + dy < H:
                S[y + dy, x + dx] = a


Page = collections.namedtuple("Page", "L0 L1 S0 S1 events rings")
# rings: per event (centre index, x, y, polarity, small ring, large ring), for the message of a failure


def pages(W, H, pairs1, pairs0, t_us):
    """pairs1 / pairs0: (small ring, large ring) value vectors for the polarity-1 / polarity-0 plane, one pair per centre,
    as many pages as the longer list takes.  Every centre that holds a pair gets one event of that polarity at t_us and
    L0 = L1 = the event's time, so the pre-check passes for both polarities."""
    cs = centres(W, H)
    t = float(event_times(records([0], [0], t_us, 1))[0])
    out = []
    for k in range(0, max(len(pairs1), len(pairs0)), len(cs)):
        S = [np.zeros((H, W)), np.zeros((H, W))]
        L = np.zeros((H, W))
        xs, ys, ps, rings = [], [], [], []
        for i, (x, y) in enumerate(cs):
            for pol, pairs in ((1, pairs1), (0, pairs0)):
                if k + i < len(pairs):
                    small, large = pairs[k + i]
                    plant(S[pol], x, y, small, large)
                    L[y, x] = t
                    xs.append(x), ys.append(y), ps.append(pol)
                    rings.append((k + i, x, y, pol, small, large))
        out.append(Page(L, L.copy(), S[0], S[1], records(xs, ys, t_us, ps), rings))
    return out


def family_pages(name, W, H):
    """the family's N = 16 rings on the polarity-1 plane (with the fixed passing large ring), its N = 20 rings on the
    polarity-0 plane (with the fixed passing small ring)"""
    return pages(W, H, [(v, PASSING[20]) for v in family(name, 16)], [(PASSING[16], v) for v in family(name, 20)],
                 family_time_us(name))


def family_sizes(name):
    return SIZES if name == "twolevel" else SIZES[:1]


def describe(page, i, got, want):
    k, x, y, pol, small, large = page.rings[i]
    return "ring %d at (%d, %d) polarity %d: got %d, want %d\n  small %s\n  large %s" % (
        k, x, y, pol, got, want, np.asarray(small).tolist(), np.asarray(large).tolist())


# ------------------------------------------------------------------ the pre-check (:315)
PRE_W, PRE_H = 346, 260
THRESHOLDS = (0.01, 0.003)                       # the default feature_filter_threshold and another
PRE_TIMES_US = (5_000_123, 1_700_000_000_123_456)  # near 5 s and near 1.7e9 s


def level_for_sum(target, thr):
    """an L with fl(L + thr) == target.  L < target, so the doubles around L are spaced no wider than those around the
    sum: stepping L by one ulp moves the rounded sum by at most one ulp and the search cannot step over the target."""
    L = target - thr
    for _ in range(64):
        s = L + thr
        if s == target:
            return float(L)
        L = np.nextafter(L, np.inf if s < target else -np.inf)
    raise AssertionError("no L with L + %r == %r" % (thr, target))


PreCase = collections.namedtuple("PreCase", "name x y pol L_own L_other")


def precheck_cases(thr):
    """[(name, cases)]: triples below / equal / above of one term of the pre-check, every case on a centre of its own
    with passing rings on both planes.
    polarity term: L[!p] one ulp below, equal to and one ulp above L[p] (= the event's time);
    refractory term: L[p] such that the event's time is one ulp below L[p] + thr, equal to it and one ulp above it."""
    cs = centres(PRE_W, PRE_H)
    out, k = [], 0
    for t_us in PRE_TIMES_US:
        et = float(event_times(records([0], [0], t_us, 1))[0])
        for pol in (1, 0):
            tri = []
            for rel, other in (("below", np.nextafter(et, -np.inf)), ("equal", et), ("above", np.nextafter(et, np.inf))):
                tri.append(PreCase("polarity/%s" % rel, cs[k][0], cs[k][1], pol, et, float(other)))
                k += 1
            out.append(("polarity p=%d t=%d" % (pol, t_us), t_us, tri))
            tri = []
            for rel, target in (("below", np.nextafter(et, np.inf)), ("equal", et), ("above", np.nextafter(et, -np.inf))):
                # "below": the event's time is below L[p] + thr, so the sum is the next double above it
                tri.append(PreCase("refractory/%s" % rel, cs[k][0], cs[k][1], pol, level_for_sum(float(target), thr), 0.0))
                k += 1
            out.append(("refractory p=%d t=%d thr=%r" % (pol, t_us, thr), t_us, tri))
    return out


def precheck_planes(thr):
    """(L0, L1, S0, S1, {which: events}) of precheck_cases(thr): events of the case's polarity p ("own"), of !p
    ("other") and of both in one batch ("both"), in case order"""
    S = [np.zeros((PRE_H, PRE_W)), np.zeros((PRE_H, PRE_W))]
    L = [np.zeros((PRE_H, PRE_W)), np.zeros((PRE_H, PRE_W))]
    own, other = [], []
    for _, t_us, tri in precheck_cases(thr):
        for c in tri:
            for pol in (0, 1):
                plant(S[pol], c.x, c.y, PASSING[16], PASSING[20])
            L[c.pol][c.y, c.x], L[1 - c.pol][c.y, c.x] = c.L_own, c.L_other
            own.append(records([c.x], [c.y], t_us, c.pol))
            other.append(records([c.x], [c.y], t_us, 1 - c.pol))
    own, other = join(own), join(other)
    both = np.empty(2 * len(own), EVENT_DTYPE)
    both[0::2], both[1::2] = own, other
    return L[0], L[1], S[0], S[1], dict(own=own, other=other, both=both)


# ------------------------------------------------------------------ the border limit (:320-324)
BORDER_W, BORDER_H = 346, 260
BORDER_MIN_DISTS = (3, 10, 30)
BORDER_T_US = 5_000_000


def border_cases(min_dist):
    """[(side, (x, y) just outside the limit, (x, y) on it)], b = min_dist + 1: a centre passes from b to W - b - 1.
    The two centres of a side lie 18 pixels apart along it, so their rings stay their own."""
    W, H, b = BORDER_W, BORDER_H, min_dist + 1
    return [("left", (b - 1, 100), (b, 118)), ("top", (150, b - 1), (168, b)),
            ("right", (W - b, 140), (W - b - 1, 158)), ("bottom", (200, H - b), (218, H - b - 1))]


def border_planes(min_dist):
    """(L0, L1, S0, S1, events): passing rings on both planes at every centre of border_cases (clipped to the plane
    where min_dist 3 puts a ring pixel outside it), one event of either polarity on each, outside centre first"""
    W, H = BORDER_W, BORDER_H
    S = [np.zeros((H, W)), np.zeros((H, W))]
    L = np.zeros((H, W))
    t = float(event_times(records([0], [0], BORDER_T_US, 1))[0])
    xs, ys, ps = [], [], []
    for _, outside, on in border_cases(min_dist):
        for x, y in (outside, on):
            for pol in (0, 1):
                plant(S[pol], x, y, PASSING[16], PASSING[20])
                xs.append(x), ys.append(y), ps.append(pol)
            L[y, x] = t
    return L, L.copy(), S[0], S[1], records(xs, ys, BORDER_T_US, ps)


# ------------------------------------------------------------------ event batches
EV_W, EV_H = 346, 260
BATCH_SIZES = (1, 255, 256, 257)


def event_page():
    """a page with a mix of corners and non-corners on both planes: the twolevel rings, shuffled"""
    rng = np.random.default_rng(77)
    p1 = [(family("twolevel", 16)[i], PASSING[20]) for i in rng.permutation(240)]
    p0 = [(PASSING[16], family("twolevel", 20)[i]) for i in rng.permutation(380)]
    return pages(EV_W, EV_H, p1, p0, 5_000_000)[0]


def outside_events(page):
    """the page's events with records at x == W, y == H and 0xffff among them"""
    W, H = EV_W, EV_H
    bad = records([W, 4, 0xffff, 4, 0xffff, W, W + 1], [4, H, 4, 0xffff, 0xffff, H, H + 1], 5_000_000, [1, 0, 1, 0, 1, 0, 1])
    ev = page.events
    cut = [0, 1, 100, 255, 256, 257, len(ev)]
    parts = []
    for k in range(len(cut) - 1):
        parts += [ev[cut[k]:cut[k + 1]], bad[k:k + 1]]
    return join(parts + [bad[len(cut) - 1:]])


def repeated_pixel_events(page, n=900):
    """one corner pixel `n` times, over more than three 256-event blocks, with stamps that leave the refractory window
    part of the way through, and a non-corner pixel between them"""
    good = next(r for r in page.rings if r[3] == 1 and ring_python(r[4]))
    bad = next(r for r in page.rings if r[3] == 1 and not ring_python(r[4]))
    x = np.where(np.arange(n) % 7 == 3, bad[1], good[1])
    y = np.where(np.arange(n) % 7 == 3, bad[2], good[2])
    t_us = 5_000_000 + 20 * np.arange(n)  # L = 5.0, thr 0.01: events from 5.010020 s on are late
    return records(x, y, t_us, 1)


# ------------------------------------------------------------------ selection (Event_FeaturesToTrack)
SEL_W, SEL_H = 346, 260
SEL_MIN_DIST = 10
SEL_T_US = 5_000_000
DECAY_S = 0.020
CENTRE_BYTES = (128, 129, 127, 200, 128, 60, 130, 126)  # what a centre's own pixel renders to, by centre index mod 8


def centre_stamp(byte, t):
    """(S0, S1) of a pixel that renders to `byte` at t: round(127.5 +- 127.5 exp(-(t - s) / decay)).  128 alternates
    between never written and a positive stamp old enough to round to it."""
    if byte == 128:
        return 0.0, 0.0
    s = t + DECAY_S * np.log(abs(byte - 127.5) / 127.5)
    return (0.0, s) if byte > 128 else (s, 0.0)


_SELECTION = []


def selection_case():
    """built once"""
    if not _SELECTION:
        _SELECTION.append(_selection_case())
    return _SELECTION[0]


def _selection_case():
    """(L0, L1, S0, S1, events, mask, t): passing rings on both planes at every grid centre whose index is not 5 mod 6
    (those get a straight edge: no corner), centres' own pixels stamped to render around TS_LK_THRESHOLD, every fourth
    128 made of an old positive stamp.  The batch is every centre's event of either polarity, shuffled, twice over: the
    second copy of a pixel's candidates lies more than 256 events after the first.  The mask blocks a disc on every
    11th centre."""
    W, H = SEL_W, SEL_H
    rng = np.random.default_rng(9)
    t = float(event_times(records([0], [0], SEL_T_US, 1))[0])
    edge = (arc_ring(16, 9, 0), arc_ring(20, 11, 0))
    p = [(PASSING[16], PASSING[20]) if i % 6 != 5 else edge for i in range(len(centres(W, H)))]
    pg = pages(W, H, p, p, SEL_T_US)[0]
    S0, S1 = pg.S0.copy(), pg.S1.copy()
    mask = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for i, (x, y) in enumerate(centres(W, H)):
        byte = CENTRE_BYTES[i % 8]
        S0[y, x], S1[y, x] = centre_stamp(byte, t)
        if i % 32 == 4:
            S1[y, x] = t + DECAY_S * np.log(0.75 / 127.5)  # 127.5 + 0.75 rounds to 128
        if i % 11 == 3:
            mask[(xx - x) ** 2 + (yy - y) ** 2 <= 9] = 255
    order = rng.permutation(len(pg.events))
    ev = join([pg.events[order], pg.events[order[::-1]]])
    return pg.L0, pg.L1, S0, S1, ev, mask, t


def epoch_batches():
    """three small batches of the selection case, each with its pixels twice and more than one 256-event block, for the
    many calls on one handle that take the first-candidate map over its epoch wrap"""
    ev = selection_case()[4]
    out = []
    for k in range(3):
        part = ev[k * 40:k * 40 + 180]
        out.append(join([part, part[::-1]]))
    return out
