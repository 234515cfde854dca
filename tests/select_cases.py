"""Candidate lists that put the min-distance selection (tests/select_ref.py; k_select_mw / k_select / k_select_gbm on
the device) on its edges.  Everything is deterministic; the seeds are written below.  tests/test_select_cases.py shows
on the CPU that the families reach the edges they are named for, tests/test_select_edges_gpu.py runs every case through
esvio_fe_select_candidates.

A case is a dict: family, name, W, H, kind ('circle' | 'euclid'), d (radius | min_distance), xy (uint32 x | y << 16),
payload (int32), mask ((H, W) u8 or None), stamps ((k, 2) float32 or None), max_corners, out_base, meta.

Sizes (the smallest with the property each is for; wpr = 32-bit words per bitmap row):
  64x48    wpr 2, 96 words     W a multiple of 32
  75x45    wpr 3, 135 words    word count mod 4 = 3: the tails of the bitmap's init / copy loops
  97x67    wpr 4, 268 words    exactly one valid bit in a row's last word
  173x131  wpr 6, 786 words    (mod 4 = 2) room for a whole radius-63 disc
  346x260  wpr 11, 2860 words  a shipped sensor
and, to reach the other two kernels the way a handle reaches them, 1280x960 with max_cnt 300 (bitmap in LDS, no room
for the 16-wave kernel's queue: k_select) and 1440x1080 (bitmap in device memory: k_select_gbm), one boundary family
and one dense family each.

Dense lists (family i) need 20 accepted and 20 refused candidates; a sensor that cannot hold 20 discs of a radius does
not get that radius:
  64x48    circle 3              75x45   circle 3, euclid 5        97x67  circle 3, 10
  173x131  circle 3, 10, 15, 16  346x260 circle 3, 15, 16, 31, 32, euclid 17, 33
  1280x960 circle 63             1440x1080 circle 32
"""
import numpy as np

from select_ref import fill_disc, halfwidths, pack_xy, select

SMALL = [(64, 48), (75, 45), (97, 67), (173, 131), (346, 260)]
MAX_CNT_SMALL = 2600  # room for every candidate of the longest list (family d: 2500, all accepted)
LARGE_ONE_WAVE = (1280, 960)
LARGE_GBM = (1440, 1080)
MAX_CNT = {s: MAX_CNT_SMALL for s in SMALL}
MAX_CNT[LARGE_ONE_WAVE] = 300
MAX_CNT[LARGE_GBM] = 300

CIRCLE_R = [3, 10, 15, 16, 31, 32, 63]
EUCLID_D = [1, 2, 5, 16, 17, 30, 32, 33, 40, 63]  # 5, 30, 40: lattice points at distance exactly d: (3,4) (18,24) (24,32)
DISCS = [("circle", r) for r in CIRCLE_R] + [("euclid", d) for d in EUCLID_D]
N_FILLER = 1100  # more than the 1024 candidates of one filter pass of the 16-wave kernel

SEED_DENSE = 20261019
SEED_LENGTHS = 7
SEED_BORDER = 11


def _case(family, name, size, disc, xy, payload=None, mask=None, stamps=None, max_corners=None, out_base=0, meta=None):
    W, H = size
    xy = np.asarray(xy, np.uint32).reshape(-1)
    assert ((xy & 0xffff) < W).all() and ((xy >> 16) < H).all(), name
    if payload is None:
        payload = (np.arange(xy.size, dtype=np.int64) * 7 + 13).astype(np.int32)
    mc = MAX_CNT[size]
    max_corners = mc - out_base if max_corners is None else max_corners
    assert 0 <= max_corners and out_base + max_corners <= mc
    return dict(family=family, name="%s %dx%d %s%g %s" % (family, W, H, disc[0][0], disc[1], name), W=W, H=H, kind=disc[0],
                d=disc[1], xy=xy, payload=np.asarray(payload, np.int32), mask=mask,
                stamps=None if stamps is None else np.asarray(stamps, np.float32).reshape(-1, 2),
                max_corners=int(max_corners), out_base=int(out_base), meta=meta or {})


def expected(case, **wrong):
    """what select_ref makes of the case (kept with the case: computed once, shared by every test that needs it);
    wrong: a wrong copy's switches, or hw=<table> for a wrong table (never kept)"""
    if not wrong and "_expected" in case:
        return case["_expected"]
    hw = wrong.pop("hw", None)
    if hw is None:
        hw = halfwidths(case["kind"], case["d"])
    out = select(case["W"], case["H"], case["xy"], case["payload"], hw, case["mask"], case["stamps"], case["max_corners"],
                 case["out_base"], **wrong)
    if not wrong and hw == halfwidths(case["kind"], case["d"]):
        case["_expected"] = out
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- a: boundary probes
def probe_offsets(hw):
    """per |dy| in 0..r+1 and sign quadrant: the disc row's last pixel and the first one outside (|dy| = r+1: dx = 0)
    -> [(dx, dy, |dy|, inside)], no offset twice"""
    r = len(hw) - 1
    out, seen = [], set()
    for ady in range(r + 2):
        for sy in (1, -1):
            for sx in (1, -1):
                for dx, inside in ((hw[ady], True), (hw[ady] + 1, False)) if ady <= r else ((0, False),):
                    o = (sx * dx, sy * ady)
                    if o not in seen:
                        seen.add(o)
                        out.append((o[0], o[1], ady, inside))
    return out


def _cells(size, r):
    """anchor positions whose pairs (anchor, probe within r+1 of it) stay more than r pixels apart, Chebyshev, from
    every pixel of every other pair: nobody's verdict depends on another pair"""
    W, H = size
    pitch, span = 3 * r + 3, 2 * r + 3
    return [(cx * pitch + r + 1, cy * pitch + r + 1) for cy in range((H - span) // pitch + 1 if H >= span else 0)
            for cx in range((W - span) // pitch + 1 if W >= span else 0)]


def family_a(size=(346, 260), discs=DISCS, per_call=32):
    """Each probe twice: right behind its anchor in the anchor's own 64-candidate sub-chunk (the kill is geometric),
    and behind the anchors and N_FILLER duplicates of their pixels (a later filter pass: the verdict is the bitmap's).
    Up to 32 pairs per call, so that the anchors are one resolve / one sub-chunk and all of them are accepted."""
    cases = []
    for disc in discs:
        hw = halfwidths(*disc)
        r = len(hw) - 1
        cells = _cells(size, r)
        assert cells, (size, disc)
        k = min(per_call, len(cells))
        offs = probe_offsets(hw)
        for c0 in range(0, len(offs), k):
            chunk = offs[c0:c0 + k]
            ax = np.array([cells[i][0] for i in range(len(chunk))])
            ay = np.array([cells[i][1] for i in range(len(chunk))])
            px = ax + np.array([o[0] for o in chunk])
            py = ay + np.array([o[1] for o in chunk])
            A, P = pack_xy(ax, ay), pack_xy(px, py)
            meta = dict(ady=np.array([o[2] for o in chunk]), inside=np.array([o[3] for o in chunk]))
            n = len(chunk)
            inter = np.empty(2 * n, np.uint32)
            inter[0::2], inter[1::2] = A, P
            cases.append(_case("a", "chunk %d" % c0, size, disc, inter,
                               meta=dict(meta, anchor_idx=np.arange(0, 2 * n, 2), probe_idx=np.arange(1, 2 * n, 2))))
            fill = A[np.arange(N_FILLER) % n]
            cases.append(_case("a", "bitmap %d" % c0, size, disc, np.concatenate([A, fill, P]),
                               meta=dict(meta, anchor_idx=np.arange(n + N_FILLER), probe_idx=n + N_FILLER + np.arange(n))))
    return cases


# ---------------------------------------------------------------------------------------- b: borders
def border_anchors(size, r):
    W, H = size
    rx, ry = min(r, W - 1), min(r, H - 1)
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2),
            (1, H // 2), (rx, H // 2), (W - 2, H // 2), (W - 1 - rx, H // 2), (W // 2, 1), (W // 2, ry), (W // 2, H - 2),
            (W // 2, H - 1 - ry)]


def border_probes(size, hw, ax, ay):
    """the boundary probes of family (a) that lie inside the sensor — the refused ones first: they leave the bitmap as
    the anchor made it — then, for every row the disc reaches and the rows next to them, the first and last pixels of
    the row and the pixels at its first word boundary: where a disc row that is not clipped, or that spills into the
    next word, shows"""
    W, H = size
    r = len(hw) - 1
    offs = probe_offsets(hw)
    pts = [(ax + o[0], ay + o[1]) for o in offs if o[3]] + [(ax + o[0], ay + o[1]) for o in offs if not o[3]]
    for y in range(ay - r - 2, ay + r + 3):
        pts += [(x, y) for x in (0, 1, 31, 32, W - 2, W - 1)]
    out, seen = [], {(ax, ay)}
    for p in pts:
        if 0 <= p[0] < W and 0 <= p[1] < H and p not in seen:
            seen.add(p)
            out.append(p)
    return out


B_DISCS = [("circle", 3), ("circle", 15), ("circle", 16), ("circle", 31), ("circle", 32), ("circle", 63), ("euclid", 5),
           ("euclid", 17), ("euclid", 33)]
# what a kept point's coordinates look like: ties on even and on odd integers, both signs, and near-ties
B_FRACTIONS = [(0.5, 0.5), (-0.5, -0.5), (0.5, -0.5), (0.0, 0.5), (0.49, -0.49), (-0.5, 0.0), (0.51, 0.5), (0.0, 0.0)]


def family_b(sizes=SMALL, discs=B_DISCS):
    cases = []
    for size in sizes:
        W, H = size
        for disc in discs:
            hw = halfwidths(*disc)
            for k, (ax, ay) in enumerate(border_anchors(size, len(hw) - 1)):
                pr = border_probes(size, hw, ax, ay)
                xy = pack_xy([ax] + [p[0] for p in pr], [ay] + [p[1] for p in pr])
                cases.append(_case("b", "anchor %d (%d,%d)" % (k, ax, ay), size, disc, xy, meta=dict(anchor=(ax, ay))))
                # the same pixel as a kept point: (x + fx, y + fy), flipped where it would round out of the sensor
                fx, fy = B_FRACTIONS[(k + len(cases)) % len(B_FRACTIONS)]
                sx = ax + fx if -0.5 <= ax + fx and np.rint(np.float32(ax + fx)) <= W - 1 else ax - fx
                sy = ay + fy if -0.5 <= ay + fy and np.rint(np.float32(ay + fy)) <= H - 1 else ay - fy
                qx, qy = int(np.rint(np.float32(sx))), int(np.rint(np.float32(sy)))
                pr = [(qx, qy)] + border_probes(size, hw, qx, qy)
                cases.append(_case("b", "stamp %d (%g,%g)" % (k, sx, sy), size, disc,
                                   pack_xy([p[0] for p in pr], [p[1] for p in pr]), stamps=[(sx, sy)],
                                   meta=dict(anchor=(qx, qy), frac=(sx, sy))))
    return cases


# ---------------------------------------------------------------------------------------- c: word geometry
C_SIZES = [(64, 48), (97, 67)]
C_RADII = [3, 15, 16, 31, 32]


def word_anchor_xs(W, r):
    xs = {x for x in range(W) if (x & 31) in (0, 1, 30, 31)}
    xs |= {x for x in range(r, W) if ((x - r) & 31) == 31}   # the centre row starts at bit 31
    xs |= {x for x in range(W - r) if ((x + r) & 31) == 0}    # ... ends at bit 0 of the next word
    xs |= {W - 1, max(W - 1 - r, 0)}                          # ... ends in the row's last (partial) word
    return sorted(xs)


def family_c(sizes=C_SIZES, radii=C_RADII):
    """Anchors on the word edges, then the WHOLE bitmap read back through probes.  A probe that is accepted blocks a
    disc itself, so one list of all pixels would hide most bits behind earlier probes.  Instead, per anchor set:
      * one call with every pixel the reference has blocked: all refused, nothing stamped — reads every set bit;
      * the free pixels in classes (x mod r+1, y mod r+1): two probes of a class are more than r apart, Chebyshev, so
        none lies in another's disc and every verdict is the anchors' bitmap's — reads every clear bit.
    Anchor sets: all word-edge columns as candidates in both orders (the greedy keeps some), a few as kept points."""
    cases = []
    for size in sizes:
        W, H = size
        for r in radii:
            disc = ("circle", r)
            hw = halfwidths(*disc)
            xs = word_anchor_xs(W, r)
            ys = [min(r + 1, H - 1), H // 2, max(H - 2 - r, 0), 0, H - 1]
            anchors = [(x, ys[i % len(ys)]) for i, x in enumerate(xs)]
            few = anchors[::max(1, len(anchors) // (12 if r <= 3 else 3))]
            sets = [("fwd", anchors, None), ("stamps", [], few)] if r > 16 else \
                   [("fwd", anchors, None), ("rev", anchors[::-1], None), ("stamps", [], few)]
            for tag, cand, stamps in sets:
                A = pack_xy([a[0] for a in cand], [a[1] for a in cand])
                st = None if stamps is None else np.array(stamps, np.float32)
                # the bitmap the anchors leave, by the reference: the discs of the anchors it accepts and of the kept points
                kept = select(W, H, A, np.zeros(A.size, np.int32), hw, None, st)[0]
                bm = bytearray(W * H)
                for px, py in list(kept) + ([] if st is None else list(np.rint(st))):
                    fill_disc(bm, W, H, int(px), int(py), hw)
                m = np.frombuffer(bytes(bm), np.uint8).reshape(H, W) != 0
                yy, xx = np.nonzero(m)
                cases.append(_case("c", "%s blocked" % tag, size, disc, np.concatenate([A, pack_xy(xx, yy)]), stamps=st,
                                   meta=dict(n_anchor=A.size, blocked=True)))
                yy, xx = np.nonzero(~m)
                cls = (xx % (r + 1)) * (r + 1) + (yy % (r + 1))
                for g in np.unique(cls):
                    sel = cls == g
                    cases.append(_case("c", "%s free %d" % (tag, g), size, disc, np.concatenate([A, pack_xy(xx[sel], yy[sel])]),
                                       stamps=st, meta=dict(n_anchor=A.size, blocked=False)))
    return cases


# ---------------------------------------------------------------------------------------- d: list lengths
D_TOTALS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1087, 1088, 1089, 2500]


def far_apart(size, r, n, seed):
    """n pixels on a grid of pitch r + 1 (nobody in anybody's disc), in a shuffled order"""
    W, H = size
    gx, gy = np.meshgrid(np.arange(0, W, r + 1), np.arange(0, H, r + 1))
    p = np.random.default_rng(seed).permutation(gx.size)[:n]
    assert p.size == n
    return pack_xy(gx.ravel()[p], gy.ravel()[p])


def family_d(size=(346, 260), disc=("circle", 3)):
    cases = []
    for n in D_TOTALS:
        cases.append(_case("d", "far %d" % n, size, disc, far_apart(size, 3, n, SEED_LENGTHS + n)))
        k = np.arange(n)
        cases.append(_case("d", "clump %d" % n, size, disc, pack_xy(100 + k % 3, 100 + (k // 3) % 3)))  # 3x3: all in all discs
    return cases


# ---------------------------------------------------------------------------------------- e: one-wave thresholds
def family_e(size=(346, 260), disc=("circle", 3)):
    """sub-chunks of 64 with a set number of live candidates, the rest on masked pixels; where they sit in a 256 step"""
    W, H = size
    mask = np.zeros((H, W), np.uint8)
    mask[H - 1, :] = 255  # the blocked candidates' pixels
    blocked = lambda n, o=0: pack_xy((o + np.arange(n)) % W, np.full(n, H - 1))
    cases = []

    def chunk(live_xy, seed):
        """64 candidates: the live ones at shuffled lanes, in their order"""
        lanes = np.sort(np.random.default_rng(seed).permutation(64)[:len(live_xy)])
        c = blocked(64, seed)
        c[lanes] = live_xy
        return c
    for live in (4, 5, 8, 9, 16, 17):
        for pos in range(4):
            xy = np.concatenate([blocked(64 * pos), chunk(far_apart(size, 3, live, live), 100 * live + pos), blocked(64 * (3 - pos)),
                                 far_apart(size, 3, 40, 99)])
            cases.append(_case("e", "live %d at %d" % (live, pos), size, disc, xy, mask=mask, meta=dict(live=live)))
    for acc in (12, 13):  # 20 live at the sub-chunk's start, `acc` accepted: the others lie in an earlier one's disc
        lead = far_apart(size, 3, acc, 5)
        dup = pack_xy((lead[:20 - acc] & 0xffff) + 1, lead[:20 - acc] >> 16)
        for pos in range(4):
            xy = np.concatenate([blocked(64 * pos), chunk(np.concatenate([lead, dup]), 7 * acc + pos), blocked(64 * (3 - pos)),
                                 far_apart(size, 3, 40, 98)])
            cases.append(_case("e", "accepted %d at %d" % (acc, pos), size, disc, xy, mask=mask, meta=dict(acc=acc)))
    for steps in (1, 2):  # whole steps of 256 blocked candidates, then live ones
        cases.append(_case("e", "%d blocked steps" % steps, size, disc, np.concatenate([blocked(256 * steps), far_apart(size, 3, 3, 4)]),
                           mask=mask))
    return cases


# ---------------------------------------------------------------------------------------- f: max_corners
def family_f(size=(346, 260), disc=("circle", 3)):
    cases = []
    far = far_apart(size, 3, 200, 21)
    rng = np.random.default_rng(SEED_DENSE + 1)
    mixed = pack_xy(rng.integers(0, size[0], 1500), rng.integers(0, size[1], 1500))
    for tag, xy in (("far", far), ("mixed", mixed)):
        full = select(size[0], size[1], xy, np.zeros(xy.size, np.int32), halfwidths(*disc))[2][0]
        # 1; inside a batch / a resolve of 64 (the second one); exactly on a batch's end; one more than there are
        for mc in (1, 70, 64, 128, full - 1, full, full + 1):
            for ob in (0, 7):
                cases.append(_case("f", "%s max %d base %d" % (tag, mc, ob), size, disc, xy, max_corners=mc, out_base=ob,
                                   meta=dict(full=int(full))))
    return cases


# ---------------------------------------------------------------------------------------- g: seeds
def family_g(sizes=SMALL):
    cases = []
    for size in sizes:
        W, H = size
        rng = np.random.default_rng(SEED_BORDER + W)
        every = pack_xy(*[a.ravel() for a in np.meshgrid(np.arange(W), np.arange(H))])
        mask = np.where(rng.random((H, W)) < 0.5, 255, 0).astype(np.uint8)
        mask[:, W - 1] = 255 * (np.arange(H) % 2)
        mask[H - 1, :] = 255 * (np.arange(W) % 3 == 0)
        # min_distance 1 is the disc of one pixel: every pixel as a candidate reads the seeded bitmap back bit by bit
        # (the shortest sensors' whole pixel count fits max_cnt; the others are cut at max_cnt accepted, and read in parts)
        for lo in range(0, every.size, 4000):
            cases.append(_case("g", "mask read %d" % lo, size, ("euclid", 1), every[lo:lo + 4000], mask=mask))
        grey = mask.copy()
        grey[mask == 0] = rng.integers(0, 255, (H, W), dtype=np.uint8)[mask == 0]  # only 255 blocks
        cases.append(_case("g", "mask grey", size, ("euclid", 1), every[:4000], mask=grey))
        cand = pack_xy(rng.integers(0, W, 600), rng.integers(0, H, 600))
        stamps = np.stack([rng.uniform(-0.5, W - 1, 9), rng.uniform(-0.5, H - 1, 9)], 1).astype(np.float32)
        stamps[:4] = np.floor(stamps[:4]) + 0.5
        for disc in (("circle", 3), ("circle", 16), ("euclid", 33)):
            cases.append(_case("g", "neither", size, disc, cand))
            cases.append(_case("g", "mask", size, disc, cand, mask=mask))
            cases.append(_case("g", "stamps", size, disc, cand, stamps=stamps))
            cases.append(_case("g", "both", size, disc, cand, mask=mask, stamps=stamps))
            cases.append(_case("g", "one stamp", size, disc, cand, stamps=stamps[:1]))
        full = np.full((H, W), 255, np.uint8)
        cases.append(_case("g", "all blocked", size, ("circle", 3), cand, mask=full))
        one = full.copy()
        one[int(cand[300] >> 16), int(cand[300] & 0xffff)] = 0
        cases.append(_case("g", "all but one", size, ("circle", 3), cand, mask=one, meta=dict(only=int(cand[300]))))
    return cases


# ---------------------------------------------------------------------------------------- h: duplicates and ties
def family_h(size=(346, 260)):
    cases = []
    for disc in (("circle", 3), ("circle", 16), ("euclid", 5)):
        r = len(halfwidths(*disc)) - 1
        pts = far_apart(size, r, 12, 3)
        for copies in (2, 3, 5):
            # the copies right behind the first one, and spread over later sub-chunks
            cases.append(_case("h", "adjacent x%d" % copies, size, disc, np.repeat(pts, copies)))
            cases.append(_case("h", "spread x%d" % copies, size, disc, np.concatenate([np.tile(pts, copies)[:12], far_apart(size, r, 12, 3)[::-1],
                                                                                         np.tile(pts, copies)])))
        a, b = pack_xy([50], [60]), pack_xy([50 + r], [60])  # each in the other's disc
        far = far_apart(size, r, 5, 8)
        cases.append(_case("h", "pair ab", size, disc, np.concatenate([a, b, far])))
        cases.append(_case("h", "pair ba", size, disc, np.concatenate([b, a, far])))
    return cases


# ---------------------------------------------------------------------------------------- i: dense lists
I_DISCS = {
    (64, 48): [("circle", 3)],
    (75, 45): [("circle", 3), ("euclid", 5)],
    (97, 67): [("circle", 3), ("circle", 10)],
    (173, 131): [("circle", 3), ("circle", 10), ("circle", 15), ("circle", 16)],
    (346, 260): [("circle", 3), ("circle", 15), ("circle", 16), ("circle", 31), ("circle", 32), ("euclid", 17), ("euclid", 33)],
    LARGE_ONE_WAVE: [("circle", 63)],
    LARGE_GBM: [("circle", 32)],
}


def dense_lists(size, seed):
    W, H = size
    rng = np.random.default_rng(seed)
    uni = pack_xy(rng.integers(0, W, 3000), rng.integers(0, H, 3000))
    cx, cy = rng.integers(0, W, 20), rng.integers(0, H, 20)
    k = rng.integers(0, 20, 3000)
    sd = max(min(W, H) / 12.0, 3.0)
    clu = pack_xy(np.clip(np.rint(cx[k] + rng.normal(0, sd, 3000)), 0, W - 1).astype(np.int64),
                  np.clip(np.rint(cy[k] + rng.normal(0, sd, 3000)), 0, H - 1).astype(np.int64))
    return uni, clu


def family_i(sizes=SMALL):
    cases = []
    for size in sizes:
        uni, clu = dense_lists(size, SEED_DENSE + size[0])
        for disc in I_DISCS[size]:
            cases.append(_case("i", "uniform", size, disc, uni))
            cases.append(_case("i", "clustered", size, disc, clu))
    return cases


# ---------------------------------------------------------------------------------------- the sets the tests run
_cache = {}


def small_cases():
    """every case of every family on the five small sensors, by family letter"""
    if "small" not in _cache:
        _cache["small"] = dict(a=family_a(), b=family_b(), c=family_c(), d=family_d(), e=family_e(), f=family_f(),
                               g=family_g(), h=family_h(), i=family_i())
    return _cache["small"]


LARGE_A_DISCS = [("circle", 15), ("circle", 16), ("circle", 63), ("euclid", 33)]


def large_cases(size):
    """one boundary family and one dense family at a size that takes another kernel"""
    if size not in _cache:
        _cache[size] = dict(a=family_a(size, LARGE_A_DISCS), i=family_i([size]))
    return _cache[size]
