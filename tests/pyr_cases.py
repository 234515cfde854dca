"""Level-0 images that take the LK image chain to its edges, and the pyramid the oracle expects of them: every level's
image with its 24-pixel BORDER_REFLECT_101 ring and its Scharr derivatives with their all-zero ring.  The chain under
test is the one a track call runs (build_lk_images in fe_stages.cpp): time surface -> k_pyr3 -> k_pad_scharr, with
`equalize` k_clahe_lut / k_clahe_interp -> k_norm_pyr -> k_pad_scharr, and the unfused kernels behind ESVIO_FE_NO_FUSE,
a median, an imported right image and trackImage.  Seeded numpy plus the oracle, no device code; shared by
test_pyr_cases.py, which shows without a GPU that the inputs reach those edges, and test_pyr_levels_gpu.py, which reads
the built pyramids back (esvio_fe_export_level) and compares every byte."""
import collections

import numpy as np

from esvio_amd.events import event_times, make_events

PAD = 24          # kPad (fe_kernels.h)
DECAY_MS = 20.0   # make_config's default
TILES = 8         # CLAHE's grid

# (W, H) -> the level widths x heights oracle.pyr_levels gives (test_pyr_cases.py asserts them)
FOUR_LEVEL = {
    (169, 169): ((169, 169), (85, 85), (43, 43), (22, 22)),
    (176, 176): ((176, 176), (88, 88), (44, 44), (22, 22)),
    (176, 169): ((176, 169), (88, 85), (44, 43), (22, 22)),
    (169, 176): ((169, 176), (85, 88), (43, 44), (22, 22)),
    (192, 176): ((192, 176), (96, 88), (48, 44), (24, 22)),
    (200, 169): ((200, 169), (100, 85), (50, 43), (25, 22)),
    (346, 260): ((346, 260), (173, 130), (87, 65), (44, 33)),
    (352, 264): ((352, 264), (176, 132), (88, 66), (44, 33)),
}
SMALL = {  # one- and two-level handles (image handles only: an event handle's fused build needs four levels)
    (42, 42): ((42, 42),),
    (43, 50): ((43, 50), (22, 25)),
    (61, 47): ((61, 47), (31, 24)),
}

Frame = collections.namedtuple("Frame", "name left right")  # two level-0 images (uint8, H x W)


def level_sizes(W, H):
    return FOUR_LEVEL.get((W, H)) or SMALL[(W, H)]


# ------------------------------------------------------------------ the expected pyramid
def reflect101_once(p, n):
    """the device's reflect101 (fe_kernels.hip): ONE reflection, valid for -n < p < 2 n - 1"""
    p = np.abs(np.asarray(p))
    return np.where(p >= n, 2 * n - 2 - p, p)


def ring_source_index(n):
    """source index of every position of a padded row of an n-pixel level: BORDER_REFLECT_101 with as many reflections as
    it takes (numpy's "reflect")"""
    return np.pad(np.arange(n), PAD, mode="reflect")


def expected_pyramid(O, img0):
    """[(image (h + 2 PAD, w + 2 PAD) u8, derivatives (h + 2 PAD, w + 2 PAD, 2) int16)] per level of oracle.pyr_levels"""
    img0 = np.ascontiguousarray(img0, np.uint8)
    H, W = img0.shape
    out, cur = [], img0
    for l in range(O.pyr_levels(W, H) + 1):
        if l:
            cur = O.pyr_down(cur)
        dv = np.zeros((cur.shape[0] + 2 * PAD, cur.shape[1] + 2 * PAD, 2), np.int16)
        dv[PAD:-PAD, PAD:-PAD] = O.scharr(cur)
        out.append((np.pad(cur, PAD, mode="reflect"), dv))
    return out


def pyr_down_sums(img):
    """cv::pyrDown's 5 x 5 sums before the (sum + 128) >> 8 (numpy restatement: [1 4 6 4 1] both ways, REFLECT_101)"""
    k = (1, 4, 6, 4, 1)
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    a = np.pad(img.astype(np.int64), 2, mode="reflect")
    r = sum(k[i] * a[:, i:i + 2 * dw - 1:2] for i in range(5))
    return sum(k[j] * r[j:j + 2 * dh - 1:2, :] for j in range(5))


# ------------------------------------------------------------------ level 0 per path
def level0(O, kind, img):
    """what a path makes of the rendered time surface (event handles) or of the caller's image (image handles)"""
    if kind == "plain":
        return img
    if kind == "equalize":      # trackEvent with equalize: CLAHE, then normalize(0, 255, NORM_MINMAX)
        return O.normalize_minmax(O.clahe(img))
    if kind == "image_equalize":  # trackImage with equalize: the node's CLAHE alone
        return O.clahe(img)
    if kind.startswith("median"):
        return O.median_blur(img, 2 * int(kind[6:]) + 1)
    raise ValueError(kind)


# ------------------------------------------------------------------ SAE planes whose time surface is a wanted image
def planes_for(img, t, decay_s=DECAY_MS / 1000.0):
    """(S0, S1) with round(127.5 +- 127.5 exp(-(t - s) / decay)) = img; 128: no event (both 0).  The oracle's rendering
    of the planes is the truth, so a byte the inversion misses by one is still a valid case."""
    b = img.astype(np.float64)
    v = np.abs(b - 127.5) / 127.5
    s = t + decay_s * np.log(v)
    unset = img == 128
    S1 = np.where((img > 128) & ~unset, s, 0.0)
    S0 = np.where((img < 128) & ~unset, s, 0.0)
    return S0, S1


def frame_time(k):
    """(time of frame k as the track call gets it, its one event per camera): the smallest batch a track call takes"""
    t_us = 10_000_000 + 50_000 * k
    ev = make_events([0], [0], [t_us], [1])
    return float(event_times(ev)[-1]), t_us


def frame_events(W, H, t_us):
    return make_events([W // 2], [H // 2], [t_us], [1]), make_events([W // 3], [H // 3], [t_us], [0])


def oracle_surfaces(O, W, H, frame, k):
    """the frame's planes and events through the oracle's detector -> (t, left events, right events, planes per camera,
    rendered surfaces per camera)"""
    t, t_us = frame_time(k)
    evs = frame_events(W, H, t_us)
    det = O.Detector(W, H, decay_ms=DECAY_MS)
    Z = np.zeros((H, W))
    planes, ts = [], []
    for cam, img in enumerate((frame.left, frame.right)):
        S0, S1 = planes_for(img, t)
        det.set_sae(cam, Z, Z, S0, S1)
        det.create_sae(cam, evs[cam])
        planes.append((S0, S1))
        ts.append(det.time_surface(cam, t))
    return t, evs[0], evs[1], planes, ts


# ------------------------------------------------------------------ contents
DENSE_FRAMES = 4  # three left slots, two right slots: the fourth frame writes over the first one's rings


def dense_frames(W, H):
    """every pixel set, stamps in [t - 3 decay, t], a random polarity: |v| >= e^-3, so no byte is 127 or 128"""
    out = []
    for f in range(DENSE_FRAMES):
        rng = np.random.default_rng(1000 * f + W + 7 * H)
        imgs = []
        for cam in range(2):
            v = np.exp(-rng.uniform(0.0, 3.0, (H, W)))
            sign = rng.integers(0, 2, (H, W)) * 2 - 1
            imgs.append(np.rint(127.5 + 127.5 * sign * v).astype(np.uint8))
        out.append(Frame("dense/%d" % f, imgs[0], imgs[1]))
    return out


def stripes(W, H, run, axis):
    y, x = np.mgrid[0:H, 0:W]
    return ((((x if axis == 0 else y) // run) & 1) * 255).astype(np.uint8)


def ties_image(W, H):
    """per-pixel noise, from the first seed with which a pyrDown sum of EVERY level is 128 mod 256 (the
    (sum + 128) >> 8 tie), and whose four corner pixels differ from both of their neighbours"""
    for seed in range(256):
        rng = np.random.default_rng(5000 + seed)
        img = rng.integers(0, 256, (H, W)).astype(np.uint8)
        for cy, cx, ny, nx in ((0, 0, 1, 1), (0, W - 1, 1, W - 2), (H - 1, 0, H - 2, 1), (H - 1, W - 1, H - 2, W - 2)):
            img[cy, cx], img[cy, nx], img[ny, cx] = 255, 0, 0
        cur, ok = img, True
        for _ in range(len(level_sizes(W, H)) - 1):
            s = pyr_down_sums(cur)
            ok = ok and bool(((s & 255) == 128).any())
            cur = ((s + 128) >> 8).astype(np.uint8)
        if ok:
            return img
    raise AssertionError("no seed gives a tie at every level of %d x %d" % (W, H))


def extremes_frames(W, H):
    imgs = [("x%d" % r, stripes(W, H, r, 0)) for r in (1, 2, 3)] + [("y%d" % r, stripes(W, H, r, 1)) for r in (1, 2, 3)]
    imgs.append(("ties", ties_image(W, H)))
    n = len(imgs)
    return [Frame("extremes/" + imgs[i][0], imgs[i][1], imgs[(i + 3) % n][1]) for i in range(n)]


def clahe_geometry(W, H):
    """(EW, EH, tile width, tile height, clip) as cv::CLAHE (clipLimit 40, 8 x 8 tiles) has them: both sides are extended
    as soon as one is no multiple of 8, the divisible one by a full 8"""
    EW, EH = W, H
    if not (W % TILES == 0 and H % TILES == 0):
        EW, EH = W + TILES - W % TILES, H + TILES - H % TILES
    tw, th = EW // TILES, EH // TILES
    return EW, EH, tw, th, max(int(40.0 * (tw * th) / 256), 1)


def clahe_tile_stats(img):
    """numpy restatement of the clip step of CLAHE's LUT, per tile: [(clipped, residual, distinct values)] in tile order"""
    H, W = img.shape
    EW, EH, tw, th, clip = clahe_geometry(W, H)
    ext = np.pad(img, ((0, EH - H), (0, EW - W)), mode="reflect")
    out = []
    for ty in range(TILES):
        for tx in range(TILES):
            h = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
            clipped = int(np.maximum(h - clip, 0).sum())
            out.append((clipped, clipped % 256, int((h > 0).sum())))
    return out


CLAHE_CLASSES = ("no_clip", "residual_0", "step_ge_2", "step_1", "one_value")


def clahe_tile_classes(img):
    """the names of CLAHE_CLASSES that occur among the image's tiles (redistribution: residual 0 adds nothing; 1..128
    steps through the bins 256 / residual >= 2 apart; above 128 the step is 1)"""
    got = set()
    for clipped, residual, values in clahe_tile_stats(img):
        if values == 1:
            got.add("one_value")
        if clipped == 0:
            got.add("no_clip")
        elif residual == 0:
            got.add("residual_0")
        elif residual <= 128:
            got.add("step_ge_2")
        else:
            got.add("step_1")
    return got


def attainable_clahe_classes(W, H):
    """a tile of `area` pixels clips at most area - clip of them: residual 0 with something clipped needs 256, a
    residual above 128 needs 129 (the tiles of the one- and two-level sizes have 36 to 48 pixels)"""
    _, _, tw, th, clip = clahe_geometry(W, H)
    room = tw * th - clip
    return {c for c in CLAHE_CLASSES if not (c == "residual_0" and room < 256) and not (c == "step_1" and room < 129)}


def _peak_tile(rng, area, clip, extra, lo=0):
    """one value holds clip + extra pixels (so `extra` are clipped), no other more than clip"""
    peak = int(rng.integers(lo, 256))
    others = rng.permutation(np.array([v for v in range(lo, 256) if v != peak]))
    t = np.concatenate([np.full(clip + extra, peak), np.resize(others, area - clip - extra)])
    assert area - clip - extra <= clip * len(others)
    return rng.permutation(t)


def two_valued_tiles(W, H, seed):
    """every CLAHE tile holds two values, half of its pixels each, above a floor per image: most of every tile is clipped
    and spread over all 256 bins, so the CLAHE output starts far above 0 (its minimum is about 40 + 0.7 of the floor)"""
    _, _, tw, th, _ = clahe_geometry(W, H)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    tile = (y // th) * TILES + x // tw
    a = rng.integers(int(rng.integers(40, 200)), 254, TILES * TILES)
    b = np.array([rng.integers(v + 1, 256) for v in a])
    return np.where(rng.integers(0, 2, (H, W)).astype(bool), a[tile], b[tile]).astype(np.uint8)


def shift_frame(O, W, H, k):
    """A frame for the SHIFT of the normalisation.  The shift is -smin * scale, computed in double and rounded to float
    once; computed in float from the rounded scale it is another float for most (smin, smax), but that moves a byte only
    where pixel * scale + shift lies next to a rounding tie: for about one (smin, smax) pair in seventeen, and then for one
    to eight pixel values.  So the frame is searched: the first two_valued_tiles image whose CLAHE output, taken of the
    surface the detector renders of it as the left camera's frame k, normalises differently under
    normalize_shift_in_float.  The right camera gets the same image but cannot tell the two apart: its one event has
    polarity 0 and renders a 0 pixel, whose CLAHE output is at most 2, and for smin <= 2 the two shifts are one float."""
    for seed in range(7400, 7600):
        img = two_valued_tiles(W, H, seed)
        eq = O.clahe(oracle_surfaces(O, W, H, Frame("", img, img), k)[4][0])
        if not np.array_equal(normalize_restated(eq), normalize_shift_in_float(eq)):
            return Frame("clahe/shift", img, img)
    raise AssertionError("no two-valued image tells the two shifts apart at %d x %d" % (W, H))


def clahe_frames(O, W, H, k0):
    """the CLAHE images of a handle; k0: the index of the first of them among the handle's frames"""
    EW, EH, tw, th, clip = clahe_geometry(W, H)
    area = tw * th
    extras = [e for e in (0, 256, 1, 100, 128, 129, 200, 255, area - clip) if clip + e <= area]

    def designed(seed, lo):
        rng = np.random.default_rng(seed)
        img = rng.integers(lo, 256, (EH, EW))
        k = 0
        for ty in range(TILES):
            for tx in range(TILES):
                if (ty + 1) * th > H or (tx + 1) * tw > W:
                    continue  # (a tile that holds reflected pixels keeps its noise)
                e = extras[k % len(extras)]
                k += 1
                if e == 0 and clip * (256 - lo) >= area:
                    t = rng.permutation(np.resize(rng.permutation(np.arange(lo, 256)), area))  # flat: nothing clipped
                else:
                    t = _peak_tile(rng, area, clip, e, lo)
                img[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = t.reshape(th, tw)
        return img[:H, :W].astype(np.uint8)

    y, x = np.mgrid[0:H, 0:W]
    tile = (y // th) * TILES + x // tw
    const_tiles = ((37 * tile + 11) % 256).astype(np.uint8)
    const_tiles_b = ((101 * tile + 64) % 256).astype(np.uint8)
    flat = np.full((H, W), 90, np.uint8)
    out = [Frame("clahe/tiles", designed(7000 + W + H, 0), designed(7100 + W + H, 0)),
           Frame("clahe/tiles_floor60", designed(7200 + W + H, 60), designed(7300 + W + H, 60)),
           Frame("clahe/constant_tiles", const_tiles, const_tiles_b),
           Frame("clahe/constant", flat, flat)]
    if (W, H) in FOUR_LEVEL:  # (the sizes that have an event handle: image handles do not normalise)
        out.append(shift_frame(O, W, H, k0 + len(out)))
    return out


def scene_frame(O, W, H):
    """one SceneStream batch through the oracle's detector: the production statistics (mostly 128)"""
    from esvio_amd.synth import SceneStream
    L, R, _ = SceneStream(W, H, rate=2e6, seed=21).next_batch()
    det = O.Detector(W, H, decay_ms=DECAY_MS)
    det.create_sae(0, L)
    det.create_sae(1, R)
    t = float(event_times(L)[-1])
    return Frame("scene", det.time_surface(0, t), det.time_surface(1, t))


_FRAMES = {}


def frames(O, W, H, clahe=False):
    """the frames of a handle in the order they are tracked, built once per size: dense (the slots rotate under them),
    extremes, the scene frame; `clahe`: the CLAHE tile images after them"""
    if (W, H) not in _FRAMES:
        base = dense_frames(W, H) + extremes_frames(W, H)
        if (W, H) in FOUR_LEVEL:
            base.append(scene_frame(O, W, H))
        _FRAMES[(W, H)] = (base, clahe_frames(O, W, H, len(base)))
    base, cl = _FRAMES[(W, H)]
    return base + cl if clahe else list(base)


# ------------------------------------------------------------------ normalize, restated
def normalize_restated(img):
    """k_normalize's / pyr3_body<1>'s arithmetic in numpy: scale and shift in double, rounded to float, one float multiply
    and one float add per pixel"""
    smin, smax = float(img.min()), float(img.max())
    scale = 255.0 * (1.0 / (smax - smin) if smax - smin > 2.2204460492503131e-16 else 0.0)
    fa, fb = np.float32(scale), np.float32(0.0 - smin * scale)
    r = np.rint((img.astype(np.float32) * fa).astype(np.float32) + fb)
    return np.clip(r, 0, 255).astype(np.uint8)


def normalize_shift_in_float(img):
    """the same with the shift computed in float from the rounded scale, fb = -(float)smin * fa: what shift_frame's
    images tell from the right arithmetic"""
    smin, smax = float(img.min()), float(img.max())
    scale = 255.0 * (1.0 / (smax - smin) if smax - smin > 2.2204460492503131e-16 else 0.0)
    fa = np.float32(scale)
    fb = np.float32(-np.float32(smin) * fa)
    r = np.rint((img.astype(np.float32) * fa).astype(np.float32) + fb)
    return np.clip(r, 0, 255).astype(np.uint8)
