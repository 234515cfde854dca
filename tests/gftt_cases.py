"""Designed inputs that take goodFeaturesToTrack on the device (k_gftt_cov, k_gftt_rowsum, k_gftt_eig, k_gftt_collect,
k_compact, k_gftt_sortprep, k_radix_pass, the Euclidean-disc selection) to its edges, and a numpy restatement of its
rules that does not go through the oracle: the float64 definition of the response, the candidate rule, the order (value,
then address, both descending) and the greedy open disc.  Every case is a Case tuple: image, mask or None, quality,
min_distance, max_corners.

The response-map and tie cases are fixed images.  The count, threshold and mask cases are cut to a response map's own
values (a quality between two candidates, a mask on exactly the peaks), so their builders take `eig_of`, a function
image -> cornerMinEigenVal map; both test files hand in the oracle's, and build(eig_of) makes every list once.  Seeded
numpy, no device code; shared by test_gftt_cases.py, which shows without a GPU that the cases reach the edges they are
for, and test_gftt_edges_gpu.py, which holds the kernels to the oracle on them."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name img mask quality min_distance max_corners")


# ------------------------------------------------------------------ the rules, restated
def response_f64(img):
    """cornerMinEigenVal by its definition in float64: the smaller eigenvalue of the 3x3-box-summed structure tensor of
    the Sobel gradients scaled by 1 / (4 * 3 * 255), BORDER_REFLECT_101"""
    f = np.asarray(img, np.float64)
    p = np.pad(f, 1, mode="reflect")
    dx = ((p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])) / 3060.0
    dy = ((p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])) / 3060.0

    def box(a):
        q = np.pad(a, 1, mode="reflect")
        return sum(q[i:i + a.shape[0], j:j + a.shape[1]] for i in range(3) for j in range(3))

    a_, b_, c_ = box(dx * dx) * 0.5, box(dx * dy), box(dy * dy) * 0.5
    return (a_ + c_) - np.sqrt((a_ - c_) ** 2 + b_ ** 2)


def threshold(eig, mask, quality):
    """(float)(max over the allowed pixels * quality), the product in double; None when nothing is allowed"""
    allowed = np.ones(eig.shape, bool) if mask is None else np.asarray(mask) != 0
    if not allowed.any():
        return None
    return np.float32(np.float64(eig[allowed].max()) * np.float64(quality))


def candidates(eig, mask=None, quality=0.01):
    """addresses (y * W + x, ascending) of the pixels the detector sorts: response above the threshold, equal to the
    3x3 maximum of the thresholded map (masked pixels take part in it), inside the one-pixel border, allowed"""
    H, W = eig.shape
    thr = threshold(eig, mask, quality)
    if thr is None:
        return np.zeros(0, np.int64)
    th = np.where(eig > thr, eig, np.float32(0))
    c = th[1:-1, 1:-1]
    dil = c.copy()
    for dy in range(3):
        for dx in range(3):
            dil = np.maximum(dil, th[dy:dy + H - 2, dx:dx + W - 2])
    take = (c != 0) & (c == dil)
    if mask is not None:
        take &= np.asarray(mask)[1:-1, 1:-1] != 0
    ys, xs = np.nonzero(take)
    return (ys + 1).astype(np.int64) * W + (xs + 1)


def order(eig, cand):
    """greaterThanPtr: by value, then by address, both descending"""
    cand = np.asarray(cand, np.int64)
    v = eig.reshape(-1)[cand].astype(np.float64)
    return cand[np.lexsort((-cand, -v))]


def greedy(xy, md, maxc):
    """a point is kept unless it lies in the open disc dx*dx + dy*dy < md*md of a kept one; stops at maxc (0: never)"""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    kept = np.zeros((len(xy), 2), np.int64)
    n = 0
    md2 = float(md) * float(md)
    for p in xy:
        d = kept[:n] - p
        if n and ((d * d).sum(1) < md2).any():
            continue
        kept[n] = p
        n += 1
        if maxc > 0 and n == maxc:
            break
    return kept[:n].astype(np.float32)


def expected(eig, case):
    """the corners of a case from a response map: candidates, order, greedy"""
    W = eig.shape[1]
    a = order(eig, candidates(eig, case.mask, case.quality))
    return greedy(np.stack([a % W, a // W], 1), case.min_distance, case.max_corners)


def tie_stats(eig, cand):
    """(groups of two or more candidates with one value, the largest group's size, groups on more than one row)"""
    W = eig.shape[1]
    cand = np.asarray(cand, np.int64)
    v = eig.reshape(-1)[cand].view(np.uint32)
    groups = spanning = largest = 0
    for bits in np.unique(v):
        rows = cand[v == bits] // W
        if rows.size >= 2:
            groups += 1
            largest = max(largest, int(rows.size))
            spanning += int(rows.min() != rows.max())
    return groups, largest, spanning


def tied_pairs(eig, corners):
    """how many of a returned list's corners share their response with another one of the list"""
    c = np.asarray(corners).astype(np.int64)
    v = eig[c[:, 1], c[:, 0]].view(np.uint32)
    return int(len(v) - len(np.unique(v)))


# ------------------------------------------------------------------ a. response map
# the smallest handle; W on both sides of one and of two 64-lane blocks, H at 2, 5, 4, 3 and 7 mod 8 (k_gftt_eig reads
# 8 rows ahead, k_gftt_cov / k_gftt_rowsum have 4-row blocks); one size that is whole blocks in both directions
RESPONSE_SIZES = ((42, 42), (63, 45), (64, 44), (65, 43), (129, 47), (128, 48))
RESPONSE_KINDS = ("noise", "binary255", "binary01", "constant", "vstep", "hstep", "dots", "border")
RANK1_KINDS = ("constant", "vstep", "hstep")      # one gradient direction at the most: the response is exactly 0
NEGATIVE_KINDS = ("dots", "binary01")             # the running column sum leaves a residue below zero
RESPONSE_MAX_CNT = 300
# {0, 1} noise: responses near 6e-6; the seed per size is the first whose map goes below zero somewhere
BINARY01_SEEDS = {(42, 42): 1, (63, 45): 1, (64, 44): 0, (65, 43): 0, (129, 47): 0, (128, 48): 0}


def dot_lattice(W, H, pitch=5, amp=255, bg=0):
    img = np.full((H, W), bg, np.uint8)
    img[pitch // 2::pitch, pitch // 2::pitch] = amp
    return img


def border_image(W, H):
    """black but for pixels on rows 0 and H-1 and on columns 0 and W-1 (the four corner pixels among them)"""
    img = np.zeros((H, W), np.uint8)
    img[0, 0::7] = 255
    img[H - 1, 3::7] = 200
    img[4::6, 0] = 255
    img[2::6, W - 1] = 180
    img[0, W - 1] = img[H - 1, 0] = img[H - 1, W - 1] = 255
    return img


def response_image(kind, W, H):
    rng = np.random.default_rng([RESPONSE_KINDS.index(kind), W, H])
    if kind == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "binary255":
        return (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8)
    if kind == "binary01":
        return np.random.default_rng(BINARY01_SEEDS[(W, H)]).integers(0, 2, (H, W), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W), 77, np.uint8)
    if kind == "vstep":
        img = np.zeros((H, W), np.uint8)
        img[:, W // 2:] = 180
        return img
    if kind == "hstep":
        img = np.zeros((H, W), np.uint8)
        img[H // 2:, :] = 180
        return img
    if kind == "dots":
        return dot_lattice(W, H)
    if kind == "border":
        return border_image(W, H)
    raise KeyError(kind)


def response_cases(W, H):
    return [Case("%s %dx%d" % (k, W, H), response_image(k, W, H), None, 0.01, 3, RESPONSE_MAX_CNT) for k in RESPONSE_KINDS]


# ------------------------------------------------------------------ b. counts and the threshold's strict comparison
# uniform noise has a local maximum at about 6.5 % of its pixels; of the sizes tried in steps of 8 this is the smallest
# with 2049 of them (seed 1: 2067)
COUNT_SIZE = (232, 136)
COUNT_SEED = 1
COUNT_MAX_CNT = 4096
# gftt_run skips the sort at n <= 1; the per-block lists are 256 wide; a radix tile is 2048 keys
COUNT_NS = (1, 2, 255, 256, 257, 2047, 2048, 2049)
COUNT_NAMES = ("n=0 quality 1", "n=0 quality 2", "n=0 constant") + tuple("n=%d" % n for n in COUNT_NS)
THRESHOLD_K = 10   # the candidate (by rank) the threshold is put on
THRESHOLD_NAMES = ("threshold == candidate %d: out" % THRESHOLD_K, "one double below: in")


def count_image():
    W, H = COUNT_SIZE
    return np.random.default_rng(COUNT_SEED).integers(0, 256, (H, W), dtype=np.uint8)


def sorted_values(eig):
    """every positive local maximum's response, descending: the candidates of any quality are a prefix of them"""
    return np.sort(eig.reshape(-1)[candidates(eig, None, 0.0)])[::-1]


def count_cases(eig_of):
    img = count_image()
    eig = eig_of(img)
    v, vmax = sorted_values(eig).astype(np.float64), np.float64(eig.max())
    W, H = COUNT_SIZE
    out = [Case(COUNT_NAMES[0], img, None, 1.0, 1, COUNT_MAX_CNT), Case(COUNT_NAMES[1], img, None, 2.0, 1, COUNT_MAX_CNT),
           Case(COUNT_NAMES[2], np.full((H, W), 131, np.uint8), None, 0.01, 1, COUNT_MAX_CNT)]
    for n in COUNT_NS:  # halfway between the n-th and the (n + 1)-th value
        out.append(Case("n=%d" % n, img, None, float((v[n - 1] + v[n]) / 2 / vmax), 1, COUNT_MAX_CNT))
    return out


def threshold_edge(vmax, v):
    """the smallest double q with (float)(vmax * q) >= v, and the double before it"""
    vmax, v = np.float64(vmax), np.float32(v)
    f = lambda q: np.float32(vmax * q)
    hi = np.float64(v) / vmax * (1 + 2.0 ** -40)
    lo = hi * (1 - 2.0 ** -20)
    assert f(lo) < v <= f(hi)
    lo, hi = int(np.float64(lo).view(np.int64)), int(np.float64(hi).view(np.int64))  # positive doubles order as integers
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(np.int64(mid).view(np.float64)) >= v:
            hi = mid
        else:
            lo = mid
    return float(np.int64(hi).view(np.float64)), float(np.int64(lo).view(np.float64))


def threshold_cases(eig_of):
    img = count_image()
    eig = eig_of(img)
    q_out, q_in = threshold_edge(eig.max(), sorted_values(eig)[THRESHOLD_K])
    return [Case(THRESHOLD_NAMES[0], img, None, q_out, 1, COUNT_MAX_CNT), Case(THRESHOLD_NAMES[1], img, None, q_in, 1, COUNT_MAX_CNT)]


# ------------------------------------------------------------------ c. ties
TIE_SIZE = (96, 72)
TIE_MAX_CNT = 8192   # the checker's plateaus: every candidate is returned
TIE_KINDS = ("dots", "squares", "checker", "tiled", "binary")
ONE_VALUE_KINDS = ("dots", "squares")
TIE_DISTANCES = (2, 2.5, 10)   # 2.5: the API takes a double
TIE_LIMITS = (1, 7)
N_TIE_CASES = len(TIE_KINDS) * (1 + len(TIE_DISTANCES) * len(TIE_LIMITS))


def square_lattice(W, H, pitch=8, amp=255, bg=128, shift=0):
    img = np.full((H, W), bg, np.uint8)
    for y in range(3, H - 4, pitch):
        for x in range(3 + shift, W - 4, pitch):
            img[y:y + 3, x:x + 3] = amp
    return img


def tie_image(kind):
    W, H = TIE_SIZE
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "dots":
        return dot_lattice(W, H, pitch=6)
    if kind == "squares":
        return square_lattice(W, H)
    if kind == "checker":  # period 4: cells of 2 x 2
        return (((xx // 2 + yy // 2) % 2) * 255).astype(np.uint8)
    if kind == "tiled":
        patch = np.random.default_rng(8).integers(0, 256, (8, 8), dtype=np.uint8)
        return np.tile(patch, (H // 8, W // 8))
    if kind == "binary":
        return (np.random.default_rng(9).integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8)
    raise KeyError(kind)


def tie_cases():
    """per image: the whole sorted candidate list (min_distance 1, no cut), then every distance with every limit"""
    out = []
    for k in TIE_KINDS:
        img = tie_image(k)
        out.append(Case("%s whole list" % k, img, None, 0.01, 1, TIE_MAX_CNT))
        out += [Case("%s md %s max %d" % (k, md, mc), img, None, 0.01, md, mc) for md in TIE_DISTANCES for mc in TIE_LIMITS]
    return out


# ------------------------------------------------------------------ d. masks (nonzero = allowed)
MASK_SIZE = (64, 48)
MASK_MAX_CNT = 300
MASK_NAMES = ("strongest masked", "peaks masked", "single interior pixel", "single pixel on row 0", "everything masked",
              "only the last pixel")
WORD_EDGE_WIDTHS = (63, 64, 65, 97)
WORD_EDGE_H = 64
WORD_EDGE_COLUMNS = (31, 0)   # x % 32: the last and the first bit of a bitmap word
N_WORD_EDGE_CASES = len(WORD_EDGE_WIDTHS) * len(WORD_EDGE_COLUMNS)


def two_level_squares():
    """one square of amplitude 255 and two of amplitude 20, whose corners stay below 1 % of the strong one's"""
    W, H = MASK_SIZE
    img = np.zeros((H, W), np.uint8)
    img[8:20, 8:24] = 255
    img[28:40, 36:52] = 20
    img[6:18, 40:56] = 20
    return img


def mask_noise(W, H):
    return np.random.default_rng([4, W, H]).integers(0, 256, (H, W), dtype=np.uint8)


def mask_cases(eig_of):
    W, H = MASK_SIZE
    sq, noise = two_level_squares(), mask_noise(W, H)
    eig = eig_of(noise)
    strongest = np.ones((H, W), np.uint8)     # "allowed" is 1 here, 255 below
    strongest[5:23, 5:27] = 0
    peaks = np.full((H, W), 255, np.uint8)    # every positive local maximum blocked: its neighbours stay suppressed
    peaks.reshape(-1)[candidates(eig, None, 0.0)] = 0
    one = np.zeros((H, W), np.uint8)          # the candidate of rank 5, alone
    one.reshape(-1)[order(eig, candidates(eig, None, 0.01))[5]] = 1
    row0 = np.zeros((H, W), np.uint8)
    row0[0, 10] = 255
    last = np.zeros((H, W), np.uint8)
    last[H - 1, W - 1] = 255
    masks = (strongest, peaks, one, row0, np.zeros((H, W), np.uint8), last)
    imgs = (sq, noise, noise, noise, noise, noise)
    return [Case(n, i, m, 0.01, 3, MASK_MAX_CNT) for n, i, m in zip(MASK_NAMES, imgs, masks)]


def word_edge_cases():
    out = []
    for W in WORD_EDGE_WIDTHS:
        img = mask_noise(W, WORD_EDGE_H)
        for col, allowed in zip(WORD_EDGE_COLUMNS, (255, 1)):
            m = np.zeros((WORD_EDGE_H, W), np.uint8)
            m[:, col::32] = allowed
            out.append(Case("columns x %% 32 == %d, W = %d" % (col, W), img, m, 0.01, 3, MASK_MAX_CNT))
    return out


# only pixels with a response below zero allowed: the maximum itself is negative, and so is the threshold.  At a quality
# below 1 the threshold lies above every allowed pixel; at 8 it lies below, and the corners have negative responses:
# of one value on the plain lattice, of several on the lattice with dots of several amplitudes, where the sort has to
# order values below zero.
NEGATIVE_MAX_NAMES = ("negative maximum, quality 0.01", "negative maximum, quality 8", "negative maximum, several values")


def mixed_dot_lattice(W, H, pitch=7):
    """the dot lattice with the right half's dots at 140 and the lower half's at 60, 100 or 140 by x % 3"""
    img = dot_lattice(W, H, pitch)
    yy, xx = np.mgrid[0:H, 0:W]
    dots = img != 0
    img[dots & (xx >= W // 2)] = 140
    low = dots & (yy >= H // 2)
    img[low] = (xx[low] % 3 * 40 + 60).astype(np.uint8)
    return img


def negative_max_cases(eig_of):
    img, mixed = dot_lattice(*TIE_SIZE, pitch=7), mixed_dot_lattice(*TIE_SIZE)
    m = np.where(eig_of(img) < 0, 255, 0).astype(np.uint8)
    out = [Case(n, img, m, q, 1, MASK_MAX_CNT) for n, q in zip(NEGATIVE_MAX_NAMES, (0.01, 8.0))]
    return out + [Case(NEGATIVE_MAX_NAMES[2], mixed, np.where(eig_of(mixed) < 0, 255, 0).astype(np.uint8), 8.0, 1, MASK_MAX_CNT)]


# ------------------------------------------------------------------ what the existing device test feeds
PARITY_PARAMS = ((160, 120, 10, False), (346, 260, 20, True))


def parity_inputs(W, H, md, use_mask):
    """the (image, mask) pairs of test_good_features_to_track_matches_oracle (tests/test_parity_gpu.py), drawn as there"""
    from esvio_amd.synth import ImageStream
    s = ImageStream(W, H, seed=W + md)
    rng = np.random.default_rng(md)
    out = []
    for k in range(2):
        img = s.next_frame()[0] if k == 0 else rng.integers(0, 256, (H, W), dtype=np.uint8)
        mask = None
        if use_mask:
            mask = np.full((H, W), 255, np.uint8)
            for _ in range(25):
                x, y = rng.integers(0, W - 30), rng.integers(0, H - 30)
                mask[y:y + rng.integers(5, 30), x:x + rng.integers(5, 30)] = 0
        out.append((img, mask))
    return out


# ------------------------------------------------------------------ everything, once
_built = {}


def build(eig_of):
    """every case list, made once per `eig_of`: {"response": {size: [...]}, "count": [...], "threshold": [...],
    "tie": [...], "mask": [...], "word_edge": [...], "negative_max": [...]}"""
    if eig_of not in _built:
        _built[eig_of] = dict(response={s: response_cases(*s) for s in RESPONSE_SIZES}, count=count_cases(eig_of),
                              threshold=threshold_cases(eig_of), tie=tie_cases(), mask=mask_cases(eig_of),
                              word_edge=word_edge_cases(), negative_max=negative_max_cases(eig_of))
    return _built[eig_of]
