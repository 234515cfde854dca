"""Inputs that take calcOpticalFlowPyrLK to the edges of the device kernel (lk_point in fe_kernels.hip): windows that
drift out of the staged tile, windows at and past the image border, every way an iteration can stop, |delta|^2 within an
ulp of eps^2, sums at the top of their range, blocks with idle waves, small and odd images.  Seeded numpy only (the
tiebreak class is cut out of an oracle trace, so its builder takes the oracle module); shared by test_lk_cases.py, which
checks with the oracle's trace that each class reaches what it is for, and test_lk_edges_gpu.py, which compares the device
with the oracle on every case."""
import collections
import math

import numpy as np

USE_INITIAL_FLOW = 4
WIN = 21

Case = collections.namedtuple("Case", "name prev next pts init max_level max_count eps flags")


def _case(name, prev, nxt, pts, init=None, max_level=3, max_count=30, eps=0.01, flags=0):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    if init is not None:
        init = np.ascontiguousarray(init, np.float32).reshape(-1, 2)
    return Case(name, np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8), pts, init,
                max_level, max_count, eps, flags)


# ------------------------------------------------------------------ images
def _box(img, k):
    ker = np.ones(k) / k
    for ax in (0, 1):
        img = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), ax, img)
    return img


def lowfreq(W, H, seed, cell=16, margin=32, lo=0, hi=255):
    """random cells of `cell` px, box-blurred twice over a cell, stretched to lo..hi; (H + 2 margin, W + 2 margin)"""
    rng = np.random.default_rng(seed)
    h, w = H + 2 * margin + 2 * cell, W + 2 * margin + 2 * cell
    img = np.kron(rng.random((h // cell + 1, w // cell + 1)), np.ones((cell, cell)))[:h, :w]
    img = _box(_box(img, cell + 1), cell + 1)[cell:-cell, cell:-cell]
    img = (img - img.min()) / (img.max() - img.min())
    return lo + img * (hi - lo)


def shifted_pair(big, W, H, margin, sx, sy):
    """(prev, next) cut from one texture so that a point of prev is at + (sx, sy) in next, without wrap-around"""
    prev = big[margin:margin + H, margin:margin + W]
    nxt = big[margin - sy:margin - sy + H, margin - sx:margin - sx + W]
    return prev.astype(np.uint8), nxt.astype(np.uint8)


def stripes(W, H):
    """period 4 along x, 0 / 255: every Scharr Ix is +-4080, every Iy 0"""
    return np.tile(np.array([0, 0, 255, 255], np.uint8), (H, W // 4 + 1))[:, :W]


def checker(W, H, px):
    y, x = np.mgrid[0:H, 0:W]
    return ((((x // px) + (y // px)) & 1) * 255).astype(np.uint8)


def blocks(W, H, px, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, (H // px + 1, W // px + 1))
    return (np.kron(b, np.ones((px, px), np.int64))[:H, :W] * 255).astype(np.uint8)


def noise01(W, H, seed):
    return (np.random.default_rng(seed).integers(0, 2, (H, W)) * 255).astype(np.uint8)


def _uniform_pts(rng, n, x0, x1, y0, y1):
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1).astype(np.float32)


# ------------------------------------------------------------------ restage
RESTAGE_SHIFTS = ((14, 0), (-14, 0), (0, 9), (0, -9), (13, 8), (-11, -8))


def restage_cases():
    """one level, a texture smooth enough for LK to follow 14 px: the window leaves the 34 x 40 B tile staged at the
    level's start (more than 9 px left, 12 px right, 6 px up or down) and has to be staged again"""
    W, H, m = 160, 120, 32
    big = lowfreq(W, H, 5, cell=16, margin=m)
    rng = np.random.default_rng(50)
    pts = _uniform_pts(rng, 64, 30, W - 30, 30, H - 30)
    out = []
    for sx, sy in RESTAGE_SHIFTS:
        prev, nxt = shifted_pair(big, W, H, m, sx, sy)
        out.append(_case("restage/shift(%d,%d)" % (sx, sy), prev, nxt, pts, None, 0))
        # the same images entered from the other side: 14 px past the true position, so the window drifts back
        r = math.hypot(sx, sy)
        init = pts + np.float32([sx, sy]) + np.float32([14 * sx / r, 14 * sy / r])
        out.append(_case("restage/shift(%d,%d)+init" % (sx, sy), prev, nxt, pts, init, 0, flags=USE_INITIAL_FLOW))
    return out


# ------------------------------------------------------------------ borders
def border_origins(size):
    """window origins floor(p - 10) at which OpenCV's limits (< -win, >= size) and the tile's clamps change sides"""
    return (-22, -21, -20, -1, 0, size - 22, size - 3, size - 2, size - 1, size)


def border_cases():
    W, H, m = 96, 80, 16
    big = lowfreq(W, H, 6, cell=8, margin=m)
    half = (WIN - 1) // 2
    ex = [o + half for o in border_origins(W)]
    ey = [o + half for o in border_origins(H)]
    inner_x, inner_y = (14, 31, 48, 65, 82), (12, 26, 40, 54, 68)
    grid = [(x, y) for x in ex for y in inner_y] + [(x, y) for y in ey for x in inner_x]
    grid += [(x, y) for x in ex for y in ey]  # the corners and everything around them
    grid = np.float32(grid)
    out = []
    for sx, sy in ((3, 0), (-3, 0), (0, 3), (0, -3)):
        prev, nxt = shifted_pair(big, W, H, m, sx, sy)
        for frac in (0.0, 0.5):
            for ml in (0, 1):
                out.append(_case("borders/shift(%d,%d)/frac%.1f/L%d" % (sx, sy, frac, ml), prev, nxt,
                                 grid + np.float32(frac), None, ml))
            # a last iteration that carries the window over the limit: only the re-validation after the loop sees it
            out.append(_case("borders/shift(%d,%d)/frac%.1f/L0/count1" % (sx, sy, frac), prev, nxt,
                             grid + np.float32(frac), None, 0, 1))
            out.append(_case("borders/shift(%d,%d)/frac%.1f/L0/eps10" % (sx, sy, frac), prev, nxt,
                             grid + np.float32(frac), None, 0, 30, 10.0))
    return out


# ------------------------------------------------------------------ termination
TERM_COUNTS = (-3, 0, 1, 2, 30, 100, 150)
TERM_EPS = (-1.0, 0.0, 1e-3, 0.01, 0.3, 10.0, 20.0)


def _termination_images():
    W, H, m = 96, 80, 16
    big = lowfreq(W, H, 7, cell=8, margin=m)
    prev, nxt = shifted_pair(big, W, H, m, 2, -1)
    prev, nxt = prev.copy(), nxt.copy()
    prev[44:, 52:] = 90  # a flat corner: windows that fail the eigenvalue gate
    nxt[44:, 52:] = 90
    return prev, nxt


def termination_cases():
    W, H = 96, 80
    prev, nxt = _termination_images()
    rng = np.random.default_rng(70)
    pts = _uniform_pts(rng, 64, -14, W + 14, -14, H + 14)
    out = []
    for mc in TERM_COUNTS:
        for eps in TERM_EPS:
            out.append(_case("termination/count%d/eps%g" % (mc, eps), prev, nxt, pts, None, 1, mc, eps))
    out.append(_case("termination/same_image/eps0", prev, prev, pts, None, 1, 30, 0.0))
    # patterns on which the iteration steps back and forth
    for px, name in ((3, "checker3"), (2, "checker2")):
        c = checker(W + 2, H + 2, px)
        for sx, sy in ((1, 0), (1, 1)):
            out.append(_case("termination/%s/shift(%d,%d)" % (name, sx, sy), c[1:H + 1, 1:W + 1],
                             c[1 - sy:H + 1 - sy, 1 - sx:W + 1 - sx], pts, None, 1, 30, 0.01))
    b = blocks(W + 2, H + 2, 4, 71)
    out.append(_case("termination/blocks4/shift(1,1)", b[1:H + 1, 1:W + 1], b[0:H, 0:W], pts, None, 1, 100, 1e-3))
    out.append(oscillation_at_the_limit_case())
    return out


def int_texture(W, H, seed, cell=8):
    """a smooth texture made with integer arithmetic only (the same bytes on every platform)"""
    rng = np.random.default_rng(seed)
    k = cell
    img = np.kron(rng.integers(0, 256, (H // k + 4, W // k + 4)), np.ones((k, k), np.int64))
    for ax in (0, 1):
        for _ in range(2):
            c = np.cumsum(img, axis=ax)
            img = (np.take(c, range(k, c.shape[ax]), axis=ax) - np.take(c, range(0, c.shape[ax] - k), axis=ax)) // k
    return img[:H, :W].astype(np.uint8)


# (prev point, start) as float32 bit patterns, found by a search over 10^6 random starts 0.01 px beside points of
# int_texture(96, 80, 140) tracked into the same image: the first two steps add up to 0.01f EXACTLY in x (and to less
# in y), the largest sum the oscillation test |d + prevD| < 0.01 (in double) still accepts.  The first in the exact mode
# of the sums only, the other two in the float-order mode as well.
OSC_LIMIT_POINTS = (((1110153182, 1108243290), (1110155809, 1108243268)),
                    ((1116709530, 1104547588), (1116710850, 1104548395)),
                    ((1117241091, 1113558878), (1117242412, 1113559668)))


def search_oscillation_limit_points(O, accum, tries=1000000, seed=141, batch=4096):
    """How OSC_LIMIT_POINTS were found (not run by any test; about a minute): points of int_texture(96, 80, 140) tracked
    into the same image from a start 0.01 px to their right, two iterations, eps 0; kept where the oracle's trace shows
    an oscillation exit whose two x steps add up to +-0.01f exactly and whose y steps to no more.  If the texture's
    bytes ever change (they come from numpy's default_rng stream), run this again and replace the table.
    -> [((pt bits), (start bits))] in the table's format"""
    img = int_texture(96, 80, 140)
    rng = np.random.default_rng(seed)
    lim, found = np.float32(0.01), []
    for _ in range(0, tries, batch):
        pts = _uniform_pts(rng, batch, 12, 84, 12, 68)
        # (LK comes all the way back in two steps, so their sum is the start's offset: 0.01 in x, give or take 1e-4)
        off = np.stack([rng.uniform(0.0099, 0.0101, batch), rng.uniform(-0.004, 0.004, batch)], 1)
        init = (pts + off).astype(np.float32)
        _, _, t = O.lk_trace(img, img, pts, init, max_level=0, max_count=2, eps=0.0, flags=USE_INITIAL_FLOW, accum=accum)
        d = t.delta[:, 0]
        hit = (t.exit[:, 0] == O.LK_EXIT["oscillation"]) & (np.abs(d[:, 0, 0] + d[:, 1, 0]) == lim) & \
            (np.abs(d[:, 0, 1] + d[:, 1, 1]) <= lim)
        found += [(tuple(pts[i].view(np.uint32).tolist()), tuple(init[i].view(np.uint32).tolist())) for i in np.nonzero(hit)[0]]
    return found


def oscillation_at_the_limit_case():
    img = int_texture(96, 80, 140)
    pts = np.array([p for p, _ in OSC_LIMIT_POINTS], np.uint32).view(np.float32)
    init = np.array([q for _, q in OSC_LIMIT_POINTS], np.uint32).view(np.float32)
    return _case("termination/oscillation_sum_is_0.01f", img, img, pts, init, 0, 2, 0.0, USE_INITIAL_FLOW)


# ------------------------------------------------------------------ tiebreak
def _tiebreak_picks(O, tr, npts, on_minus_win=False):
    """(point, k, d2_k) of a level-0 trace made with eps 0: iterations whose |delta|^2 lies in [1e-8, 1] and below every
    earlier one of the point (so that an eps next to sqrt(d2_k) lets the run come as far as k).  on_minus_win: only those
    that leave the window ON the last origin the image allows in x, -WIN, with the run going on from there"""
    osc = O.LK_EXIT["oscillation"]
    picks = []
    for p in range(npts):
        n = int(tr.iters[p, 0])
        # (an oscillation exit ends the run at its last iteration: nothing before it is affected)
        if tr.exit[p, 0] == osc:
            n -= 1
        d = tr.delta[p, 0, :n].astype(np.float64)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        for k in range(n):
            if on_minus_win and not (k + 1 < int(tr.iters[p, 0]) and tr.inext[p, 0, k + 1, 0] == -WIN):
                continue
            if 1e-8 <= d2[k] <= 1.0 and (k == 0 or d2[k] * (1 + 1e-6) < d2[:k].min()):
                picks.append((p, k, float(d2[k])))
    return picks


def _eps_around(d2k):
    """sqrt(d2_k) and its two neighbours on each side"""
    e0 = math.sqrt(d2k)
    e = [e0]
    for direction in (0.0, math.inf):
        v = e0
        for _ in range(2):
            v = math.nextafter(v, direction)
            e.append(v)
    return sorted(e)


TIEBREAK_ON_MINUS_WIN = 6  # picks of the second kind, at least


def tiebreak_cases(O, accum=1, want=24):
    """|delta|^2 of a chosen iteration k within two ulps of eps^2: eps = sqrt(d2_k) and its two neighbours on each side.
    The fp32 pre-test of the kernel cannot decide these; the double compare has to.  One point per call.
    -> [(case, point index in the base run, k, d2_k, d2_k <= eps * eps)], the last in Python doubles: OpenCV's own test,
    (double)dx * dx + (double)dy * dy <= eps * eps, stops the point at iteration k exactly when it holds.
    Two kinds: `want` picks inside the image, and (names tiebreak/on_minus_win/...) picks from the border cases whose
    iteration k leaves the window on x origin -WIN: where the answer is "not converged" the kernel comes out of its loop
    and has to apply the per-iteration limit test to a window that sits exactly on the limit"""
    W, H, m = 96, 80, 16
    big = lowfreq(W, H, 8, cell=8, margin=m)
    prev, nxt = shifted_pair(big, W, H, m, 2, 1)
    rng = np.random.default_rng(80)
    pts = _uniform_pts(rng, 64, 12, W - 12, 12, H - 12)
    _, _, tr = O.lk_trace(prev, nxt, pts, None, max_level=0, max_count=30, eps=0.0, accum=accum)
    picks = _tiebreak_picks(O, tr, len(pts))
    # the picks all have small k (1 or 2 with these images: LK is nearly there after its first step); take one of
    # each k in turn so that neither is left out
    by_k = collections.defaultdict(list)
    for t in picks:
        by_k[t[1]].append(t)
    picks = []
    while len(picks) < want and any(by_k.values()):
        for k in sorted(by_k):
            if by_k[k] and len(picks) < want:
                picks.append(by_k[k].pop(0))
    out = []
    for p, k, d2k in picks:
        for eps in _eps_around(d2k):
            c = _case("tiebreak/pt%d/k%d/eps%r/accum%d" % (p, k, eps, accum), prev, nxt, pts[p:p + 1], None, 0, 30,
                      eps)
            out.append((c, p, k, d2k, d2k <= eps * eps))
    b = mirrored_onto_minus_win_case()
    _, _, tr = O.lk_trace(b.prev, b.next, b.pts, b.init, max_level=0, max_count=30, eps=0.0, flags=b.flags, accum=accum)
    picks = _tiebreak_picks(O, tr, len(b.pts), on_minus_win=True)
    seen = set()
    for p, k, d2k in picks:
        if p in seen or len(seen) >= 2 * TIEBREAK_ON_MINUS_WIN:  # one k per point
            continue
        seen.add(p)
        for eps in _eps_around(d2k):
            c = _case("tiebreak/on_minus_win/pt%d/k%d/eps%r/accum%d" % (p, k, eps, accum), b.prev, b.next,
                      b.pts[p:p + 1], b.init[p:p + 1], 0, 30, eps, b.flags)
            out.append((c, p, k, d2k, d2k <= eps * eps))
    return out


def mirrored_onto_minus_win_case():
    """Well-textured windows that settle with their x origin ON -WIN.  A window there lies wholly in the border the
    tracker reflects about column 0 (J(-u) = next(u)), so next is prev mirrored: next(x) = prev(c - x), which makes
    J(x) = prev(x + c) for x < 0 — the point at px is found at px - c, and px in [c - 11, c - 10) puts that window on
    -21.  The points come from inside the image (a full-rank A) and enter by USE_INITIAL_FLOW 1.3 px to the right"""
    W, H, m, c = 96, 80, 16, 51
    big = lowfreq(W, H, 9, cell=8, margin=m)
    prev = big[m:m + H, m:m + W]
    nxt = big[m:m + H, m + c - np.arange(W)]
    pts = np.float32([(c - 11 + fx, y + fy) for y in range(12, H - 12, 6) for fx, fy in
                      ((0.125, 0.25), (0.3, 0.0), (0.5, 0.5), (0.7, 0.75), (0.9, 0.125))])
    init = pts - np.float32([c, 0]) + np.float32([1.3, 0.4])
    return _case("borders/mirrored/onto_minus_win", prev, nxt, pts, init, 0, flags=USE_INITIAL_FLOW)


# ------------------------------------------------------------------ saturated
def saturated_cases():
    W, H = 96, 80
    rng = np.random.default_rng(90)
    pts = np.concatenate([_uniform_pts(rng, 48, -12, W + 12, -12, H + 12),
                          np.round(_uniform_pts(rng, 16, 12, W - 12, 12, H - 12))])  # (whole pixels: derivatives as they are)
    pats = (("stripes4", stripes(W, H)), ("checker3", checker(W, H, 3)), ("blocks5", blocks(W, H, 5, 94)),
            ("noise", noise01(W, H, 92)))
    out = []
    for name, prev in pats:
        nxt = np.roll(prev, (1, 1), (0, 1))
        for ml in (0, 1):
            out.append(_case("saturated/%s/L%d" % (name, ml), prev, nxt, pts, None, ml))
    dark = lowfreq(W, H, 93, cell=8, margin=0, lo=0, hi=120).astype(np.uint8)
    for ml in (0, 1):
        out.append(_case("saturated/dark+130/L%d" % ml, dark, dark + 130, pts, None, ml))
    return out


# ------------------------------------------------------------------ counts
COUNTS_MAX_CNT = 12


def counts_cases():
    """blocks of four waves with one, two and three of them idle, on a handle made for COUNTS_MAX_CNT points"""
    W, H, m = 96, 80, 16
    big = lowfreq(W, H, 10, cell=8, margin=m)
    prev, nxt = shifted_pair(big, W, H, m, -2, 1)
    rng = np.random.default_rng(100)
    pts = _uniform_pts(rng, COUNTS_MAX_CNT + 1, 5, W - 5, 5, H - 5)
    ns = (1, 2, 3, 4, 5, 7, 8, 9, COUNTS_MAX_CNT - 1, COUNTS_MAX_CNT)
    return [_case("counts/n%d" % n, prev, nxt, pts[:n], None, 1) for n in ns], \
        _case("counts/n%d(too many)" % (COUNTS_MAX_CNT + 1), prev, nxt, pts, None, 1)


# ------------------------------------------------------------------ sizes
def quarters_image(W, H, seed):
    """a constant with +-a of per-pixel noise, a different a in each quarter: texture at level 0 that pyrDown averages
    away, so the eigenvalue gate fails at the upper levels and passes at level 0"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.int64)
    amp = np.empty((H, W), np.int64)
    amp[:H // 2, :W // 2], amp[:H // 2, W // 2:], amp[H // 2:, :W // 2], amp[H // 2:, W // 2:] = 5, 7, 9, 12
    return (img + amp * (2 * rng.integers(0, 2, (H, W)) - 1)).astype(np.uint8)


def sizes_cases():
    out = []
    for k, (W, H) in enumerate(((42, 42), (43, 50), (61, 47), (173, 131))):
        m = 8
        big = lowfreq(W, H, 110 + k, cell=8, margin=m)
        prev, nxt = shifted_pair(big, W, H, m, 2, -1)
        rng = np.random.default_rng(120 + k)
        out.append(_case("sizes/%dx%d" % (W, H), prev, nxt, _uniform_pts(rng, 64, -12, W + 12, -12, H + 12), None, 3))
    W, H = 346, 260
    q = quarters_image(W + 1, H, 130)
    rng = np.random.default_rng(131)
    out.append(_case("sizes/346x260/quarters", q[:, :W], q[:, 1:], _uniform_pts(rng, 64, 20, W - 20, 20, H - 20), None, 3))
    return out


def all_cases_without_oracle():
    cases = restage_cases() + border_cases() + termination_cases() + saturated_cases() + counts_cases()[0] + sizes_cases()
    return cases


LARGEST = (346, 260)  # the largest image of any case (what a handle for all of them is made for)
MAX_POINTS = 200      # ... and at least the largest point count


# ------------------------------------------------------------------ trackImage on saturated data
def saturated_sequence(kind, frames=5, W=160, H=120, step=2):
    """0 / 255 blocks or per-pixel noise moving `step` px a frame to the right and down"""
    m = step * frames
    big = blocks(W + m, H + m, 5, 150) if kind == "blocks" else noise01(W + m, H + m, 151)
    return [big[m - step * f:m - step * f + H, m - step * f:m - step * f + W].copy() for f in range(frames)]


SEQUENCE_CONFIG = dict(max_cnt=100, min_dist=8, flow_back=1)
