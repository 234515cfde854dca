"""The keyframe stage's rules (include/esvio_fe.h "keyframes": B, F, D, M) read sequentially in numpy: what
tests/test_kf_gpu.py holds the device against, byte for byte.  Nothing here shares a trick with the kernels: the corner
score comes from trying the barriers, not from fe_kernels.hip's (or tests/fast_ref.py's) doubling steps."""
import numpy as np

TAPS = np.array([7, 17, 32, 46, 52, 46, 32, 17, 7], np.int64)  # getGaussianKernel(9, 2.0) x 256, rounded; sum 256
BEST_INIT, MATCH_DIST = 128, 80
# the radius-3 ring from (0, 3) through (3, 0), (0, -3), (-3, 0)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
        (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def reflect101(p, n):
    p = np.where(p < 0, -p, p)
    return np.where(p >= n, 2 * n - 2 - p, p)


def blur(img):
    """B[y][x] = (sum_j sum_i c_j c_i I[r(y+j-4)][r(x+i-4)] + 32768) >> 16.  The double sum is taken row pass first,
    in integers, nothing rounded between the passes: the same number by distributivity."""
    I = np.asarray(img, np.uint8).astype(np.int64)
    H, W = I.shape
    rows = np.zeros((H, W), np.int64)
    for i in range(9):
        rows += TAPS[i] * I[:, reflect101(np.arange(W) + i - 4, W)]
    out = np.zeros((H, W), np.int64)
    for j in range(9):
        out += TAPS[j] * rows[reflect101(np.arange(H) + j - 4, H), :]
    return ((out + 32768) >> 16).astype(np.uint8)


def _is_corner(c, ring, b):
    """9 contiguous of the 16 ring pixels all > c + b or all < c - b; c [n], ring [16, n]"""
    br, dk = ring > c + b, ring < c - b
    out = np.zeros(c.shape, bool)
    for s in range(16):
        k = [(s + j) % 16 for j in range(9)]
        out |= br[k].all(0) | dk[k].all(0)
    return out


def fast_scores(img, t):
    """(corner map at barrier t, score map): score = the largest barrier at which the pixel still is a corner, found
    by trying them one after the other; 0 for every pixel that is no corner at t"""
    I = np.asarray(img, np.uint8).astype(np.int32)
    H, W = I.shape
    corner = np.zeros((H, W), bool)
    score = np.zeros((H, W), np.int32)
    if W < 7 or H < 7:
        return corner, score
    ys, xs = np.mgrid[3:H - 3, 3:W - 3]
    ys, xs = ys.ravel(), xs.ravel()
    c = I[ys, xs]
    ring = np.stack([I[ys + dy, xs + dx] for dx, dy in RING])
    alive = np.nonzero(_is_corner(c, ring, t))[0]
    corner[ys[alive], xs[alive]] = True
    b = t
    while len(alive):
        score[ys[alive], xs[alive]] = b
        b += 1
        alive = alive[_is_corner(c[alive], ring[:, alive], b)]  # (nobody is a corner at 255: the loop ends)
    return corner, score


def fast(img, t):
    """F(I, t) -> (xy float32 [n, 2] in raster order, score int32 [n], corners before the non-max)"""
    corner, score = fast_scores(img, t)
    H, W = score.shape
    keep = corner.copy()
    pad = np.pad(score, 1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ys, xs = np.nonzero(keep)  # (row-major: raster order)
    return np.stack([xs, ys], 1).astype(np.float32).reshape(-1, 2), score[ys, xs].astype(np.int32), int(corner.sum())


def brief(blurred, pts, pattern):
    """D(Bimg, p) for every (x, y) of pts -> uint32 [n, 8]; the loop of BRIEF.cpp:84-106 with np.float32 additions"""
    B = np.asarray(blurred, np.uint8)
    H, W = B.shape
    x1, y1, x2, y2 = [np.asarray(a, np.int32).astype(np.float32) for a in pattern]
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros((len(pts), 8), np.uint32)
    for k, (px, py) in enumerate(pts):
        if not (np.isfinite(px) and np.isfinite(py)) or abs(px) >= 32768 or abs(py) >= 32768:
            continue
        with np.errstate(all="ignore"):
            X1, Y1 = np.trunc(np.float32(px) + x1).astype(np.int64), np.trunc(np.float32(py) + y1).astype(np.int64)
            X2, Y2 = np.trunc(np.float32(px) + x2).astype(np.int64), np.trunc(np.float32(py) + y2).astype(np.int64)
        inside = (X1 >= 0) & (X1 < W) & (Y1 >= 0) & (Y1 < H) & (X2 >= 0) & (X2 < W) & (Y2 >= 0) & (Y2 < H)
        bit = np.zeros(len(x1), np.uint8)
        bit[inside] = B[Y1[inside], X1[inside]] < B[Y2[inside], X2[inside]]
        out[k] = np.packbits(bit, bitorder="little").view("<u4")  # bit i: word i >> 5, bit i & 31
    return out


def hamming(q, T):
    """popcount(q xor T_i) for every row of T"""
    x = np.bitwise_xor(np.asarray(T, np.uint32).reshape(-1, 8), np.asarray(q, np.uint32).reshape(1, 8))
    return np.unpackbits(x.view(np.uint8), axis=1).sum(1).astype(np.int64) if len(x) else np.zeros(0, np.int64)


def match(Q, T):
    """M(Q, T) -> (idx int32, dist int32, status uint8); the loop of keyframe.cpp:191-202 for every query"""
    Q = np.asarray(Q, np.uint32).reshape(-1, 8)
    idx, dist, status = np.zeros(len(Q), np.int32), np.zeros(len(Q), np.int32), np.zeros(len(Q), np.uint8)
    for k, q in enumerate(Q):
        best_dist, best_index = BEST_INIT, -1
        for i, dis in enumerate(hamming(q, T).tolist()):
            if dis < best_dist:
                best_dist, best_index = dis, i
        idx[k], dist[k], status[k] = best_index, best_dist, int(best_index != -1 and best_dist < MATCH_DIST)
    return idx, dist, status
