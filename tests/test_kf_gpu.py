"""GPU: the keyframe stage (esvio_fe_kf_*) against tests/kf_ref.py, the sequential reading of the rules in
include/esvio_fe.h "keyframes" — byte for byte and index for index; nothing here has a tolerance.  The shapes are the
smallest at which each kernel can go wrong: the handle's minimum, an odd size below a wave's width that is no multiple
of 4, the DAVIS346 size, and a width one past a multiple of the blur tile (read from the test-side getter)."""
import ctypes as C
import os

import numpy as np
import pytest

import kf_ref as K
import shipped_configs as S
from esvio_amd import frontend as FE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def blur_tile():
    tw, th = C.c_int32(0), C.c_int32(0)
    assert FE.load_library().esvio_fe_kf_blur_tile(C.byref(tw), C.byref(th)) == 0
    return tw.value, th.value


def shapes():
    tw, th = blur_tile()
    return [(42, 42), (67, 45), (346, 260), (2 * tw + 1, max(2 * th + 3, 43))]


SHAPES = shapes()
PATTERN = FE.load_brief_pattern(os.path.join(GOLDEN, "brief_pattern.yml"))


class Dev:
    """device memory of the library's runtime: upload, download"""

    def __init__(self, nbytes, data=None):
        self.L, self.hip, self.p, self.n = FE.load_library(), C.CDLL("libamdhip64.so"), C.c_void_p(), int(nbytes)
        assert self.L.esvio_fe_mem_alloc(FE.DEVICE, max(self.n, 16), C.byref(self.p)) == 0
        if data is not None:
            a = np.ascontiguousarray(data)
            assert a.nbytes == self.n and self.L.esvio_fe_mem_upload(self.p, FE._p(a), a.nbytes) == 0

    @property
    def ptr(self):
        return self.p.value

    def get(self, dtype=np.uint8, shape=None):
        out = np.zeros(self.n, np.uint8)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.n), 2) == 0
        out = out.view(dtype)
        return out.reshape(shape) if shape else out

    def free(self):
        self.L.esvio_fe_mem_free(FE.DEVICE, self.p)


_trackers = {}


@pytest.fixture(scope="module")
def trk():
    """one handle per shape (and configuration), the pattern set"""
    def get(shape, **kw):
        key = (shape, tuple(sorted(kw.items(), key=str)))
        if key not in _trackers:
            ft = FE.FeatureTracker(FE.make_config(shape[0], shape[1], device=0, max_cnt=40, min_dist=5, **kw))
            ft.kf_set_pattern(*PATTERN)
            _trackers[key] = ft
        return _trackers[key]
    yield get
    for ft in _trackers.values():
        ft.close()
    _trackers.clear()


def rand_image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, (shape[1], shape[0]), dtype=np.uint8)


def blocky(shape, seed, cell=5, levels=(20, 90, 160, 230)):
    """cells of equal gray: plateaus of equal corner score along the cells' edges"""
    rng = np.random.default_rng(seed)
    W, H = shape
    g = rng.choice(np.array(levels, np.uint8), ((H + cell - 1) // cell, (W + cell - 1) // cell))
    return np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.uint8))[:H, :W])


# ---- blur ------------------------------------------------------------------------------------------------------------
def blur_cases(shape):
    W, H = shape
    tw, th = blur_tile()
    yy, xx = np.mgrid[0:H, 0:W]
    imp = np.zeros((H, W), np.uint8)
    for x in sorted({0, W - 1} | {s + d for s in range(tw, W, tw) for d in (-1, 0)}):
        for y in sorted({0, H - 1} | {s + d for s in range(th, H, th) for d in (-1, 0)}):
            imp[y, x] = 255 - ((x * 7 + y * 3) % 50)
    return {"random": rand_image(shape, 1), "all 255": np.full((H, W), 255, np.uint8),
            "checkerboard 1": (((xx + yy) & 1) * 255).astype(np.uint8), "checkerboard 2": ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8),
            "impulses at seams and corners": imp}


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_equals_the_rule(trk, shape):
    ft = trk(shape)
    for name, img in blur_cases(shape).items():
        got = ft.kf_blur(img)
        want = K.blur(img)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int((got != want).sum()))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_blur_from_and_into_host_and_device_memory_and_the_second_call_allocates_nothing(trk, shape):
    ft, img = trk(shape), rand_image(shape, 2)
    want = K.blur(img)
    W, H = shape
    src, dst = Dev(W * H, img), Dev(W * H + 3)
    try:
        assert np.array_equal(ft.kf_blur(src.ptr), want)
        ft.kf_blur(img, dst=dst.ptr)
        assert np.array_equal(dst.get()[:W * H].reshape(H, W), want)
        ft.kf_blur(src.ptr, dst=dst.ptr + 1)  # (a destination at an odd address: no word store may assume more)
        assert np.array_equal(dst.get()[1:W * H + 1].reshape(H, W), want)
        ft.latency_stats(reset=True)
        assert np.array_equal(ft.kf_blur(img), want) and np.array_equal(ft.kf_blur(src.ptr), want)
        ft.kf_blur(img, dst=dst.ptr)
        assert ft.latency_stats()["allocs"] == 0
    finally:
        src.free(), dst.free()


# ---- FAST ------------------------------------------------------------------------------------------------------------
def check_fast(ft, img, t):
    xy, sc, (n, nd) = ft.kf_fast(img, t, want_count=True)
    wxy, wsc, wnd = K.fast(img, t)
    assert (n, nd) == (len(wxy), wnd), (t, n, nd, len(wxy), wnd)
    assert xy.dtype == np.float32 and np.array_equal(xy, wxy) and np.array_equal(sc, wsc), t
    return wxy, wsc


def hand_made(shape):
    """the hand-made rings of tests/test_kf_ref.py at the 3-pixel border and on both sides of k_fast_score's tile seams
    (64 x 4 pixels): arcs of 9 and of 8, bright and dark, one over ring index 15 -> 0, a score of 36, an equal pair"""
    W, H = shape
    img = np.full((H, W), 100, np.int32)

    def ring(c, start, length, deltas):
        for k in range(length):
            dx, dy = K.RING[(start + k) % 16]
            img[c[1] + dy, c[0] + dx] = 100 + deltas[k % len(deltas)]
    xs = [3, W - 4] + [x for s in range(64, W - 10, 64) for x in (s - 1, s + 9)]
    cases = [(0, 9, [50]), (12, 9, [-50]), (5, 8, [50]), (3, 9, [60, 41, 37, 90, 55, 38, 37, 100, 64]), (8, 9, [-37])]
    k = 0
    for y in range(3, H - 3, 9):
        for x in xs:
            if y + 3 < H and all(abs(x - o) > 8 or x == o for o in xs):
                ring((x, y), *cases[k % len(cases)])
                k += 1
    if W > 40 and H > 30:  # two adjacent corners of equal score, away from the others
        for c in ((W // 2, H - 6), (W // 2 + 1, H - 6)):
            ring(c, 2, 9, [40])
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_fast_equals_the_rule_on_hand_made_rings_random_and_blocky_images(trk, shape):
    ft = trk(shape)
    rnd, rings = rand_image(shape, 3), hand_made(shape)
    binary = ((rand_image(shape, 4) > 200) * 255).astype(np.uint8)  # differences of 255: corners at barrier 254, none at 255
    for t in (10, 36, 37):
        check_fast(ft, rings, t)
    assert len(K.fast(rings, 10)[0]) > len(K.fast(rings, 37)[0]) > 0
    small = shape[0] * shape[1] < 20000
    for t in (0, 20, 254, 255) if small else (20,):
        check_fast(ft, rnd, t)
    for t in (254, 255):
        xy, _ = check_fast(ft, binary, t)
        assert bool(len(xy)) == (t == 254)
    check_fast(ft, blocky(shape, 5), 20)
    if small:
        low = (rand_image(shape, 6) % 3 + 100).astype(np.uint8)  # differences of 1 and 2: scores of 0 and 1 side by side
        corner, score = K.fast_scores(low, 0)
        assert (corner & (score == 0)).any()
        check_fast(ft, low, 0)


def test_fast_capacity_below_the_count_and_arc_9_of_fast_corners_is_still_refused(trk):
    shape = SHAPES[2]
    ft, img = trk(shape), rand_image(shape, 3)
    wxy, wsc, _ = K.fast(img, 20)
    assert len(wxy) > 50
    d = Dev(img.nbytes, img)
    try:
        for cap in (0, 1, 17):
            xy, sc, (n, _) = ft.kf_fast(d.ptr, 20, capacity=cap, want_count=True)
            assert n == len(wxy) and np.array_equal(xy, wxy[:cap]) and np.array_equal(sc, wsc[:cap])
    finally:
        d.free()
    with pytest.raises(FE.FrontendError, match="arc 9"):
        ft.fast_corners(img, arc=9, nonmax=True)
    xy10, sc10 = ft.fast_corners(img, arc=10, barrier=20)  # ... and the scratch the two share still serves it
    assert len(xy10) and sc10.min() >= 20
    check_fast(ft, img, 20)


# ---- BRIEF -----------------------------------------------------------------------------------------------------------
def brief_points(shape, n=1000):
    """a grid of sub-pixel offsets over the image and 30 pixels round it: the three float cases of the rule (x + x1 =
    -0.5 from the halves at the left border, -1.0 from the integers, 0.99999994f + 24), then non-finite points"""
    W, H = shape
    rng = np.random.default_rng(7)
    off = np.array([0.0, 0.25, 0.5, 0.75, 0.99999994, 0.00001], np.float32)
    x = rng.integers(-30, W + 30, n).astype(np.float32) + off[rng.integers(0, len(off), n)]
    y = rng.integers(-30, H + 30, n).astype(np.float32) + off[rng.integers(0, len(off), n)]
    pts = np.stack([x, y], 1).astype(np.float32)
    pts[:6] = [(0.99999994, 20.0), (23.5, 0.5), (2.0, 23.0), (W - 0.5, H - 0.5), (W - 24.5, H - 24.0), (W / 2, H / 2)]
    pts[6:12] = [(np.nan, 5.0), (5.0, np.inf), (-np.inf, np.nan), (40000.0, 5.0), (5.0, -32768.0), (32767.5, 5.0)]
    return pts


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_brief_equals_the_rule(trk, shape):
    ft = trk(shape)
    blurred = K.blur(rand_image(shape, 8))
    pts = brief_points(shape)
    want = K.brief(blurred, pts, PATTERN)
    assert want[:6].any(axis=1).all() and not want[6:12].any() and len({w.tobytes() for w in want}) > 500
    d = Dev(blurred.nbytes, blurred)
    out = Dev(1000 * 32)
    try:
        for n in (0, 1, 63, 64, 65, 1000):
            assert np.array_equal(ft.kf_brief(blurred if n != 65 else d.ptr, pts[:n]), want[:n]), n
        ft.kf_brief(d.ptr, pts, desc=out.ptr)
        assert np.array_equal(out.get(np.uint32, (1000, 8)), want)
        ft.latency_stats(reset=True)
        ft.kf_brief(blurred, pts)
        assert ft.latency_stats()["allocs"] == 0
        assert not ft.kf_brief(np.full_like(blurred, 77), pts).any()  # equal pixels
        ft.reset()  # the pattern is a setting
        assert np.array_equal(ft.kf_brief(blurred, pts[:65]), want[:65])
    finally:
        d.free(), out.free()


def test_brief_before_a_pattern_is_refused_and_the_pattern_is_checked():
    ft = FE.FeatureTracker(FE.make_config(42, 42, device=0, max_cnt=40, min_dist=5))
    try:
        img = rand_image((42, 42), 1)
        with pytest.raises(FE.FrontendError, match="no pattern"):
            ft.kf_brief(img, [(20.0, 20.0)])
        with pytest.raises(FE.FrontendError, match="no pattern"):
            ft.keyframe_describe(img, [(20.0, 20.0)])
        with pytest.raises(FE.FrontendError, match="256"):
            ft.kf_set_pattern(*[a[:255] for a in PATTERN])
        bad = [a.copy() for a in PATTERN]
        bad[2][100] = 128
        with pytest.raises(FE.FrontendError, match="127"):
            ft.kf_set_pattern(*bad)
        with pytest.raises(FE.FrontendError, match="no pattern"):
            ft.kf_brief(img, [(20.0, 20.0)])
        ft.kf_set_pattern(*PATTERN)
        assert np.array_equal(ft.kf_brief(K.blur(img), [(20.0, 20.0)]), K.brief(K.blur(img), [(20.0, 20.0)], PATTERN))
    finally:
        ft.close()


# ---- match -----------------------------------------------------------------------------------------------------------
def with_bits(n):
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d, bitorder="little").view("<u4")


@pytest.fixture(scope="module")
def descriptors():
    rng = np.random.default_rng(9)
    T = rng.integers(0, 2 ** 32, (5000, 8), dtype=np.uint64).astype(np.uint32)
    Q = T[rng.integers(0, 5000, 300)].copy()
    for k in range(300):  # k % 140 bits of the copy flipped: distances on both sides of 80 and 128
        flip = rng.choice(256, k % 140, replace=False)
        for b in flip:
            Q[k, b >> 5] ^= np.uint32(1 << (b & 31))
    return Q, T


def same_match(got, want, tag=""):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), tag


def test_match_equals_the_rule_at_every_size(trk, descriptors):
    ft = trk(SHAPES[0])
    Q, T = descriptors
    for nt in (0, 1, 63, 64, 65):
        want = K.match(Q[:40], T[:nt])
        same_match(ft.kf_match(Q[:40], T[:nt]), want, nt)
        if nt == 1:  # (one random descriptor: about every second query is 128 or more bits away)
            assert (want[0] < 0).any() and (want[0] == 0).any()
    want = K.match(Q, T)
    assert 0 < want[2].sum() < 300
    same_match(ft.kf_match(Q, T), want, "300 x 5000")
    got = ft.kf_match(Q[:0], T)
    assert all(len(g) == 0 for g in got)
    dq, dt = Dev(Q.nbytes, Q), Dev(T.nbytes, T)
    try:
        same_match(ft.kf_match(dq.ptr, dt.ptr, nq=300, nt=5000), want, "device")
        same_match(ft.kf_match(dq.ptr + 32 * 10, dt.ptr, nq=5, nt=65), K.match(Q[10:15], T[:65]), "device, offset")
        ft.latency_stats(reset=True)
        ft.kf_match(Q, T)
        assert ft.latency_stats()["allocs"] == 0
    finally:
        dq.free(), dt.free()


@pytest.mark.parametrize("d, idx, dist, status", [(79, 0, 79, 1), (80, 0, 80, 0), (127, 0, 127, 0), (128, -1, 128, 0), (256, -1, 128, 0)])
def test_match_boundaries(trk, d, idx, dist, status):
    got = trk(SHAPES[0]).kf_match(np.zeros((1, 8), np.uint32), with_bits(d).reshape(1, 8))
    assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == (idx, dist, status)


def test_match_takes_the_lowest_index_of_a_duplicated_minimum(trk, descriptors):
    ft = trk(SHAPES[0])
    Q, T = descriptors
    q = T[4000].copy()
    q[3] ^= np.uint32(0x3ff)  # 10 bits away from its source
    # copies of the minimum in other lanes of a wave, other waves of the workgroup, later strides of the same lane
    for places in ([4000], [300, 4000], [70, 300], [7, 70, 300, 4000], [7 + 256, 7 + 512], [7 + 512, 8 + 256], [63, 64], [255, 256], [4999, 1]):
        Tm = T.copy()
        for p in places:
            Tm[p] = T[4000]
        got = ft.kf_match(q.reshape(1, 8), Tm)
        assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == (min(places + [4000]), 10, 1), places
        same_match(got, K.match(q.reshape(1, 8), Tm), places)


# ---- describe --------------------------------------------------------------------------------------------------------
def chain(ft, img, window, t):
    """the four stage calls one after the other"""
    blurred = ft.kf_blur(img)
    xy, sc = ft.kf_fast(img, t)
    return dict(window_desc=ft.kf_brief(blurred, window), kp_xy=xy, kp_score=sc, kp_desc=ft.kf_brief(blurred, xy))


def check_describe(ft, got, img, window, t, cam, oracle):
    want_blur = K.blur(img)
    wxy, wsc, wnd = K.fast(img, t)
    assert (got["n_kp"], got["n_detected"]) == (len(wxy), wnd)
    assert np.array_equal(got["kp_xy"], wxy) and np.array_equal(got["kp_score"], wsc)
    assert np.array_equal(got["window_desc"], K.brief(want_blur, window, PATTERN))
    assert np.array_equal(got["kp_desc"], K.brief(want_blur, wxy, PATTERN))
    if oracle is not None:
        norm = np.zeros((len(wxy), 2), np.float32)
        for i, (x, y) in enumerate(wxy):
            p = oracle.lift_projective(cam, float(x), float(y))
            norm[i] = (np.float32(p[0] / p[2]), np.float32(p[1] / p[2]))
        assert len(norm) and np.array_equal(got["kp_norm"], norm)


@pytest.mark.parametrize("cams", ["pinhole only", "distorted"])
def test_describe_equals_the_stage_calls_chained_and_the_rule(trk, oracle, cams):
    shape = SHAPES[2]
    cam = S.SHIPPED["esvio_DSEC"]["img_cams"][0] if cams == "pinhole only" else S.SHIPPED["esvio"]["img_cams"][0]
    assert (cam["k1"] == 0) == (cams == "pinhole only")
    ft = FE.FeatureTracker(FE.make_config(shape[0], shape[1], device=0, max_cnt=40, min_dist=5, cams=[cam, cam]))
    try:
        ft.kf_set_pattern(*PATTERN)
        img = blocky(shape, 12, cell=9, levels=(10, 70, 140, 250)) // 2 + rand_image(shape, 13) // 8
        window = brief_points(shape, 150)
        got = ft.keyframe_describe(img, window, fast_threshold=20)
        check_describe(ft, got, img, window, 20, cam, oracle)
        for k, v in chain(ft, img, window, 20).items():
            assert np.array_equal(got[k], v), k
        # a capacity below the count: the first ones everywhere, the full count
        few = ft.keyframe_describe(img, window, fast_threshold=20, kp_capacity=9)
        assert few["n_kp"] == got["n_kp"] > 9
        for k in ("kp_xy", "kp_score", "kp_norm", "kp_desc"):
            assert np.array_equal(few[k], got[k][:9]), k
        # no window points; descriptors left on the device, matched where they lie
        none = ft.keyframe_describe(img, [], fast_threshold=20)
        assert len(none["window_desc"]) == 0 and np.array_equal(none["kp_desc"], got["kp_desc"])
        n = got["n_kp"]
        dw, dk = Dev(len(window) * 32), Dev(n * 32)
        try:
            dev = ft.keyframe_describe(img, window, fast_threshold=20, device_desc=(dw.ptr, dk.ptr))
            assert dev["window_desc"] is None and np.array_equal(dev["kp_norm"], got["kp_norm"])
            assert np.array_equal(dw.get(np.uint32, (len(window), 8)), got["window_desc"]) and np.array_equal(dk.get(np.uint32, (n, 8)), got["kp_desc"])
            same_match(ft.kf_match(dw.ptr, dk.ptr, nq=len(window), nt=n), K.match(got["window_desc"], got["kp_desc"]))
            ft.latency_stats(reset=True)
            ft.keyframe_describe(img, window, fast_threshold=20)
            assert ft.latency_stats()["allocs"] == 0
        finally:
            dw.free(), dk.free()
    finally:
        ft.close()


def test_describe_of_a_converted_device_image_and_of_the_handles_own_plane(trk):
    shape = SHAPES[2]
    W, H = shape
    ft = trk(shape)
    window = brief_points(shape, 60)
    gray = blocky(shape, 21, cell=7) // 2 + rand_image(shape, 22) // 4
    dev = ft.convert_image(gray, H, W, W, FE.ENC_MONO, device=True)
    try:
        got = ft.keyframe_describe(dev.image(0), window)
        check_describe(ft, got, gray, window, 20, None, None)
    finally:
        dev.free()
    right = np.roll(gray, 3, axis=1)
    ft.trackImage(0.1, gray, right, True)
    for cam, img in ((0, gray), (1, right)):
        plane = ft.export_image(cam)
        assert np.array_equal(plane, img)
        own, given = ft.keyframe_describe(None, window, cam=cam), ft.keyframe_describe(plane, window, cam=cam)
        for k in own:
            assert np.array_equal(own[k], given[k]), (cam, k)
        check_describe(ft, own, img, window, 20, None, None)
    assert np.array_equal(ft.kf_blur(None), K.blur(gray)) and np.array_equal(ft.kf_fast(None)[0], K.fast(gray, 20)[0])


def test_the_handles_own_plane_is_refused_with_equalize(trk):
    shape = SHAPES[1]
    ft = trk(shape, equalize=1)
    img = rand_image(shape, 30)
    for call in (lambda: ft.keyframe_describe(None, []), lambda: ft.kf_blur(None), lambda: ft.kf_fast(None)):
        with pytest.raises(FE.FrontendError, match="equalize"):
            call()
    assert np.array_equal(ft.kf_blur(img), K.blur(img))  # a caller's image is taken, and the handle is usable


def test_describe_between_track_calls_with_batches_announced_changes_no_later_result():
    from esvio_amd.events import event_times
    from esvio_amd.synth import SceneStream
    W, H = 346, 260
    s = SceneStream(W, H, rate=1e6, seed=3, n_rect=12, size=(30.0, 90.0))
    batches = [s.next_batch()[:2] for _ in range(6)]
    img, window = rand_image((W, H), 40), brief_points((W, H), 50)
    results = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
               "right_pts_velocity")

    def run(describe):
        ft = FE.FeatureTracker(FE.make_config(W, H, device=0, max_cnt=60, min_dist=8, f_ransac=1))
        out = []
        try:
            ft.kf_set_pattern(*PATTERN)
            nxt = 1
            for k, (L, R) in enumerate(batches):
                while nxt < len(batches) and nxt <= k + 2:  # two batches ahead (the first call is a plain one)
                    ft.set_next_batch(event_times(batches[nxt][0])[-1], batches[nxt][0], batches[nxt][1], True)
                    nxt += 1
                if describe:
                    d = ft.keyframe_describe(img, window)
                    assert np.array_equal(d["kp_xy"], K.fast(img, 20)[0])
                    ft.kf_match(d["window_desc"], d["kp_desc"])
                ft.trackEvent(event_times(L)[-1], L, R, True)
                out.append({n: np.array(getattr(ft, n)) for n in results})
        finally:
            ft.close()
        return out
    plain, mixed = run(False), run(True)
    assert len(plain[-1]["ids"]) > 10
    for k, (a, b) in enumerate(zip(plain, mixed)):
        for n in results:
            assert np.array_equal(a[n], b[n]), (k, n)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_every_argument_error_is_einval_with_a_message_and_leaves_the_handle_usable(trk):
    shape = SHAPES[1]
    W, H = shape
    ft = trk(shape)
    L, h, p = ft._hd.L, ft._hd.h, FE._p
    img, out, pts = rand_image(shape, 50), np.zeros((H, W), np.uint8), np.array([[20.0, 20.0]], np.float32)
    desc, n, o = np.zeros((4, 8), np.uint32), C.c_int32(0), FE.KfOut()
    res = (np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint8))
    big = np.zeros(2 * W * H, np.uint8)
    dev = Dev(256)

    def described(**kw):
        o2 = FE.KfOut()
        o2.window_desc, o2.kp_desc, o2.desc_space, o2.kp_capacity = desc.ctypes.data, None, FE.HOST, 0
        for k, v in kw.items():
            setattr(o2, k, v)
        return C.byref(o2)
    calls = {
        "blur: bad space": lambda: L.esvio_fe_kf_blur(h, p(img), 7, p(out), FE.HOST),
        "blur: bad dst space": lambda: L.esvio_fe_kf_blur(h, p(img), FE.HOST, p(out), -1),
        "blur: null dst": lambda: L.esvio_fe_kf_blur(h, p(img), FE.HOST, None, FE.HOST),
        "blur: dst is img": lambda: L.esvio_fe_kf_blur(h, p(big), FE.HOST, p(big), FE.HOST),
        "blur: dst overlaps img": lambda: L.esvio_fe_kf_blur(h, p(big), FE.HOST, C.c_void_p(big.ctypes.data + W * H - 1), FE.HOST),
        "fast: threshold -1": lambda: L.esvio_fe_kf_fast(h, p(img), FE.HOST, -1, None, None, 0, C.byref(n), None),
        "fast: threshold 256": lambda: L.esvio_fe_kf_fast(h, p(img), FE.HOST, 256, None, None, 0, C.byref(n), None),
        "fast: capacity without out_xy": lambda: L.esvio_fe_kf_fast(h, p(img), FE.HOST, 20, None, None, 5, C.byref(n), None),
        "fast: negative capacity": lambda: L.esvio_fe_kf_fast(h, p(img), FE.HOST, 20, p(desc), None, -1, C.byref(n), None),
        "fast: null n_out": lambda: L.esvio_fe_kf_fast(h, p(img), FE.HOST, 20, None, None, 0, None, None),
        "fast: bad space": lambda: L.esvio_fe_kf_fast(h, p(img), 2, 20, None, None, 0, C.byref(n), None),
        "brief: null image": lambda: L.esvio_fe_kf_brief(h, None, FE.HOST, p(pts), 1, p(desc), FE.HOST),
        "brief: negative n": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, p(pts), -1, p(desc), FE.HOST),
        "brief: n above the limit": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, p(pts), (1 << 20) + 1, p(desc), FE.HOST),
        "brief: null pts": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, None, 1, p(desc), FE.HOST),
        "brief: null desc": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, p(pts), 1, None, FE.HOST),
        "brief: bad desc space": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, p(pts), 1, p(desc), 3),
        "brief: unaligned device desc": lambda: L.esvio_fe_kf_brief(h, p(img), FE.HOST, p(pts), 1, C.c_void_p(dev.ptr + 4), FE.DEVICE),
        "match: bad space": lambda: L.esvio_fe_kf_match(h, p(desc), 1, p(desc), 1, 9, *[p(r) for r in res]),
        "match: negative nq": lambda: L.esvio_fe_kf_match(h, p(desc), -1, p(desc), 1, FE.HOST, *[p(r) for r in res]),
        "match: nt above 2^20": lambda: L.esvio_fe_kf_match(h, p(desc), 1, p(desc), (1 << 20) + 1, FE.HOST, *[p(r) for r in res]),
        "match: null train": lambda: L.esvio_fe_kf_match(h, p(desc), 1, None, 1, FE.HOST, *[p(r) for r in res]),
        "match: null results": lambda: L.esvio_fe_kf_match(h, p(desc), 1, p(desc), 1, FE.HOST, None, p(res[1]), p(res[2])),
        "match: unaligned device descriptors": lambda: L.esvio_fe_kf_match(h, C.c_void_p(dev.ptr + 8), 1, C.c_void_p(dev.ptr + 32), 1, FE.DEVICE, *[p(r) for r in res]),
        "describe: null out": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), 1, 20, None),
        "describe: cam 2": lambda: L.esvio_fe_kf_describe(h, 2, p(img), FE.HOST, p(pts), 1, 20, described()),
        "describe: threshold 300": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), 1, 300, described()),
        "describe: null window_pts": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, None, 1, 20, described()),
        "describe: null window_desc": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), 1, 20, described(window_desc=None)),
        "describe: negative n_window": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), -2, 20, described()),
        "describe: negative capacity": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), 1, 20, described(kp_capacity=-1)),
        "describe: bad desc space": lambda: L.esvio_fe_kf_describe(h, 0, p(img), FE.HOST, p(pts), 1, 20, described(desc_space=5)),
        "describe: bad space": lambda: L.esvio_fe_kf_describe(h, 0, p(img), 5, p(pts), 1, 20, described()),
    }
    try:
        ft.latency_stats(reset=True)
        ft.kf_blur(img), ft.kf_fast(img), ft.kf_brief(img, pts), ft.kf_match(desc, desc), ft.keyframe_describe(img, pts)
        ft.latency_stats(reset=True)
        for name, call in calls.items():
            L.esvio_fe_reset(h)  # (clears nothing of the message: each refusal must write its own)
            assert call() == -1, name
            msg = L.esvio_fe_last_error(h).decode()
            assert msg.startswith("kf_" + name.split(":")[0]), (name, msg)
        assert ft.latency_stats()["allocs"] == 0  # refused before any device work
        assert np.array_equal(ft.kf_blur(img), K.blur(img))
        assert np.array_equal(ft.keyframe_describe(img, pts)["kp_xy"], K.fast(img, 20)[0])
    finally:
        dev.free()
