"""GPU: esvio_fe_fast_corners (k_fast_score + k_fast_collect + k_compact) against outputs of the reference's own
compiled FAST (tests/golden/fast_ref_*.npz, see tests/golden/make_fast_ref.py) and, on inputs the fixtures do not
hold, against the numpy restatement tests/fast_ref.py that tests/test_fast_ref.py ties to those fixtures.
Integers only: every comparison is equality, element for element and in order; no case is left out."""
import ctypes as C
import os

import numpy as np
import pytest

import fast_ref
from esvio_amd import frontend as FE
from esvio_amd.events import event_times
from esvio_amd.synth import SceneStream
from test_fast_ref import FILES, fixture_cases

pytestmark = pytest.mark.gpu


class DeviceImage:
    """a (H, W) u8 image in device memory of the library's own HIP runtime"""

    def __init__(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        self.ptr = C.c_void_p()
        L = FE.load_library()
        assert L.esvio_fe_mem_alloc(FE.DEVICE, img.nbytes, C.byref(self.ptr)) == 0
        assert L.esvio_fe_mem_upload(self.ptr, img.ctypes.data_as(C.c_void_p), img.nbytes) == 0

    def free(self):
        FE.load_library().esvio_fe_mem_free(FE.DEVICE, self.ptr)


def _handle(W, H, **kw):
    return FE.FeatureTracker(FE.make_config(W, H, **kw))


def _check_against(ft, img, arg, b, d9, d10, s10, nm, tag):
    """every mode of the call on one image and barrier"""
    xy, sc, (n, nd) = ft.fast_corners(arg, arc=9, barrier=b, nonmax=False, want_count=True)
    assert sc is None and n == len(d9) and nd == len(d9), (tag, "detect_9 count", n, len(d9))
    assert xy.dtype == np.int16 and np.array_equal(xy, d9), (tag, "detect_9")
    xy, sc, (n, nd) = ft.fast_corners(arg, arc=10, barrier=b, nonmax=False, want_count=True)
    assert n == len(d10) and nd == len(d10), (tag, "detect_10 count", n, len(d10))
    assert np.array_equal(xy, d10), (tag, "detect_10")
    assert sc.dtype == np.int32 and np.array_equal(sc, s10), (tag, "score_10")
    xy, sc, (n, nd) = ft.fast_corners(arg, arc=10, barrier=b, nonmax=True, want_count=True)
    assert n == len(nm) and nd == len(d10), (tag, "nonmax count", n, len(nm), nd, len(d10))
    assert np.array_equal(xy, d10[nm]) and np.array_equal(sc, s10[nm]), (tag, "nonmax_3x3")


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[9:-4] for f in FILES])
def test_fast_equals_reference_fixtures(path):
    """every fixture image x barrier x {9, 10} x non-max on / off, image in host and in device memory
    (the 7x7 / 6x9 images are below the smallest handle, 42 x 42: the restatement alone covers them)"""
    handles, n = {}, 0
    for name, img, b, d9, d10, s10, nm in fixture_cases(path):
        H, W = img.shape
        if W < 42 or H < 42:
            assert name.startswith("tiny")
            continue
        if (W, H) not in handles:
            handles[(W, H)] = _handle(W, H)
        ft = handles[(W, H)]
        dev = DeviceImage(img)
        for space, arg in (("host", img), ("device", dev.ptr.value)):
            _check_against(ft, img, arg, b, d9, d10, s10, nm, (name, b, space))
        dev.free()
        n += 1
    assert n >= 2
    for ft in handles.values():
        ft.close()


def _ref(img, b, maps=None):
    m9, m10 = maps if maps is not None else (fast_ref.score_map(img, 9), fast_ref.score_map(img, 10))
    d9, _ = fast_ref.detect(img, 9, b, m9)
    d10, s10 = fast_ref.detect(img, 10, b, m10)
    return d9, d10, s10, fast_ref.nonmax_3x3(d10, s10, img.shape)


@pytest.mark.parametrize("W,H", [(346, 260), (641, 479), (1279, 721), (42, 42), (70, 45)])
def test_fast_equals_restatement_on_seeded_images(W, H):
    """widths that are no multiple of the tile / block width, the smallest handle, barrier 0 and 255, an all-equal
    image, and a capacity below the count"""
    rng = np.random.default_rng(W * 1000 + H)
    smooth = np.kron(rng.integers(0, 256, (H // 5 + 1, W // 5 + 1)), np.ones((5, 5)))[:H, :W]
    images = {
        "noise": rng.integers(0, 256, (H, W)).astype(np.uint8),
        "blocks": np.clip(smooth + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8),
        "sparse": (rng.random((H, W)) < 0.02).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8),
        "extremes": rng.choice(np.array([0, 255], np.uint8), (H, W)),
        "equal": np.full((H, W), 131, np.uint8),
    }
    ft = _handle(W, H)
    for name, img in images.items():
        dev = DeviceImage(img)
        maps = (fast_ref.score_map(img, 9), fast_ref.score_map(img, 10))
        for b in (0, 20, 254, 255):
            d9, d10, s10, nm = _ref(img, b, maps)
            print(name, (W, H), "barrier", b, "n9", len(d9), "n10", len(d10), "nonmax", len(nm))
            _check_against(ft, img, img if b != 20 else dev.ptr.value, b, d9, d10, s10, nm, (name, W, H, b))
        dev.free()
    assert len(_ref(images["extremes"], 254)[1]) > 0 and len(_ref(images["extremes"], 255)[1]) == 0
    assert len(_ref(images["equal"], 0)[0]) == 0
    # capacity below the count: the first entries in raster order, the full counts
    img = images["blocks"]
    d9, d10, s10, nm = _ref(img, 7)
    assert len(nm) > 12
    for cap in (0, 1, len(nm) // 2, len(nm) - 1, len(nm), len(nm) + 5):
        xy, sc, (n, nd) = ft.fast_corners(img, barrier=7, nonmax=True, capacity=cap, want_count=True)
        k = min(cap, len(nm))
        assert n == len(nm) and nd == len(d10) and len(xy) == k, (cap, n, nd)
        assert np.array_equal(xy, d10[nm][:k]) and np.array_equal(sc, s10[nm][:k]), cap
    xy, sc, (n, nd) = ft.fast_corners(img, arc=9, barrier=7, nonmax=False, capacity=3, want_count=True)
    assert n == len(d9) and np.array_equal(xy, d9[:3]) and sc is None
    ft.close()


def test_fast_rejects_bad_arguments():
    ft = _handle(64, 48)
    hd, L = ft._hd, ft._hd.L
    img = np.zeros((48, 64), np.uint8)
    xy, sc = np.zeros((8, 2), np.int16), np.zeros(8, np.int32)
    n = C.c_int32(0)

    def call(arc=10, barrier=20, nonmax=1, score=True, cam=0, image=img, space=FE.HOST, cap=8, n_out=n):
        return L.esvio_fe_fast_corners(hd.h, cam, image.ctypes.data_as(C.c_void_p) if image is not None else None, space,
                                       arc, barrier, nonmax, xy.ctypes.data_as(C.c_void_p),
                                       sc.ctypes.data_as(C.c_void_p) if score else None, cap,
                                       C.byref(n_out) if n_out is not None else None, None)

    assert call() == 0 and n.value == 0
    for kw in (dict(arc=8), dict(arc=11), dict(arc=12), dict(arc=0), dict(barrier=-1), dict(barrier=256),
               dict(arc=9, nonmax=1, score=False), dict(arc=9, nonmax=0, score=True), dict(nonmax=2), dict(space=7),
               dict(image=None, cam=2), dict(image=None, cam=-1), dict(cap=-1)):
        assert call(**kw) == -1, kw  # ESVIO_FE_EINVAL
        assert b"fast_corners" in L.esvio_fe_last_error(hd.h), kw
    assert call(n_out=None) == -1
    assert call(arc=9, nonmax=0, score=False) == 0
    with pytest.raises(FE.FrontendError):
        ft.fast_corners(img, arc=9, nonmax=True)
    ft.close()


@pytest.mark.parametrize("W,H,rate,equalize", [(346, 260, 1e6, 0), (640, 480, 4e6, 0), (640, 480, 4e6, 1),
                                               (1280, 720, 6e6, 0)])
@pytest.mark.parametrize("replay", [False, True])
def test_fast_on_the_handles_time_surface(W, H, rate, equalize, replay):
    """img == NULL reads the plane esvio_fe_get_time_surface returns, in place (a padded pyramid level: stride !=
    width), for both cameras, at the sensor sizes of C1 / C3 / C5, after plain calls and inside a replay schedule
    with batches announced ahead; with equalize the surface lies in the raw planes, not in the LK pyramid"""
    s = SceneStream(W, H, rate=rate, seed=5 + W)
    batches = [s.next_batch()[:2] for _ in range(5)]
    ft = _handle(W, H, max_cnt=150, equalize=equalize)
    if replay:
        ft.set_lazy_new_stereo(True)
    announced, total = 0, 0
    for f, (L, R) in enumerate(batches):
        if replay:
            while announced < min(f + 2, len(batches) - 1):
                announced += 1
                La, Ra = batches[announced]
                ft.set_next_batch(event_times(La)[-1], La, Ra, True)
        ft.trackEvent(event_times(L)[-1], L, R, True)
        if f in (0, 2, 4):
            for cam in (0, 1):
                ts = ft.gettimesurface(cam)
                d9, d10, s10, nm = _ref(ts, 20)
                xy, sc = ft.fast_corners(cam=cam, barrier=20, nonmax=True)
                assert np.array_equal(xy, d10[nm]) and np.array_equal(sc, s10[nm]), (f, cam, "nonmax")
                xy, sc = ft.fast_corners(cam=cam, arc=9, barrier=20, nonmax=False)
                assert np.array_equal(xy, d9), (f, cam, "detect_9")
                assert np.array_equal(ft.gettimesurface(cam), ts)
                total += len(d9)
    assert total > 100
    ft.close()


def _run_sequence(W, H, batches, pubs, replay, with_fast):
    kw = dict(max_cnt=150)
    ft = _handle(W, H, **kw)
    if replay:
        ft.set_lazy_new_stereo(True)
        ft.set_launch_thread(True)
    out, announced = [], 0
    for f, (L, R) in enumerate(batches):
        if replay:
            while announced < min(f + 3, len(batches) - 1):
                announced += 1
                La, Ra = batches[announced]
                ft.set_next_batch(event_times(La)[-1], La, Ra, pubs[announced])
        ft.trackEvent(event_times(L)[-1], L, R, pubs[f])
        if with_fast:
            for cam in (0, 1):
                xy, _ = ft.fast_corners(cam=cam, barrier=20, nonmax=bool(f % 2))
                assert len(xy) > 0
            ft.fast_corners(np.full((H, W), f, np.uint8), arc=9, nonmax=False)
        out.append([ft.ids.copy(), ft.track_cnt.copy(), ft.cur_pts.copy(), ft.cur_un_pts.copy(), ft.pts_velocity.copy()])
    ft.finish()
    out.append([ft.ids.copy(), ft.track_cnt.copy(), ft.ids_right.copy(), ft.cur_pts.copy(), ft.cur_un_pts.copy(),
                ft.pts_velocity.copy(), ft.cur_right_pts.copy(), ft.cur_un_right_pts.copy(), ft.right_pts_velocity.copy(),
                ft.gettimesurface(0), ft.gettimesurface(1)])
    ft.close()
    return out


@pytest.mark.parametrize("replay", [False, True])
def test_fast_does_not_interfere_with_tracking(replay):
    """the same trackEvent sequence with and without fast_corners calls after every frame: ids, counts and every
    float vector bit for bit (the LK mode is the suite's ESVIO_LK_ACCUM switch)"""
    W, H = 640, 480
    s = SceneStream(W, H, rate=4e6, seed=77)
    batches = [s.next_batch()[:2] for _ in range(9)]
    pubs = [(f % 3) != 1 for f in range(len(batches))]
    a = _run_sequence(W, H, batches, pubs, replay, False)
    b = _run_sequence(W, H, batches, pubs, replay, True)
    assert len(a) == len(b) and len(a[-1][0]) > 40
    for f, (ra, rb) in enumerate(zip(a, b)):
        for k, (va, vb) in enumerate(zip(ra, rb)):
            assert va.dtype == vb.dtype and va.shape == vb.shape, (f, k)
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), (f, k)
