"""GPU: the event images (include/esvio_fe.h "event images") against the plain loop of tests/event_image_ref.py, byte for
byte: stage calls accumulate, track calls rewrite, the last event of a pixel wins whatever the stamps say, the packed
emit's tail, events the update skips, both cameras and the canvas, the motion-compensated pixels (read off the oracle's
planes, tests/event_image_cases.py) in both forms of the SAE update, filtered and lazily returned calls, reset, every
refusal, and a handle with the setting off: nothing allocated, nothing launched, the same results."""
import ctypes as C

import numpy as np
import pytest

import ba_filter_ref as BA
import event_image_cases as K
import event_image_ref as R
from conftest import scene_batches
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times

pytestmark = pytest.mark.gpu

W, H = K.W, K.H
KW = dict(max_cnt=40, min_dist=5, f_ransac=1)
NONE = np.zeros(0, EVENT_DTYPE)


def tracker(w=W, h=H, on=True, **kw):
    ft = FE.FeatureTracker(FE.make_config(w, h, device=0, **dict(KW, **kw)))
    if on:
        ft.set_event_images(True)
    return ft


def images(ft):
    return ft.event_image(0), ft.event_image(1)


def same(got, want, tag=""):
    assert got.shape == want.shape and got.dtype == np.uint8, tag
    assert np.array_equal(got, want), (tag, int((got != want).any(axis=-1).sum()))


def evimg_launches(ft):
    out = []
    for which in (0, 1):
        n = C.c_uint64(0)
        ft._hd.check(ft._hd.L.esvio_fe_event_image_kernel_stats(ft._hd.h, which, None, C.byref(n), None))
        out.append(n.value)
    return out


@pytest.fixture(scope="module")
def ft():
    t = tracker()
    yield t
    t.close()


def test_stage_calls_accumulate_and_clear_gives_zeros(ft):
    zero = np.zeros((H, W, 3), np.uint8)
    ft.clear_event_images()
    same(ft.event_image(0), zero, "before any event")
    same(ft.event_canvas(), R.canvas(zero, zero))
    for name, (L, Rt) in K.counts().items():
        ft.clear_event_images()
        L2, R2 = K.uniform(len(L), 300 + len(L)), K.uniform(len(Rt), 400 + len(Rt))
        for cam, (a, b) in enumerate(((L, L2), (Rt, R2))):  # two esvio_fe_create_sae calls per camera
            ft.detector._create_sae(cam, a)
            same(ft.event_image(cam), R.event_image(a, W, H), (name, cam, "first"))
            ft.detector._create_sae(cam, b)
            same(ft.event_image(cam), R.event_image(b, W, H, base=R.event_image(a, W, H)), (name, cam, "second"))
        # ... and the stereo stage call on top of both
        wantL = R.event_image(Rt, W, H, base=R.event_image(L2, W, H, base=R.event_image(L, W, H)))
        wantR = R.event_image(L, W, H, base=R.event_image(R2, W, H, base=R.event_image(Rt, W, H)))
        ft.detector.createSAE_stereo(Rt, L)
        same(ft.event_image(0), wantL, (name, "stereo left"))
        same(ft.detector.cur_event_mat_right, wantR, (name, "stereo right"))
        ft.clear_event_images()
        same(ft.event_image(0), zero, (name, "cleared"))
        same(ft.event_image(1), zero, (name, "cleared"))


def test_both_sides_of_the_mark_kernels_density_threshold(ft):
    for nl, nr in K.THRESHOLD:
        L, Rt = K.uniform(nl, 500 + nl), K.uniform(nr, 600 + nr)
        ft.clear_event_images()
        if nr:
            ft.detector.createSAE_stereo(L, Rt)
        else:
            ft.detector.createSAE_left(L)
        same(ft.event_image(0), R.event_image(L, W, H), (nl, nr, "left"))
        same(ft.event_image(1), R.event_image(Rt, W, H), (nl, nr, "right"))
        ft.trackEvent(event_times(L)[-1], L, Rt, False)
        same(ft.event_canvas(), R.canvas(R.event_image(L, W, H), R.event_image(Rt, W, H)), (nl, nr, "track"))


@pytest.mark.parametrize("last_on", [True, False])
def test_contention_the_last_event_of_a_pixel_wins(ft, last_on):
    ev = K.contention(last_on)
    ft.clear_event_images()
    ft.detector.createSAE_left(ev)
    got = ft.event_image(0)
    same(got, R.event_image(ev, W, H))
    assert tuple(got[K.HOT[1], K.HOT[0]]) == (R.ON if last_on else R.OFF)
    ft.trackEvent(event_times(ev)[-1], ev, ev[:-1], True)  # a track call: the right camera ends on the other polarity
    same(ft.event_image(0), R.event_image(ev, W, H))
    same(ft.event_image(1), R.event_image(ev[:-1], W, H))


def test_stamps_play_no_part_stream_order_does(ft):
    st = K.stamps()
    want = R.event_image(st["equal"], W, H)
    for name, ev in st.items():
        ft.clear_event_images()
        ft.detector.createSAE_right(ev)
        same(ft.event_image(1), want, name)
        same(ft.event_image(0), np.zeros_like(want), name)


@pytest.mark.parametrize("size", [(W, H), K.SMALL])
def test_corner_pixels_and_the_tail_of_the_packed_emit(size):
    w, h = size
    t = tracker(w, h)
    try:
        c, lp = K.corners(w, h), K.last_pixel(w, h)
        t.detector.createSAE_left(c)
        same(t.event_image(0), R.event_image(c, w, h), "corners")
        t.detector.createSAE_right(lp)
        got = t.event_image(1)
        same(got, R.event_image(lp, w, h), "last pixel alone")
        assert tuple(got[h - 1, w - 1]) == R.OFF and np.count_nonzero(got) == 1
        same(t.event_canvas(), R.canvas(R.event_image(c, w, h), R.event_image(lp, w, h)))
        # a track call over the same pixels: every other pixel is written zero, the tail group included
        both = np.zeros(len(c) + 1, EVENT_DTYPE)
        both[:len(c)], both[len(c):] = c, lp
        both["sec"], both["nsec"] = c["sec"][0], np.arange(len(both)) * 1000
        t.trackEvent(event_times(both)[-1], both, lp, False)
        same(t.event_image(0), R.event_image(both, w, h), "track")
        same(t.event_image(1), R.event_image(lp, w, h), "track right")
    finally:
        t.close()


def test_out_of_sensor_events_write_nothing(ft):
    o = K.out_of_sensor()
    ft.clear_event_images()
    assert ft.detector.createSAE_left(o) == 6
    same(ft.event_image(0), R.event_image(o, W, H))
    only_out = o[(o["x"] >= W) | (o["y"] >= H)]
    ft.detector.createSAE_right(only_out)
    same(ft.event_image(1), np.zeros((H, W, 3), np.uint8))


def test_stereo_left_and_right_differ_and_the_canvas_is_hconcat_on_host_and_device(ft):
    L, Rt = K.uniform(5000, 41), K.uniform(257, 42)
    ft.trackEvent(event_times(L)[-1], L, Rt, True)
    wantL, wantR = R.event_image(L, W, H), R.event_image(Rt, W, H)
    assert not np.array_equal(wantL, wantR)
    same(ft.event_image(0), wantL)
    same(ft.event_image(1), wantR)
    same(ft.event_canvas(), R.canvas(wantL, wantR))
    # device dst: the canvas and one image into memory of the library's runtime, read back with its hipMemcpy
    L_, hip = ft._hd.L, C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert L_.esvio_fe_mem_alloc(FE.DEVICE, W * H * 6, C.byref(p)) == 0
    try:
        back = np.zeros((H, 2 * W, 3), np.uint8)
        ft._hd.check(L_.esvio_fe_get_event_canvas(ft._hd.h, p, FE.DEVICE))
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), p, C.c_size_t(back.nbytes), 2) == 0
        same(back, R.canvas(wantL, wantR), "device canvas")
        one = np.zeros((H, W, 3), np.uint8)
        ft._hd.check(L_.esvio_fe_get_event_image(ft._hd.h, 1, p, FE.DEVICE))
        assert hip.hipMemcpy(C.c_void_p(one.ctypes.data), p, C.c_size_t(one.nbytes), 2) == 0
        same(one, wantR, "device image")
    finally:
        L_.esvio_fe_mem_free(FE.DEVICE, p)
    # nR = 0: the right camera's update is skipped, its image is zero
    ft.trackEvent(event_times(L)[-1] + 0.01, L, NONE, False)
    same(ft.event_image(0), wantL)
    same(ft.event_image(1), np.zeros_like(wantR), "nR = 0")


RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def test_track_calls_rewrite_both_images_and_change_no_result():
    w, h = 346, 260
    batches = scene_batches(w, h, 3, 3e5, 5, n_rect=12, size=(30.0, 90.0))
    a, b = tracker(w, h, max_cnt=150, min_dist=10), tracker(w, h, on=False, max_cnt=150, min_dist=10)
    try:
        a.set_profiling(True)
        refs, bufs = [], []
        for k, (L, Rt, _) in enumerate(batches):
            t = event_times(L)[-1]
            # (a's batch lies in device memory: the call is split by camera, the right camera's update and its image
            # run on the stereo stream; b's in host memory)
            bufs += [FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(Rt, FE.DEVICE)]
            a.trackEvent(t, bufs[-2].arg, bufs[-1].arg, True)
            b.trackEvent(t, L, Rt, True)
            wantL, wantR = R.event_image(L, w, h), R.event_image(Rt, w, h)
            refs.append(wantL)
            same(a.event_image(0), wantL, (k, "left"))
            same(a.event_image(1), wantR, (k, "right"))
            same(a.event_canvas(), R.canvas(wantL, wantR), (k, "canvas"))
            for name in RESULTS:
                x, y = getattr(a, name), getattr(b, name)
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), (k, name)
        assert len(a.ids) > 20
        gone = refs[0].any(axis=2) & ~refs[1].any(axis=2)  # hit in batch 1 only: zero after batch 2
        assert gone.sum() > 100
        # per call split by camera two marks and two emits (left: main stream, right: stereo stream), else one of each
        split = a.plain_call_counters()["split_by_camera"]
        assert split > 0 and evimg_launches(a) == [3 + split, 3 + split]
    finally:
        a.close()
        b.close()
        for e in bufs:
            e.free()


@pytest.mark.parametrize("sort_form", [False, True])
def test_motion_compensated_calls_write_the_warped_pixels(oracle, monkeypatch, sort_form):
    if sort_form:
        monkeypatch.setenv("ESVIO_FE_SAE_SORT", "1")  # (read when the handle is created)
    L, Rt, t1, _, pxL, pxR = K.mc_case(oracle)
    m = FE.make_motion(t1, K.MC["v"], K.MC["v_pre"], K.MC["accel"], K.MC["omega"], K.MC["fx"], K.MC["fy"], K.MC["cx"], K.MC["cy"])
    wantL, wantR = R.event_image(L, W, H, pixels=pxL), R.event_image(Rt, W, H, pixels=pxR)
    t = tracker()
    try:
        t.trackEvent(event_times(L)[-1], L, Rt, True, measurements=m)
        same(t.event_image(0), wantL, "track_event_mc left")
        same(t.event_image(1), wantR, "track_event_mc right")
        # the first thousand of each camera: below one event per pixel, the mark kernel's other form (an event's warped
        # pixel depends on the event, t_0 and the motion alone: the oracle's pixels of the whole batch hold)
        t.trackEvent(event_times(L)[-1] + 0.001, L[:1000], Rt[:1000], False, measurements=m)
        same(t.event_image(0), R.event_image(L[:1000], W, H, pixels=pxL[:1000]), "sparse left")
        same(t.event_image(1), R.event_image(Rt[:1000], W, H, pixels=pxR[:1000]), "sparse right")
        t.trackEvent(event_times(L)[-1] + 0.002, L, Rt, False, measurements=m)
        # the stage call accumulates at the warped pixels too: the cameras' batches swapped, on top
        pxRl = K.oracle_pixels(oracle, Rt, Rt[:1], oracle.make_motion(t1, **K.MC), 0)  # (t_0 is the first LEFT event's: Rt's own here)
        pxLr = K.oracle_pixels(oracle, L, Rt[:1], oracle.make_motion(t1, **K.MC), 1)
        t.detector.createSAE_stereo_mc(Rt, L, m)
        same(t.event_image(0), R.event_image(Rt, W, H, base=wantL, pixels=pxRl), "create_sae_stereo_mc left")
        same(t.event_image(1), R.event_image(L, W, H, base=wantR, pixels=pxLr), "create_sae_stereo_mc right")
        # one plain batch in this form of the update
        ev = K.uniform(5000, 77)
        t.trackEvent(event_times(ev)[-1] + 1.0, ev, ev[:257], False)
        same(t.event_image(0), R.event_image(ev, W, H), "plain")
        same(t.event_image(1), R.event_image(ev[:257], W, H), "plain right")
    finally:
        t.close()


def test_the_node_shows_event_loop_for_the_motion_compensated_overload_only():
    from esvio_amd.node import MotionCorrection, StereoEventTrackerNode
    L, Rt = K.uniform(3000, 61), K.uniform(3000, 62)
    for mc in (False, True):
        t = tracker(on=False)
        try:
            motion = MotionCorrection(K.MC["fx"], K.MC["fy"], K.MC["cx"], K.MC["cy"]) if mc else None
            node = StereoEventTrackerNode(t, 15, motion=motion, make_motion=FE.make_motion, show_track=True)  # turns the setting on
            assert node.handle(L, Rt, 5.01) is None  # the first frame is not tracked
            out = node.handle(L, Rt, 5.02)
            assert set(out) == {"points", "feature_img_base", "time_surface"} | ({"event_loop"} if mc else set())
            wantL, wantR = R.event_image(L, W, H), R.event_image(Rt, W, H)  # (no IMU message: the batch is not warped)
            same(out["feature_img_base"], R.canvas(wantL, wantR), mc)
            assert np.array_equal(out["time_surface"], t.gettimesurface(0))
            if mc:
                same(out["event_loop"], wantL, "event_loop")
        finally:
            t.close()


def test_filtered_calls_give_the_image_of_the_kept_records():
    L, Rt = K.uniform(3000, 51, region=(5, 5, 30, 30)), K.uniform(2000, 52, region=(8, 8, 40, 40))
    prm = FE.FilterParams(window_ns=1_000_000, min_support=1)
    keep = []
    for ev in (L, Rt):
        flags, _ = BA.filter_events(BA.fresh_plane(W, H), W, H, ev, prm.window_ns, prm.min_support)
        assert 0 < flags.sum() < len(ev)
        keep.append(ev[flags != 0])
    t = tracker()
    try:
        info = t.track_batch(L, Rt, params=prm)
        assert list(info.kept) == [len(keep[0]), len(keep[1])] and info.tracked
        same(t.event_image(0), R.event_image(keep[0], W, H), "kept left")
        same(t.event_image(1), R.event_image(keep[1], W, H), "kept right")
        assert not np.array_equal(R.event_image(keep[0], W, H), R.event_image(L, W, H))
    finally:
        t.close()


def test_lazy_returns_and_reset():
    w, h = 346, 260
    batches = scene_batches(w, h, 3, 3e5, 9, n_rect=12, size=(30.0, 90.0))
    t = tracker(w, h, max_cnt=150, min_dist=10)
    try:
        t.set_lazy_new_stereo(True)
        for k, (L, Rt, _) in enumerate(batches):
            t.trackEvent(event_times(L)[-1], L, Rt, k != 1)  # the second frame publishes nothing: it returns before its stereo LK
            same(t.event_image(0), R.event_image(L, w, h), (k, "lazy left"))
            same(t.event_canvas(), R.canvas(R.event_image(L, w, h), R.event_image(Rt, w, h)), (k, "lazy canvas"))
        t.finish()
        t.reset()
        zero = np.zeros((h, w, 3), np.uint8)
        same(t.event_image(0), zero, "reset")
        same(t.event_image(1), zero, "reset")
        t.clear_event_images()  # the setting is still on
        L, Rt, _ = batches[0]
        t.trackEvent(event_times(L)[-1], L, Rt, True)
        same(t.event_image(1), R.event_image(Rt, w, h), "after reset")
    finally:
        t.close()


def test_every_refusal_names_itself():
    t = tracker(on=False)
    try:
        L_, h = t._hd.L, t._hd.h
        buf = np.zeros((H, 2 * W, 3), np.uint8)
        err = lambda: L_.esvio_fe_last_error(h).decode()
        # the setting is off
        for call in (lambda: L_.esvio_fe_get_event_image(h, 0, FE._p(buf), FE.HOST), lambda: L_.esvio_fe_get_event_canvas(h, FE._p(buf), FE.HOST),
                     lambda: L_.esvio_fe_clear_event_images(h)):
            assert call() == -1 and "off" in err()
        t.set_event_images(True)
        for cam in (-1, 2):
            assert L_.esvio_fe_get_event_image(h, cam, FE._p(buf), FE.HOST) == -1 and "cam" in err()
        assert L_.esvio_fe_get_event_image(h, 0, None, FE.HOST) == -1 and "null" in err()
        assert L_.esvio_fe_get_event_canvas(h, None, FE.DEVICE) == -1 and "null" in err()
        for space in (-1, 2):
            assert L_.esvio_fe_get_event_image(h, 0, FE._p(buf), space) == -1 and "space" in err()
            assert L_.esvio_fe_get_event_canvas(h, FE._p(buf), space) == -1 and "space" in err()
        assert not buf.any()
        # announced batches: refused while the setting is on, and the setting is refused while batches are announced
        ev = K.uniform(300, 3)
        with pytest.raises(FE.FrontendError, match="set_event_images"):
            t.set_next_batch(event_times(ev)[-1], ev, ev, True)
        m = FE.make_motion(6.0, **K.MC)
        with pytest.raises(FE.FrontendError, match="set_event_images"):
            t.set_next_batch(event_times(ev)[-1], ev, ev, True, measurements=m)
        t.set_event_images(False)
        t.set_next_batch(event_times(ev)[-1], ev, ev, True)
        with pytest.raises(FE.FrontendError, match="announced"):
            t.set_event_images(True)
        t.trackEvent(event_times(ev)[-1], ev, ev, True)  # the announced batch is tracked: the setting can be turned on again
        t.set_event_images(True)
        same(t.event_image(0), np.zeros((H, W, 3), np.uint8), "set leaves both images zero")
    finally:
        t.close()


def test_with_the_setting_off_nothing_is_allocated_and_nothing_is_launched():
    w, h = 640, 480
    t = tracker(w, h, on=False, max_cnt=150, min_dist=10)
    try:
        t.set_profiling(True)
        L, Rt, _ = scene_batches(w, h, 1, 3e5, 13)[0]
        t.detector.createSAE_stereo(L, Rt)
        t.trackEvent(event_times(L)[-1] - 0.02, L, Rt, True)
        t.trackEvent(event_times(L)[-1] - 0.01, L, Rt, True)
        t.trackEvent(event_times(L)[-1], L, Rt, True)
        assert evimg_launches(t) == [0, 0]
        names = t.kernel_stats(stages=True)
        assert not [n for n in names if "evimg" in n]
        free0 = t.device_memory()[0]
        t.set_event_images(True)
        free1 = t.device_memory()[0]
        assert free1 < free0  # 20 bytes per pixel: 6 MB here
        t.trackEvent(event_times(L)[-1] + 0.01, L, Rt, True)
        assert t.device_memory()[0] == free1  # no later call allocates for it
        on = evimg_launches(t)
        assert on[0] == on[1] and on[0] in (1, 2)
        t.set_event_images(False)
        assert t.device_memory()[0] == free0
        t.trackEvent(event_times(L)[-1] + 0.02, L, Rt, True)
        assert evimg_launches(t) == on and t.device_memory()[0] == free0
    finally:
        t.close()
