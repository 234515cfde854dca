"""GPU: the event images that follow announced batches (include/esvio_fe.h "event images", mode 2).  The designed
sequence of tests/event_image_ahead_cases.py — every frame's images differ from those of the four frames on either side —
is announced 1, 2 and 3 batches ahead, from device and from pageable host memory, with lazy returns and the launch
thread on and off: after every track call both images and the canvas, fetched to host and to device memory, are that
frame's by the plain loop of tests/event_image_ref.py and by a mode-1 handle tracking the same batches with plain calls,
and the tracks are those of the same schedule with the setting off.  Then: fetching every third frame only, announced
motion-compensated batches in both forms of the update, esvio_fe_reset with batches announced, the refusals, and what
the mode allocates."""
import ctypes as C

import numpy as np
import pytest

import event_image_ahead_cases as A
import event_image_cases as K
import event_image_ref as R
from esvio_amd import frontend as FE

pytestmark = pytest.mark.gpu

W, H = A.W, A.H
KW = dict(max_cnt=40, min_dist=5, f_ransac=1)
A_MODE = FE.EVENT_IMAGES_AHEAD
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def tracker(mode, **kw):
    ft = FE.FeatureTracker(FE.make_config(W, H, device=0, **dict(KW, **kw)))
    if mode:
        ft.set_event_images(mode)
    return ft


def same(got, want, tag=""):
    assert got.shape == want.shape and got.dtype == np.uint8, tag
    assert np.array_equal(got, want), (tag, int((got != want).any(axis=-1).sum()))


class DeviceScratch:
    """memory of the library's runtime for the getters' device destinations, read back with its hipMemcpy"""

    def __init__(self):
        self.L, self.hip, self.p = FE.load_library(), C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.L.esvio_fe_mem_alloc(FE.DEVICE, W * H * 6, C.byref(self.p)) == 0

    def fetch(self, ft):
        out = []
        for cam, shape in ((0, (H, W, 3)), (1, (H, W, 3)), (None, (H, 2 * W, 3))):
            back = np.zeros(shape, np.uint8)
            if cam is None:
                ft._hd.check(self.L.esvio_fe_get_event_canvas(ft._hd.h, self.p, FE.DEVICE))
            else:
                ft._hd.check(self.L.esvio_fe_get_event_image(ft._hd.h, cam, self.p, FE.DEVICE))
            assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), self.p, C.c_size_t(back.nbytes), 2) == 0
            out.append(back)
        return out

    def free(self):
        self.L.esvio_fe_mem_free(FE.DEVICE, self.p)


@pytest.fixture(scope="module")
def scratch():
    s = DeviceScratch()
    yield s
    s.free()


@pytest.fixture(scope="module")
def mode1_images():
    """the images a mode-1 handle gives for the sequence tracked by plain calls: (left, right, canvas) per frame"""
    ft, out = tracker(1), []
    try:
        for (L, Rt, t), pub in zip(A.sequence(), A.PUB):
            ft.trackEvent(t, L, Rt, bool(pub))
            out.append((ft.event_image(0), ft.event_image(1), ft.event_canvas()))
    finally:
        ft.close()
    for k, (got, want) in enumerate(zip(out, A.reference())):
        for g, w in zip(got, want):
            same(g, w, ("mode 1", k))
    return out


class Placed:
    """a sequence's batches where a run wants them: pageable host arrays, or device memory of the library's runtime"""

    def __init__(self, seq, space):
        self.bufs, self.args = [], []
        for L, Rt, t in seq:
            if space == FE.DEVICE:
                bl = FE.EventBuffer(L, FE.DEVICE)
                self.bufs.append(bl)
                if len(Rt):
                    br = FE.EventBuffer(Rt, FE.DEVICE)
                    self.bufs.append(br)
                    self.args.append((bl.arg, br.arg, t))
                else:
                    self.args.append((bl.arg, (bl.arg[0], 0), t))  # nR = 0: any pointer
            else:
                self.args.append((np.array(L), np.array(Rt), t))

    def free(self):
        for b in self.bufs:
            b.free()


def replay(ft, placed, ahead, pub=A.PUB, after=None, mc=None, stop=None):
    """track the batches (the first `stop` of them), each announced `ahead` batches ahead of its call (the first one is
    a plain call); after(k): called when frame k's call has returned"""
    nxt = 1
    for k, (L, Rt, t) in enumerate(placed.args[:stop]):
        while ahead and nxt < len(placed.args) and nxt <= k + ahead:
            l2, r2, t2 = placed.args[nxt]
            ft.set_next_batch(t2, l2, r2, bool(pub[nxt]), measurements=mc)
            nxt += 1
        ft.trackEvent(t, L, Rt, bool(pub[k]), measurements=mc)
        if after:
            after(k)


def results(ft):
    return [np.array(getattr(ft, name)) for name in RESULTS]


@pytest.mark.parametrize("ahead", [1, 2, 3])
@pytest.mark.parametrize("space", [FE.DEVICE, FE.HOST], ids=["device", "pageable"])
def test_every_frames_images_are_its_own_and_the_tracks_are_the_settings_off(mode1_images, scratch, ahead, space):
    placed = Placed(A.sequence(), space)
    a, b = tracker(A_MODE), tracker(0)
    try:
        for lazy in (False, True):
            for thread in (False, True):
                tag = (ahead, space, lazy, thread)
                for ft in (a, b):
                    ft.reset()
                    ft.set_lazy_new_stereo(lazy)
                    ft.set_launch_thread(thread)
                tracks = []
                replay(b, placed, ahead, after=lambda k: tracks.append(results(b)))

                def check(k):
                    host = (a.event_image(0), a.event_image(1), a.event_canvas())
                    dev = scratch.fetch(a)
                    for part, name in enumerate(("left", "right", "canvas")):
                        same(host[part], A.reference()[k][part], tag + (k, name, "restatement"))
                        same(host[part], mode1_images[k][part], tag + (k, name, "mode 1"))
                        same(dev[part], host[part], tag + (k, name, "device"))
                    for name, x, y in zip(RESULTS, results(a), tracks[k]):
                        assert x.shape == y.shape and x.tobytes() == y.tobytes(), tag + (k, name)

                replay(a, placed, ahead, after=check)
                a.finish()
                b.finish()
                for name, x, y in zip(RESULTS, results(a), results(b)):
                    assert x.shape == y.shape and x.tobytes() == y.tobytes(), tag + ("finish", name)
                same(a.event_canvas(), A.reference()[-1][2], tag + ("after finish",))
    finally:
        a.close()
        b.close()
        placed.free()


def test_fetching_every_third_frame_only_nothing_of_the_frames_between_is_left():
    seq = A.sequence(n=2 * A.N_BATCHES)  # 18 frames over 4 sets: every set is reused several times, most of them unfetched
    placed = Placed(seq, FE.DEVICE)
    t = tracker(A_MODE)
    try:
        t.set_launch_thread(True)
        seen = []

        def check(k):
            if k % 3 == 2:
                L, Rt, _ = seq[k]
                wantL, wantR = R.event_image(L, W, H), R.event_image(Rt, W, H)
                same(t.event_image(1), wantR, (k, "right"))
                same(t.event_canvas(), R.canvas(wantL, wantR), (k, "canvas"))
                seen.append(k)

        replay(t, placed, 3, pub=A.PUB * 2, after=check)
        assert seen == [2, 5, 8, 11, 14, 17]
    finally:
        t.close()
        placed.free()


def test_plain_calls_and_stage_calls_in_mode_2_are_mode_1s(mode1_images):
    t, seq = tracker(A_MODE), A.sequence()
    try:
        for k, ((L, Rt, tt), pub) in enumerate(zip(seq, A.PUB)):
            t.trackEvent(tt, L, Rt, bool(pub))
            same(t.event_image(0), mode1_images[k][0], (k, "left"))
            same(t.event_canvas(), mode1_images[k][2], (k, "canvas"))
        # a stage call accumulates into the set the getters read; clear zeroes it
        L0 = seq[0][0]
        t.detector.createSAE_left(L0)
        same(t.event_image(0), R.event_image(L0, W, H, base=mode1_images[-1][0]), "accumulated")
        t.clear_event_images()
        assert not t.event_canvas().any()
    finally:
        t.close()


@pytest.mark.parametrize("sort_form", [False, True])
def test_announced_motion_compensated_batches_write_the_warped_pixels(oracle, monkeypatch, sort_form):
    if sort_form:
        monkeypatch.setenv("ESVIO_FE_SAE_SORT", "1")  # (read when the handle is created)
    L, Rt, t1, _, pxL, pxR = K.mc_case(oracle)
    m = FE.make_motion(t1, K.MC["v"], K.MC["v_pre"], K.MC["accel"], K.MC["omega"], K.MC["fx"], K.MC["fy"], K.MC["cx"], K.MC["cy"])
    # (an event's warped pixel depends on the event, t_0 and the motion alone: prefixes of the batch that keep the first
    # left event keep the oracle's pixels)  the whole batch is above one event per pixel, the prefixes below: both forms
    # of the mark kernel, each frame unlike the others
    cuts = ((len(L), len(Rt)), (1000, 700), (1500, 1500), (600, 1000))
    want = [(R.event_image(L[:a], W, H, pixels=pxL[:a]), R.event_image(Rt[:b], W, H, pixels=pxR[:b])) for a, b in cuts]
    assert not np.array_equal(want[0][0], R.event_image(L, W, H))  # the warp moves pixels
    for i in range(len(want)):
        for j in range(i + 1, len(want)):
            assert not np.array_equal(want[i][0], want[j][0]) and not np.array_equal(want[i][1], want[j][1])
    seq = [(L[:a], Rt[:b], t1 + 0.001 * k) for k, (a, b) in enumerate(cuts)]
    for space in (FE.HOST, FE.DEVICE):
        placed = Placed(seq, space)
        t = tracker(A_MODE)
        try:
            def check(k):
                same(t.event_image(0), want[k][0], (space, k, "left"))
                same(t.event_image(1), want[k][1], (space, k, "right"))
                same(t.event_canvas(), R.canvas(*want[k]), (space, k, "canvas"))

            replay(t, placed, 2, pub=(1, 0, 1, 1), after=check, mc=m)
        finally:
            t.close()
            placed.free()


def test_reset_with_batches_announced_then_a_fresh_sequence(mode1_images):
    placed, other = Placed(A.sequence(), FE.DEVICE), Placed(A.sequence(seed=1), FE.HOST)
    t = tracker(A_MODE)
    try:
        t.set_launch_thread(True)
        # frames 0..2 tracked; 3, 4 and 5 are announced, their updates under way or done
        replay(t, placed, 3, stop=3, after=lambda k: same(t.event_canvas(), mode1_images[k][2], (k, "before reset")))
        with pytest.raises(FE.FrontendError, match="announced"):
            t.set_event_images(A_MODE)
        t.reset()
        zero = np.zeros((H, W, 3), np.uint8)
        same(t.event_image(0), zero, "reset left")
        same(t.event_image(1), zero, "reset right")
        t.set_event_images(A_MODE)  # nothing is announced any more: accepted (and the setting had been kept)
        ref = A.reference(seed=1)
        replay(t, other, 3, after=lambda k: [same(t.event_image(c), ref[k][c], ("fresh", k, c)) for c in (0, 1)])
    finally:
        t.close()
        placed.free()
        other.free()


def test_refusals_and_what_the_mode_allocates():
    # (at 640 x 480: 19 MB for the mode, 6 MB for mode 1 — sizes the device's free-memory figure shows)
    t = FE.FeatureTracker(FE.make_config(640, 480, device=0, **KW))
    try:
        L_, h = t._hd.L, t._hd.h
        err = lambda: L_.esvio_fe_last_error(h).decode()
        for bad in (3, -1, 256):
            assert L_.esvio_fe_set_event_images(h, bad) == -1 and "ESVIO_FE_EVENT_IMAGES_AHEAD" in err(), bad
        with pytest.raises(FE.FrontendError, match="off"):
            t.event_image(0)  # a refused value turns nothing on
        (L, Rt, tt), (L1, Rt1, tt1), (L2, Rt2, tt2) = A.sequence()[:3]
        t.trackEvent(tt, L, Rt, True)
        t.set_next_batch(tt1, L1, Rt1, True)  # (with the setting off: what an announced batch itself allocates is there)
        t.trackEvent(tt1, L1, Rt1, True)
        free0 = t.device_memory()[0]
        t.set_event_images(A_MODE)
        free2 = t.device_memory()[0]
        assert free2 < free0
        # changing the setting — to any value — with a batch announced is refused, and changes nothing
        t.set_next_batch(tt2, L2, Rt2, True)
        for on in (0, 1, 2, 3):
            assert L_.esvio_fe_set_event_images(h, on) == -1 and ("announced" in err() or on == 3), on
        t.trackEvent(tt2, L2, Rt2, True)
        same(t.event_image(0), R.event_image(L2, 640, 480), "still on")
        assert t.device_memory()[0] == free2  # no later call allocates for it
        # mode 1 on the same handle: announcing is refused again, the extra sets are gone
        t.set_event_images(1)
        free1 = t.device_memory()[0]
        assert free2 < free1 < free0
        with pytest.raises(FE.FrontendError, match="set_event_images"):
            t.set_next_batch(tt2 + 0.02, L2, Rt2, True)
        t.set_event_images(0)
        assert t.device_memory()[0] == free0
    finally:
        t.close()
