"""GPU: esvio_fe_slice_events / _flush / _reset against the sequential reading of the rule, tests/slice_ref.py
(Slicer.push).  Integers and exact doubles only: every cut entry and every esvio_fe_slice_info field is compared for
equality.  T is the chain's tile in events (esvio_fe_slice_tile_events): the lengths and the crossings lie around its
edges."""
import ctypes as C

import numpy as np
import pytest

import slice_ref as S
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5A5A5A5A5
O1K = (10, 500)  # with 1000 Hz: E_k = 10 s + (k + 1) ms + 500 ns (worked by hand in tests/test_slice_ref.py)


def tile():
    return FE.load_library().esvio_fe_slice_tile_events()


def records(ns):
    """stamps in integer nanoseconds -> EVENT_DTYPE records (x, y count the events)"""
    ns = np.asarray(ns, np.int64)
    ev = np.zeros(len(ns), EVENT_DTYPE)
    ev["x"], ev["y"] = np.arange(len(ns)) & 0xffff, np.arange(len(ns)) >> 16
    ev["sec"], ev["nsec"], ev["polarity"] = ns // 10**9, ns % 10**9, np.arange(len(ns)) & 1
    return ev


class Sl:
    """a handle and the restatement's slicers of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.fresh()

    def fresh(self, how="slice_reset"):
        getattr(self.ft, how)()
        self.ref = [None, None]

    def close(self):
        self.ft.close()

    def call(self, cam, ev, frequency, origin=None, space=FE.HOST, cuts_cap=FE.SLICE_MAX_WINDOWS, extra=3):
        """one esvio_fe_slice_events call -> (rc, cuts array of cuts_cap + extra entries, SliceInfo); the restatement
        does not move"""
        ev = np.ascontiguousarray(ev)
        prm = FE.SliceParams(frequency, origin)
        info = FE.SliceInfo(first_sec=71, first_nsec=72, last_sec=73, last_nsec=74)
        cuts = np.full(cuts_cap + extra, GUARD, np.uint64)
        dsrc = None
        src = C.c_void_p(ev.ctypes.data if len(ev) else 0)
        if space == FE.DEVICE:
            dsrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, max(ev.nbytes, 16), C.byref(dsrc)) == 0
            if ev.nbytes:
                assert self.L.esvio_fe_mem_upload(dsrc, C.c_void_p(ev.ctypes.data), ev.nbytes) == 0
            src = dsrc
        rc = self.L.esvio_fe_slice_events(self.h, cam, src, len(ev), space, C.byref(prm), C.c_void_p(cuts.ctypes.data), cuts_cap,
                                          C.byref(info))
        if dsrc is not None:
            self.L.esvio_fe_mem_free(FE.DEVICE, dsrc)
        return rc, cuts, info

    def check(self, cam, ev, frequency, origin=None, space=FE.HOST, tag=None, exact_cap=False):
        """a call that succeeds equals the restatement, which advances with it -> (cuts, info of the restatement)"""
        if self.ref[cam] is None:
            self.ref[cam] = S.Slicer(frequency, origin)
        want, wi = self.ref[cam].push(ev["sec"], ev["nsec"])
        cap = len(want) if exact_cap else FE.SLICE_MAX_WINDOWS
        rc, cuts, info = self.call(cam, ev, frequency, origin, space, cap)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        assert cuts[:len(want)].tolist() == want, (tag, cuts[:len(want)].tolist(), want)
        assert (cuts[len(want):] == GUARD).all(), (tag, "entries behind the closed windows or behind cuts_cap touched")
        self.same_info(info, wi, tag)
        return want, wi

    @staticmethod
    def same_info(info, wi, tag=None):
        got = (info.closed, info.first_window, info.count, info.open_events)
        assert got == (wi["closed"], wi["first_window"], wi["count"], wi["open_events"]), (tag, got, wi)
        stamps = (info.first_sec, info.first_nsec, info.last_sec, info.last_nsec)
        assert stamps == (wi["first"] + wi["last"] if wi["closed"] else (71, 72, 73, 74)), (tag, stamps, wi)


@pytest.fixture(scope="module")
def sl():
    s = Sl()
    yield s
    s.close()


def crossing_stream(n, T):
    """1000 Hz from O1K: steps of 100 ns, and a whole millisecond more at the last event of tile 0, the first event of tile
    1, the middle of tile 0 and inside tile 3 — the ones that exist at this length"""
    ns = 10 * 10**9 + 500 + 100 * np.arange(n, dtype=np.int64)
    for at in (T // 2, T - 1, T, 3 * T + 2):
        if at < n:
            ns[at:] += 1000000
    return ns


@pytest.mark.parametrize("space", [FE.HOST, FE.DEVICE])
def test_lengths_around_the_tile_edges(sl, space):
    T = tile()
    assert T >= 64
    for n in (1, T - 1, T, T + 1, 3 * T + 5):
        sl.fresh()
        ev = records(crossing_stream(n, T))
        want, wi = sl.check(0, ev, 1000.0, space=space, tag=("n", n), exact_cap=n != T)
        assert want == [at for at in (T // 2, T - 1, T, 3 * T + 2) if at < n]
        assert wi["open_events"] == n - (want[-1] if want else 0)


def test_stamp_edges(sl):
    T = tile()
    cases = {
        "on a boundary": [500, 1000500],
        "1 ns below": [500, 1000499, 1000499],
        "equal stamps": [500, 500, 1000500, 1000500, 1000500, 2000500],
        "back-step across a boundary": [500, 1000600, 900000, 300, 2000500, 1999999],
        "three-window gap": [500, 3000600, 3000700, 3000800],
        "gaps and back-steps": [500, 7000500, 100, 7000499, 19000500, 19000499, 8000000, 20000500],
    }
    for tag, off in cases.items():
        for origin in (None, O1K):
            sl.fresh()
            sl.check(1, records(10 * 10**9 + np.asarray(off, np.int64)), 1000.0, origin=origin, tag=(tag, origin))
    sl.fresh()  # events before an explicit origin belong to window 0
    want, wi = sl.check(0, records(10 * 10**9 + np.asarray([100, 200, 1000499, 1000500], np.int64)), 1000.0, origin=O1K)
    assert want == [3]
    # 30 Hz over more than 100 windows and 1000 Hz over more than 2000, a quarter of the steps zero, a fifth of the events
    # stepping back; more than one tile
    rng = np.random.default_rng(11)
    for frequency, n in ((30.0, 2 * T + 77), (1000.0, 3 * T + 1)):
        period = 1e9 / frequency
        step = rng.integers(0, int((160 if frequency == 30.0 else 3000) * period / n * 2), n)
        step[rng.random(n) < 0.25] = 0
        ns = 1700000000 * 10**9 + 999000000 + np.cumsum(step)
        back = rng.random(n) < 0.2
        ns[back] -= rng.integers(0, int(2.5 * period), int(back.sum()))
        sl.fresh()
        want, wi = sl.check(0, records(ns), frequency, tag=frequency)
        assert wi["closed"] > (100 if frequency == 30.0 else 2000)
        assert frequency == 30.0 or len(set(want)) < len(want)  # at 1000 Hz some event closes several windows


def test_chunking_at_every_position_and_flush(sl):
    T = tile()
    rng = np.random.default_rng(3)
    step = rng.integers(0, 30000000, 40)
    step[25] = 200000000  # a gap of several windows
    ns = 1000 * 10**9 + np.cumsum(step)
    ns[[7, 19, 33]] -= 40000000
    ev = records(ns)
    whole, winfo = S.Slicer(30.0).push(ev["sec"], ev["nsec"])
    assert len(whole) > 8
    for cut in range(41):
        sl.fresh()
        a, _ = sl.check(0, ev[:cut], 30.0, tag=("cut", cut, 0))
        b, ib = sl.check(0, ev[cut:], 30.0, space=FE.DEVICE if cut & 1 else FE.HOST, tag=("cut", cut, 1))
        assert a + [c + cut for c in b] == whole
        assert (ib["count"], ib["open_events"]) == (winfo["count"], winfo["open_events"])
    info = sl.ft.slice_flush(0)
    wf = sl.ref[0].flush()
    assert (info.closed, info.first_window, info.count, info.open_events) == (1, winfo["count"], winfo["count"] + 1, 0)
    assert (info.first_sec, info.first_nsec) == wf["first"] == (info.last_sec, info.last_nsec)
    sl.check(0, ev[38:], 30.0, tag="behind a flush")  # (stamps below the flushed window's end: they stay in the new open window)
    ns3 = crossing_stream(3 * T, T)
    ev3 = records(ns3)
    whole, _ = S.Slicer(1000.0).push(ev3["sec"], ev3["nsec"])
    for cut in (T - 1, T, T + 1):
        sl.fresh()
        a, _ = sl.check(1, ev3[:cut], 1000.0, tag=("3T", cut, 0))
        b, _ = sl.check(1, ev3[cut:], 1000.0, tag=("3T", cut, 1))
        assert a + [c + cut for c in b] == whole
    # a camera that has seen nothing has nothing to flush
    sl.fresh()
    info = sl.ft.slice_flush(1)
    assert (info.closed, info.count) == (0, 0)


def test_failures_leave_the_state_as_it_was(sl):
    sl.fresh()
    far = 1000500 + 4096 * 1000000  # E_4096 from O1K: the last boundary of a first call's range
    first = records(10 * 10**9 + np.asarray([500, 700, 1000600], np.int64))
    sl.check(0, first, 1000.0)  # one window closed, one event in the open one
    bad = records(10 * 10**9 + np.asarray([1000700, far + 1000000], np.int64))  # at E_{1 + 4096}
    rc, cuts, info = sl.call(0, bad, 1000.0)
    assert rc == -1 and b"4096" in sl.L.esvio_fe_last_error(sl.h)
    assert (info.closed, info.first_window, info.count, info.open_events) == (0, 1, 1, 1)
    assert (cuts == GUARD).all()
    # the same events in two smaller calls
    sl.check(0, bad[:1], 1000.0)
    ok = records(10 * 10**9 + np.asarray([far + 1000000 - 1], np.int64))  # 1 ns below: exactly 4096 windows
    want, wi = sl.check(0, ok, 1000.0)
    assert wi["closed"] == 4096 and want == [0] * 4096
    sl.check(0, bad[1:], 1000.0)
    # too little room for the cuts: the number needed, and the state as it was
    before = sl.ref[0].m
    gap = records(14200000000 + np.asarray([0, 5000000], np.int64))  # ~100 windows behind the last event, then 5 more
    rc, cuts, info = sl.call(0, gap, 1000.0, cuts_cap=2)
    assert rc == -1 and info.closed > 2 and info.count == before and (cuts == GUARD).all()
    sl.check(0, gap, 1000.0)
    # other parameters on a running camera
    assert sl.call(0, gap, 30.0)[0] == -1 and sl.call(0, gap, 1000.0, origin=O1K)[0] == -1
    assert sl.call(0, gap, 1e7)[0] == -1 and sl.call(2, gap, 30.0)[0] == -1
    sl.check(0, gap[1:], 1000.0)
    # the first call of a camera fails: the origin it would have set is forgotten
    sl.fresh()
    rc, _, info = sl.call(1, records(np.asarray([10 * 10**9, 20 * 10**9], np.int64)), 1000.0)
    assert rc == -1 and info.count == 0
    sl.check(1, records(np.asarray([50 * 10**9 + 5, 50 * 10**9 + 2000005], np.int64)), 1000.0)
    assert sl.ref[1].origin == (50, 5)


@pytest.mark.parametrize("how", ["slice_reset", "reset"])
def test_resets_give_a_fresh_state(sl, how):
    sl.fresh()
    ev = records(10 * 10**9 + np.asarray([500, 1000600, 2000700], np.int64))
    sl.check(0, ev, 1000.0)
    sl.check(1, ev, 1000.0, origin=O1K)
    sl.fresh(how)
    want, wi = sl.check(0, ev[1:], 30.0)  # other parameters, a new origin
    assert wi["first_window"] == 0 and sl.ref[0].origin == (10, 1000600)
    want, wi = sl.check(1, ev, 1000.0)
    assert wi["first_window"] == 0 and want == [1, 2]


# ---- the feed: chunks of a stereo stream in, esvio_fe_track_event on time-aligned windows out -----------------------------
import ba_filter2_ref as BF  # noqa: E402
import evt_ref as R  # noqa: E402
from esvio_amd.events import EventFields, event_times, make_events  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

W, H = 64, 48
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
PRM = FE.FilterParams(5_000_000, 1, 200_000)
# chunk sizes in events / words: 1 event (2 bytes of EVT3), sizes that fill the first 4096-record buffer in the middle of a
# window (the tail moves), one that does not fit any buffer so far (it grows), then irregular ones
SIZES = (1, 7, 3001, 2, 2500, 9000, 333, 1, 4096, 5000, 17, 6500)


@pytest.fixture(scope="module")
def scene():
    """about 9 windows of a seeded SceneStream for both cameras, in a sensor's read-out order: per camera x, y, p, t_us,
    the records, the words of both formats (stamps relative to `base`), and the filter's verdict on the whole stream"""
    st = SceneStream(W=W, H=H, rate=2e5, seed=7, n_rect=8, size=(12.0, 30.0), speed=(40.0, 110.0), disparity=4)
    base = st.t_us - 1000
    parts = [[], []]
    for _ in range(9):
        left, right, _ = st.next_batch()
        for cam, ev in enumerate((left, right)):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10**6 + ev["nsec"].astype(np.int64) // 1000
            o = R.readout_order(x, y, p, t)
            parts[cam].append((x[o], y[o], p[o], t[o]))
    cams = []
    for cam in range(2):
        x, y, p, t = (np.concatenate([q[k] for q in parts[cam]]) for k in range(4))
        rec = make_events(x, y, t, p)
        words = {f: np.concatenate([R.encode(f, *q[:3], q[3] - base) for q in parts[cam]]) for f in (R.EVT3, R.EVT2)}
        keep = BF.filter_events(BF.fresh_plane(W, H), W, H, rec, PRM.window_ns, PRM.min_support, PRM.refractory_ns)[0].astype(bool)
        cams.append(dict(x=x.astype(np.uint16), y=y.astype(np.uint16), p=p.astype(np.int8), t=t, rec=rec, words=words, keep=keep))
    assert 20000 < len(cams[0]["rec"]) < 200000
    return base, cams


def windows_of(left, right, frequency=30.0):
    """both cameras' records cut by slice_windows() with the first left record as the shared origin ->
    [(E_k, left records, right records)] for every window closed in both"""
    cl, wl, El, _ = S.slice_windows(left["sec"], left["nsec"], frequency)
    cr, wr, Er, _ = S.slice_windows(right["sec"], right["nsec"], frequency, origin=(int(left["sec"][0]), int(left["nsec"][0])))
    k = min(len(wl), len(wr))
    assert El[:k] == Er[:k]
    return [(El[j], left[wl[j][0]:wl[j][-1] + 1] if wl[j] else left[:0], right[wr[j][0]:wr[j][-1] + 1] if wr[j] else right[:0])
            for j in range(k)]


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def chunks(n, sizes=SIZES):
    a, k = 0, 0
    while a < n:
        b = min(n, a + sizes[k % len(sizes)])
        yield a, b
        a, k = b, k + 1


def run_feed(scene, kind, filtered=False, motion=False, hole=False, device=False):
    base, cams = scene
    recs = [cams[0]["rec"], cams[1]["rec"]]
    drop = np.zeros(len(recs[0]), bool)
    if hole:  # the left camera is silent for the whole of window 3 (and a little more)
        t = event_times(recs[0])
        drop = (t >= t[0] + 2.9 / 30) & (t < t[0] + 4.2 / 30)
        assert kind == "records" and drop.any()
    want_rec = [recs[0][cams[0]["keep"]] if filtered else recs[0][~drop], recs[1][cams[1]["keep"]] if filtered else recs[1]]
    want = windows_of(*want_rec)
    assert len(want) >= 7
    a, b = (FE.FeatureTracker(FE.make_config(W, H, max_cnt=40)) for _ in range(2))
    bufs = []
    try:
        a.feed_open(30.0, params=PRM if filtered else None)
        with pytest.raises(FE.FrontendError, match="left"):  # the origin is the first left record
            a.feed_push_events(1, recs[1][:5])
        if kind in ("evt3", "evt2"):
            fmt = R.EVT3 if kind == "evt3" else R.EVT2
            src = [cams[0]["words"][fmt], cams[1]["words"][fmt]]
        else:
            src = [recs[0][~drop], recs[1]]
            idx = [np.flatnonzero(~drop), np.arange(len(recs[1]))]
        its = [chunks(len(src[0])), chunks(len(src[1]))]
        done, tracked, appended = [False, False], 0, [0, 0]
        while not all(done):
            for cam in range(2):
                if cam == 1 and appended[0] == 0 and not done[0]:
                    continue  # (behind a filter the first left chunks may append nothing: the origin is not known yet)
                ab = next(its[cam], None)
                if ab is None:
                    done[cam] = True
                    continue
                lo, hi = ab
                if kind in ("evt3", "evt2"):
                    info = a.feed_push_raw(cam, fmt, src[cam][lo:hi], base)
                elif kind == "fields":
                    c, i = cams[cam], idx[cam][lo:hi]
                    info = a.feed_push_fields(cam, EventFields.from_arrays(c["x"][i], c["y"][i], c["t"][i], c["p"][i]))
                elif device:
                    bufs.append(FE.EventBuffer(src[cam][lo:hi], FE.DEVICE))
                    info = a.feed_push_events(cam, bufs[-1].arg)
                else:
                    info = a.feed_push_events(cam, src[cam][lo:hi])
                appended[cam] += info.appended
                while True:
                    w = a.feed_peek()
                    if w is None:
                        break
                    E, L, Rr = want[tracked]
                    assert (w.index, (w.end_sec, w.end_nsec), w.count[0], w.count[1]) == (tracked, E, len(L), len(Rr)), (kind, tracked)
                    pub = tracked % 3 != 1
                    m = None
                    if motion and len(L):
                        t1 = float(event_times(L[-1:])[0])
                        m = FE.make_motion(t1, (0.4, -0.2, 0.1), (0.1, 0.0, 0.0), (6.0, 2.0, -1.0), (0.3, -0.5, 0.2), 0.9 * W, 0.9 * W, W / 2.0, H / 2.0)
                    before = results(a) if len(L) == 0 else None
                    info = a.feed_track(pub, measurements=m)
                    assert (info.kept[0], info.kept[1]) == (len(L), len(Rr))
                    if len(L) == 0:
                        assert info.tracked == 0 and results(a) == before, "an empty left window is consumed and not tracked"
                    else:
                        cur = float(event_times(L[-1:])[0])
                        assert info.tracked == 1 and info.cur_time == cur
                        b.trackEvent(cur, L, Rr, pub, measurements=m)
                        assert results(a) == results(b), (kind, filtered, motion, tracked)
                    tracked += 1
        assert tracked == len(want) and appended == [len(want_rec[0]), len(want_rec[1])]
        if hole:
            assert any(len(L) == 0 for _, L, _ in want)
        return len(a.ids), len(a.ids_right)
    finally:
        for e in bufs:
            e.free()
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["records", "fields", "evt3", "evt2"])
def test_feed_equals_tracking_the_windows_slice_windows_cuts(scene, kind):
    n_left, n_right = run_feed(scene, kind)
    assert n_left > 0


@pytest.mark.parametrize("kind", ["records", "records-device", "fields", "evt3", "evt2"])
def test_feed_with_a_filter(scene, kind):
    run_feed(scene, kind.split("-")[0], filtered=True, device=kind.endswith("device"))


@pytest.mark.parametrize("kind", ["records-device", "fields", "evt2"])
def test_feed_with_motion(scene, kind):
    run_feed(scene, kind.split("-")[0], motion=True, device=kind.endswith("device"))


def test_feed_with_a_filter_and_motion_from_evt3_words(scene):
    run_feed(scene, "evt3", filtered=True, motion=True)


def test_feed_closed_and_reopened_right_behind_a_track_call(scene):
    """close + open rewinds the append position to the front of the buffers the last track call may still be reading: the
    first push behind it must not disturb that call (include/esvio_fe.h: buffer lifetime).  The stream's first part is
    fed until window 3 has been tracked; then, at once, the feed is closed, opened again and given the rest of the stream
    as a new one.  Every tracked window equals the second handle's."""
    base, cams = scene
    L, Rr = cams[0]["rec"], cams[1]["rec"]
    tl, tr = event_times(L), event_times(Rr)
    t_cut = tl[0] + 4.6 / 30

    def feed(a, b, left, right, stop_after=None):
        want = windows_of(left, right)
        its, src, tracked, done = [chunks(len(left)), chunks(len(right))], [left, right], 0, [False, False]
        while not all(done):
            for cam in range(2):
                ab = next(its[cam], None)
                if ab is None:
                    done[cam] = True
                    continue
                a.feed_push_events(cam, src[cam][ab[0]:ab[1]])
                while a.feed_peek() is not None:
                    E, wl, wr = want[tracked]
                    w = a.feed_peek()
                    assert (w.index, (w.end_sec, w.end_nsec), w.count[0], w.count[1]) == (tracked, E, len(wl), len(wr))
                    cur = float(event_times(wl[-1:])[0])
                    assert a.feed_track(tracked % 2 == 0).cur_time == cur
                    tracked += 1
                    if tracked == stop_after:
                        return tracked, (cur, wl, wr, tracked % 2 == 1)
                    b.trackEvent(cur, wl, wr, tracked % 2 == 1)
                    assert results(a) == results(b), tracked
        return tracked, None

    a, b = (FE.FeatureTracker(FE.make_config(W, H, max_cnt=40)) for _ in range(2))
    try:
        a.feed_open(30.0)
        n, last = feed(a, b, L, Rr, stop_after=4)
        assert n == 4
        a.feed_close()  # right behind the track call of window 3
        a.feed_open(30.0)
        info = a.feed_push_events(0, L[tl >= t_cut][:3000])  # lands at the front of the left buffer
        assert info.appended == 3000
        b.trackEvent(*last)
        assert results(a) == results(b), "the window tracked in front of the close"
        a.feed_close()
        a.feed_open(30.0)
        n, _ = feed(a, b, L[tl >= t_cut], Rr[tr >= t_cut])
        assert n >= 3 and len(a.ids) > 0
        with pytest.raises(FE.FrontendError, match="feed is open"):  # an open feed owns the slicer
            a.slice_reset()
        with pytest.raises(FE.FrontendError, match="feed is open"):
            a.slice_events(0, L[:10], 30.0)
        with pytest.raises(FE.FrontendError, match="feed is open"):
            a.slice_flush(0)
        a.feed_close()
        a.slice_reset()
    finally:
        a.close()
        b.close()


def test_feed_with_a_silent_left_window(scene):
    run_feed(scene, "records", hole=True)


def test_feed_with_an_explicit_origin_a_reset_and_the_refusals(scene):
    base, cams = scene
    L, Rr = cams[0]["rec"], cams[1]["rec"]
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    try:
        with pytest.raises(FE.FrontendError, match="no feed"):
            ft.feed_push_events(0, L[:10])
        o = (int(L["sec"][0]), int(L["nsec"][0]))
        ft.feed_open(30.0, origin=o)
        with pytest.raises(FE.FrontendError, match="open"):
            ft.feed_open(30.0)
        ref = [S.Slicer(30.0, o), S.Slicer(30.0, o)]
        n = len(L) // 3
        info = ft.feed_push_events(1, Rr[:n])  # with an explicit origin the right camera may come first
        cuts, wi = ref[1].push(Rr["sec"][:n], Rr["nsec"][:n])
        assert (info.appended, info.closed, info.queued) == (n, len(cuts), len(cuts)) and ft.feed_peek() is None
        info = ft.feed_push_events(0, L[:n])
        cuts, wi = ref[0].push(L["sec"][:n], L["nsec"][:n])
        w = ft.feed_peek()
        assert info.closed == len(cuts) > 1 and (w.index, (w.end_sec, w.end_nsec)) == (0, ref[0].boundary(0))
        assert ft.feed_track(True).tracked == 1 and ft.feed_peek().index == 1
        ft.reset()  # empties the feed, which stays open with its origin
        assert ft.feed_peek() is None
        info = ft.feed_push_events(1, Rr[:n])
        assert info.closed == info.queued > 1
        ft.feed_close()
        with pytest.raises(FE.FrontendError, match="no feed"):
            ft.feed_peek()
        # refused while batches are announced
        dl, dr = FE.EventBuffer(L[:n], FE.DEVICE), FE.EventBuffer(Rr[:n], FE.DEVICE)
        t = float(event_times(L[n - 1:n])[0])
        ft.set_next_batch(t, dl.arg, dr.arg, True)
        with pytest.raises(FE.FrontendError, match="announced"):
            ft.feed_open(30.0)
        ft.trackEvent(t, dl.arg, dr.arg, True)
        dl.free()
        dr.free()
    finally:
        ft.close()
