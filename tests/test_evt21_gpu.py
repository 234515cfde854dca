"""GPU: EVT2.1 (ESVIO_FE_RAW_EVT21) through esvio_fe_decode_raw, esvio_fe_track_raw and the feed, against the sequential
restatement tests/evt21_ref.py.  Integers only: all 16 bytes of every record and every esvio_fe_raw_info field are
compared for equality, tracking results bit for bit.  T is the chain's tile in 64-bit words (512): the lengths and
the carry cases lie around the lane (2 words), the wave (128) and the tile."""
import copy
import ctypes as C

import numpy as np
import pytest

import evt21_ref as E
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times, make_events
from esvio_amd.synth import SceneStream
from raw21_harness import EVENT, OTHER, TOP, Dec, as_words, stream, th_word, tile_words

pytestmark = pytest.mark.gpu

F = E.EVT21
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
FULL = E.event_word(1, 3, 100, 5, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def dec():
    d = Dec()
    yield d
    d.close()


@pytest.mark.parametrize("space", ["host", "device"])
def test_lengths_around_the_lane_the_wave_and_the_tile(dec, space):
    T = tile_words(F)
    assert T == 512
    rng = np.random.default_rng(21)
    for nbytes in (8, 16, 1016, 1024, 1032, 4088, 4096, 4104, 3 * 4096 + 8):
        dec.fresh()
        want, wi = dec.check(F, stream(F, nbytes // 8, rng, triggers=False), space=space,
                             dst_space=FE.DEVICE if space == "device" else FE.HOST, tag=(space, nbytes))
        assert nbytes < 1016 or wi["events"] > 0


def test_page_locked_and_unaligned_sources(dec):
    T = tile_words(F)
    rng = np.random.default_rng(22)
    for skew in (0, 8):
        dec.fresh()
        dec.check(F, stream(F, 3 * T + 1, rng), space="pinned", skew=skew, tag=("pinned", skew))
    # a device source at offset 8 is not 16-byte aligned: read byte by byte, the same answer
    for skew in (8, 4, 1):
        dec.fresh()
        dec.check(F, stream(F, T + 9, rng), space="device", skew=skew, tag=("skew", skew))


def test_the_only_time_high_lies_in_tile_0_and_the_events_in_tile_2(dec):
    T = tile_words(F)
    w = [OTHER[F]] * (2 * T + 20)
    w[5] = th_word(F, 0x0ABCDEF)
    w[2 * T + 2], w[2 * T + 3], w[2 * T + 4] = EVENT[F], E.event_word(0, 63, 2047, 2047, 1 << 31), FULL
    dec.fresh()
    want, wi = dec.check(F, as_words(F, w))
    assert wi["events"] == 2 + 1 + 32 and wi["other"] == 2 * T + 20 - 4
    assert int(want["sec"][0]) * 10 ** 6 + int(want["nsec"][0]) // 1000 == 0x0ABCDEF * 64 + 9
    assert want["x"][2] == 2078 and want["y"][2] == 2047 and want["polarity"][2] == 0


def test_a_wrap_whose_time_highs_sit_on_both_sides_of_a_tile_edge(dec):
    T = tile_words(F)
    w = [EVENT[F]] * (2 * T)
    w[0] = th_word(F, 3)
    w[T - 1], w[T] = th_word(F, TOP[F]), th_word(F, 0)
    dec.fresh()
    want, wi = dec.check(F, as_words(F, w))
    assert wi["wraps"] == 1
    # ... and the state carries the count: a second and a third wrap in ONE call add up
    w2 = [EVENT[F]] * (3 * T + 5)
    w2[10], w2[11] = th_word(F, TOP[F]), th_word(F, 1)
    w2[2 * T + 100], w2[2 * T + 101], w2[2 * T + 102] = th_word(F, TOP[F] - 1), OTHER[F], th_word(F, 0)
    want, wi = dec.check(F, as_words(F, w2))
    assert wi["wraps"] == 3


def test_a_whole_tile_of_full_masks_exact_room_one_short_then_room(dec):
    T = tile_words(F)
    n = 32 * T
    assert n == 16384
    dec.fresh()
    dec.check(F, as_words(F, [th_word(F, 1)]), tag="time base")
    for dst_space in (FE.DEVICE, FE.HOST):
        want, wi = dec.check(F, as_words(F, [FULL] * T), exact_cap=True, dst_space=dst_space, tag=("exact", dst_space))
        assert wi["events"] == n and want["x"][31] == 131 and want["x"][32] == 100
    # one short, with words that would move the state if they were taken over: a wrap in front of the tile
    w2 = as_words(F, [th_word(F, TOP[F]), th_word(F, 0)] + [FULL] * T)
    rc, _, info = dec.call(F, w2, dst_cap=n - 1)
    assert rc == -1 and info.events == n and info.bad == 0 and info.wraps == 0
    assert b"decoder state" in dec.L.esvio_fe_last_error(dec.h)
    want, _ = dec.check(F, as_words(F, [EVENT[F]]), tag="probe from the state before the refusal")
    assert want["nsec"][0] == (64 + 9) * 1000 and want["sec"][0] == 0
    want, wi = dec.check(F, w2, tag="room after the refusal")
    assert wi["events"] == n and wi["wraps"] == 1


def test_a_middle_tile_of_other_words_and_one_of_zero_masks(dec):
    T = tile_words(F)
    rng = np.random.default_rng(23)
    for fill, what in ((OTHER[F], "other"), (E.event_word(1, 7, 300, 200, 0), "zero masks")):
        w = [int(v) for v in stream(F, 3 * T + 50, rng)]
        w[T:2 * T] = [fill] * T
        dec.fresh()
        _, wi = dec.check(F, as_words(F, w), space="device", tag=what)
        assert wi["events"] > 0 and (wi["other"] >= T) == (what == "other")


def test_no_time_high_at_all(dec):
    T = tile_words(F)
    w = [EVENT[F]] * (T + 7)
    dec.fresh()
    want, wi = dec.check(F, as_words(F, w))
    assert wi["events"] == 0 and wi["untimed"] == 2 * (T + 7) and len(want) == 0
    want, _ = dec.check(F, as_words(F, [th_word(F, 2), EVENT[F]]))
    assert len(want) == 2 and want["nsec"][0] == (2 * 64 + 9) * 1000


def test_one_bad_event_in_the_last_tile(dec):
    T = tile_words(F)
    one = E.event_word(1, 0, 5, 5, 1 << 17)
    w = [one] * (2 * T + 9)
    w[0] = th_word(F, 50)
    w[2 * T + 4] = th_word(F, 0)  # (a back-step to time 0 ..)
    w[2 * T + 6:] = [OTHER[F]] * 3  # .. with one event behind it; the offset makes exactly that one negative
    dec.fresh()
    dec.check(F, as_words(F, [th_word(F, 7), EVENT[F]]), tag="before")
    before = copy.deepcopy(dec.st[0])
    _, wi = E.decode(F, as_words(F, w), copy.deepcopy(before), -64)
    assert wi["bad"] == 1
    rc, _, info = dec.call(F, as_words(F, w), off=-64)
    assert rc == -1 and info.bad == 1 and info.events == wi["events"] and info.wraps == before["wraps"]
    assert b"decoder state" in dec.L.esvio_fe_last_error(dec.h)
    dec.check(F, as_words(F, [EVENT[F], OTHER[F], EVENT[F]]), tag="the next call is normal, from the state before the failure")


def test_a_stream_cut_in_two_calls_at_40_positions(dec):
    T = tile_words(F)
    rng = np.random.default_rng(24)
    w = stream(F, 3 * T + 11, rng)
    probe = stream(F, 40, np.random.default_rng(5))[1:]  # (no time base of its own: it shows the carried one)
    whole, _ = E.decode(F, w, E.fresh_state())
    s = E.fresh_state()
    E.decode(F, w, s)
    probe_want, _ = E.decode(F, probe, s)
    cuts = [0, 1, len(w) - 1, len(w)] + [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)] + [127, 128, 129]
    cuts += [int(c) for c in rng.integers(2, len(w) - 1, 40 - len(cuts))]
    assert len(cuts) == 40
    for i, cut in enumerate(cuts):
        dec.fresh()
        space = ("host", "device")[i % 2]
        a, _ = dec.check(F, w[:cut], space=space, tag=(cut, "first"))
        b, _ = dec.check(F, w[cut:], space=space, tag=(cut, "second"))
        assert a.tobytes() + b.tobytes() == whole.tobytes(), cut
        p, _ = dec.check(F, probe, tag=(cut, "probe"))
        assert p.tobytes() == probe_want.tobytes(), cut


def test_argument_errors_come_before_device_work(dec):
    L, h = dec.L, dec.h
    w = as_words(F, [th_word(F, 0), EVENT[F], EVENT[F]])
    out = np.zeros(8, EVENT_DTYPE)
    info = FE.RawInfo()

    def call(fmt=F, nbytes=24, cap=8):
        return L.esvio_fe_decode_raw(h, 0, fmt, FE._p(w), nbytes, FE.HOST, 0, FE._p(out), cap, FE.HOST, C.byref(info))
    dec.fresh()
    for nbytes in (4, 12, 20, 23):
        assert call(nbytes=nbytes) == -1 and b"8-byte words" in L.esvio_fe_last_error(h), nbytes
    for fmt in (0, 1, 4, 20, 22, 210):
        assert call(fmt=fmt) == -1 and b"format" in L.esvio_fe_last_error(h), fmt
    tr, binfo, raw, finfo = FE.Tracks(), FE.BatchInfo(), (FE.RawInfo * 2)(), FE.FeedInfo()
    assert L.esvio_fe_track_raw(h, F, FE._p(w), 20, None, 0, FE.HOST, 0, 1, None, None, C.byref(tr), C.byref(binfo), C.byref(raw)) == -1
    # 4 * n_bytes records always suffice, fewer may not: the count needed comes back
    assert call(cap=3) == -1 and info.events == 4
    dec.check(F, w, tag="after the refusals: from the fresh state")


# ---- end to end --------------------------------------------------------------------------------------------------------
W, H = 346, 260


@pytest.fixture(scope="module")
def frames():
    """5 frames of a scene stream at ~1 Mev/s, each camera's batch in read-out order inside equal stamps: per frame the
    records and the EVT2.1 / EVT2 words (stamps relative to `base`, which travels as t_offset_us)"""
    st = SceneStream(W=W, H=H, rate=1e6, seed=7)
    base = st.t_us - 1000
    out = []
    for _ in range(5):
        left, right, _ = st.next_batch()
        fr = dict(rec=[], words={F: [], E.EVT2: []}, xypt=[])
        for ev in (left, right):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
            o = E.R.readout_order(x, y, p, t)
            x, y, p, t = x[o], y[o], p[o], t[o]
            fr["rec"].append(make_events(x, y, t, p))
            fr["xypt"].append((x, y, p, t))
            for f in (F, E.EVT2):
                fr["words"][f].append(E.encode(f, x, y, p, t - base))
        out.append(fr)
    return base, out


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def make_tracker():
    return FE.FeatureTracker(FE.make_config(W, H, max_cnt=150))


def test_track_raw_equals_track_event_on_the_same_events(frames):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    try:
        for i, fr in enumerate(frs):
            pub = i % 2 == 0
            L, Rr = fr["rec"]
            a.trackEvent(float(event_times(L[-1:])[0]), L, Rr, pub)
            info, raw = b.track_raw(F, fr["words"][F][0], fr["words"][F][1], base, pub)
            assert info.tracked == 1 and (info.kept[0], info.kept[1]) == (len(L), len(Rr)) and info.cur_time == float(event_times(L[-1:])[0])
            assert raw[0].events == len(L) and raw[1].events == len(Rr) and raw[0].untimed == raw[0].bad == 0
            assert results(a) == results(b), i
        assert len(a.ids) > 0 and len(a.ids_right) > 0
        # dense words: more records than one per word, the buffers grow and the emit launch alone is repeated
        dense = as_words(F, [th_word(F, 1)] + [E.event_word(1, 1, 32 * (k % 8), k % 200, 0xFFFFFFFF) for k in range(3000)])
        rec, _ = E.decode(F, dense, E.fresh_state(), base)
        a.trackEvent(float(event_times(rec[-1:])[0]), rec, rec[:32], True)
        b.decode_reset()
        info, raw = b.track_raw(F, dense, dense[:2], base, True)
        assert (info.kept[0], info.kept[1], raw[0].events) == (96000, 32, 96000) and results(a) == results(b)
    finally:
        a.close()
        b.close()


def test_a_feed_fed_evt21_chunks_equals_the_feed_fed_evt2_window_for_window(frames):
    base, frs = frames
    a, b = (FE.FeatureTracker(FE.make_config(W, H, max_cnt=40)) for _ in range(2))
    sizes = (1, 700, 3001, 2, 9000, 333, 4096, 12000)
    try:
        a.feed_open(200.0)
        b.feed_open(200.0)
        tracked = 0
        for fr in frs[:3]:
            for cam in range(2):
                x, y, p, t = fr["xypt"][cam]
                lo, k = 0, cam
                while lo < len(t):
                    hi = min(len(t), lo + sizes[k % len(sizes)])
                    ia = a.feed_push_raw(cam, F, E.encode(F, x[lo:hi], y[lo:hi], p[lo:hi], t[lo:hi] - base), base)
                    ib = b.feed_push_raw(cam, E.EVT2, E.encode(E.EVT2, x[lo:hi], y[lo:hi], p[lo:hi], t[lo:hi] - base), base)
                    assert (ia.appended, ia.closed, ia.queued, ia.bad) == (ib.appended, ib.closed, ib.queued, ib.bad) == (hi - lo, ib.closed, ib.queued, 0)
                    lo, k = hi, k + 1
                    while True:
                        wa, wb = a.feed_peek(), b.feed_peek()
                        assert (wa is None) == (wb is None)
                        if wa is None:
                            break
                        assert (wa.index, wa.end_sec, wa.end_nsec, wa.count[0], wa.count[1]) == (wb.index, wb.end_sec, wb.end_nsec, wb.count[0], wb.count[1])
                        ja, jb = a.feed_track(tracked % 3 != 1), b.feed_track(tracked % 3 != 1)
                        assert (ja.tracked, ja.cur_time, ja.kept[0], ja.kept[1]) == (jb.tracked, jb.cur_time, jb.kept[0], jb.kept[1])
                        if ja.tracked:
                            assert results(a) == results(b), tracked
                        tracked += 1
        assert tracked >= 5 and len(a.ids) > 0
    finally:
        a.close()
        b.close()
