"""GPU: esvio_fe_decode_raw and esvio_fe_track_raw against the sequential restatement tests/evt_ref.py.  Integers only:
all 16 bytes of every record and every esvio_fe_raw_info field are compared for equality, tracking results bit for
bit.  T is the chain's tile in words (esvio_fe_raw_tile_bytes): the lengths and the carry cases lie around its edges."""
import copy
import ctypes as C

import numpy as np
import pytest

import evt_ref as R
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times, make_events
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
FMTS = (R.EVT3, R.EVT2)
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def tile_words(fmt):
    return FE.load_library().esvio_fe_raw_tile_bytes() // R.word_dtype(fmt).itemsize


class Dec:
    """a handle and the restatement's decoder states of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.hip = C.CDLL("libamdhip64.so")
        self.fresh()

    def fresh(self):
        self.ft.decode_reset()
        self.st = [R.fresh_state(), R.fresh_state()]

    def close(self):
        self.ft.close()

    def call(self, fmt, words, cam=0, off=0, space="host", dst_cap=None, dst_space=FE.HOST, skew=0):
        """one esvio_fe_decode_raw call -> (rc, the dst_cap records as bytes, RawInfo); nothing of the restatement moves.
        skew: a device source that many bytes behind a 16-byte boundary"""
        words = np.ascontiguousarray(words, R.word_dtype(fmt))
        nbytes = words.nbytes
        if dst_cap is None:
            dst_cap = nbytes // 2 * 12 if fmt == R.EVT3 else nbytes // 4
        info = FE.RawInfo(first_t_us=-77, last_t_us=-78)
        back = np.full(16 * (dst_cap + 2), GUARD, np.uint8)
        src = dsrc = ddst = psrc = None
        if space == "device":
            dsrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, nbytes + 32, C.byref(dsrc)) == 0
            src, sp = C.c_void_p(dsrc.value + skew), FE.DEVICE
            assert self.L.esvio_fe_mem_upload(src, C.c_void_p(words.ctypes.data), nbytes) == 0
        elif space == "pinned":  # page-locked memory of the library's runtime: read in place by the kernels
            psrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.HOST, nbytes + 32, C.byref(psrc)) == 0
            np.ctypeslib.as_array(C.cast(psrc, C.POINTER(C.c_uint8)), shape=(nbytes + 32,))[skew:skew + nbytes] = words.view(np.uint8)
            src, sp = C.c_void_p(psrc.value + skew), FE.HOST
        else:
            src, sp = C.c_void_p(words.ctypes.data if nbytes else 0), FE.HOST
        if dst_space == FE.DEVICE:
            ddst = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, len(back), C.byref(ddst)) == 0
            assert self.L.esvio_fe_mem_upload(ddst, C.c_void_p(back.ctypes.data), len(back)) == 0
            dst = ddst
        else:
            dst = C.c_void_p(back.ctypes.data)
        rc = self.L.esvio_fe_decode_raw(self.h, cam, fmt, src, nbytes, sp, off, dst, dst_cap, dst_space, C.byref(info))
        if ddst is not None:
            assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(len(back)), 2) == 0
            self.L.esvio_fe_mem_free(FE.DEVICE, ddst)
        if dsrc is not None:
            self.L.esvio_fe_mem_free(FE.DEVICE, dsrc)
        if psrc is not None:
            self.L.esvio_fe_mem_free(FE.HOST, psrc)
        assert (back[16 * dst_cap:] == GUARD).all(), "bytes beyond dst_cap records touched"
        return rc, back[:16 * dst_cap], info

    def check(self, fmt, words, cam=0, off=0, space="host", dst_space=FE.HOST, tag=None, exact_cap=False, skew=0):
        """a call that succeeds equals the restatement, which advances with it -> (records, info of the restatement)"""
        want, wi = R.decode(fmt, np.asarray(words), self.st[cam], off)
        rc, got, info = self.call(fmt, words, cam, off, space, len(want) if exact_cap else None, dst_space, skew)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        for k in ("events", "untimed", "other", "bad", "wraps"):
            assert getattr(info, k) == wi[k], (tag, k, getattr(info, k), wi[k])
        if len(want):
            assert (info.first_t_us, info.last_t_us) == (wi["first_t_us"], wi["last_t_us"]), tag
        else:
            assert (info.first_t_us, info.last_t_us) == (-77, -78), (tag, "untouched if none")
        n = len(want)
        if got[:16 * n].tobytes() != want.tobytes():
            g = got[:16 * n].view(EVENT_DTYPE)
            i = int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0]) // 16
            raise AssertionError((tag, "first differing record", i, g[i], want[i], n))
        assert (got[16 * n:] == GUARD).all(), (tag, "records beyond the count touched")
        return want, wi


@pytest.fixture(scope="module")
def dec():
    d = Dec()
    yield d
    d.close()


def stream(fmt, n, rng):
    """n words with every type: a time base first, then events, vectors, time words and others"""
    if fmt == R.EVT2:
        typ = rng.choice([0, 1, 0, 1, 8, 0xA], n)
        w = (typ.astype(np.int64) << 28) | rng.integers(0, 1 << 28, n)
        th = typ == 8
        w[th] = 0x80000000 | (1000 + np.cumsum(th)[th])
        if n:
            w[0] = 0x80000000 | 1000
        return w.astype("<u4")
    typ = rng.choice([0x0, 0x2, 0x2, 0x3, 0x4, 0x4, 0x5, 0x6, 0x8, 0xA], n)
    w = (typ.astype(np.int64) << 12) | rng.integers(0, 4096, n)
    th = typ == 0x8
    w[th] = 0x8000 | ((100 + np.cumsum(th)[th]) & 0xFFF)
    if n:
        w[0] = 0x8000 | 100
    return w.astype("<u2")


EVENT = {R.EVT3: 0x2000 | 0x800 | 77, R.EVT2: (1 << 28) | (9 << 22) | (77 << 11) | 33}   # one event, p = 1
OTHER = {R.EVT3: 0xE000, R.EVT2: 0xE0000000}


def th_word(fmt, v):
    return (0x8000 | v) if fmt == R.EVT3 else (0x80000000 | v)


# ---- lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("fmt", FMTS)
def test_lengths_around_the_wave_and_the_tile(dec, fmt, space):
    T = tile_words(fmt)
    rng = np.random.default_rng(fmt)
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17):
        dec.fresh()
        want, wi = dec.check(fmt, stream(fmt, n, rng), space=space, dst_space=FE.DEVICE if space == "device" else FE.HOST, tag=(fmt, n))
        assert n < 2 or wi["events"] > 0


@pytest.mark.parametrize("fmt", FMTS)
def test_page_locked_and_unaligned_sources(dec, fmt):
    T = tile_words(fmt)
    rng = np.random.default_rng(40 + fmt)
    # page-locked words are read where they lie, aligned or not
    for skew in (0, 2):
        dec.fresh()
        dec.check(fmt, stream(fmt, 3 * T + 17, rng), space="pinned", skew=skew, tag=(fmt, "pinned", skew))
    # a device source that is not 16-byte aligned is read byte by byte: the same answer
    for skew in (1, 2, 4, 8):
        dec.fresh()
        dec.check(fmt, stream(fmt, T + 9, rng), space="device", skew=skew, tag=(fmt, "skew", skew))


# ---- carry across tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["time_high", "addr_y", "time_low", "vect_base"])
def test_the_only_setter_lies_in_tile_0_and_the_events_in_tile_2(dec, which):
    T = tile_words(R.EVT3)
    w = np.full(2 * T + 40, 0xE000, np.int64)
    w[0] = 0x8005  # (a time base: without one nothing is emitted)
    setter = {"time_high": 0x8123, "addr_y": 0x0155, "time_low": 0x6ABC, "vect_base": 0x3800 | 321}[which]
    w[7] = setter
    w[2 * T + 3:2 * T + 9] = [0x2011, 0x4805, 0x2812, 0x50F0, 0x4FFF, 0x2013]
    dec.fresh()
    want, wi = dec.check(R.EVT3, w.astype("<u2"), tag=which)
    assert wi["events"] == 1 + 3 + 1 + 4 + 12 + 1 and wi["other"] == 2 * T + 40 - 8
    if which == "vect_base":
        assert want["x"][1] == 321 and want["polarity"][1] == 1
    if which == "addr_y":
        assert (want["y"] == 0x155).all()


def test_evt2_time_high_in_tile_0_events_in_tile_2(dec):
    T = tile_words(R.EVT2)
    w = np.full(2 * T + 20, OTHER[R.EVT2], np.int64)
    w[5] = th_word(R.EVT2, 0x0ABCDEF)
    w[2 * T + 2:2 * T + 5] = EVENT[R.EVT2]
    dec.fresh()
    want, wi = dec.check(R.EVT2, w.astype("<u4"))
    assert wi["events"] == 3 and int(want["sec"][0]) * 10 ** 6 + int(want["nsec"][0]) // 1000 == 0x0ABCDEF * 64 + 9


def test_a_vector_run_crosses_a_tile_edge(dec):
    T = tile_words(R.EVT3)
    w = np.full(T + 30, 0x2001, np.int64)
    w[0], w[1], w[2] = 0x8001, 0x0010, 0x3000 | 100
    w[T - 3:T + 3] = [0x4FFF, 0x4A05, 0x4FFF, 0x4FFF, 0x5081, 0x4001]   # bx runs 100, 112, ... across the edge
    dec.fresh()
    want, wi = dec.check(R.EVT3, w.astype("<u2"))
    first_vec = T - 3 - 3  # records in front of the run: one per ADDR_X word
    assert want["x"][first_vec] == 100 and want["x"][first_vec + 12 + 4] == 124 and wi["events"] == (T + 30 - 9) + 12 + 4 + 24 + 2 + 1


@pytest.mark.parametrize("fmt", FMTS)
def test_a_wrap_whose_time_highs_sit_on_both_sides_of_a_tile_edge(dec, fmt):
    T = tile_words(fmt)
    top = 0xFFF if fmt == R.EVT3 else 0x0FFFFFFF
    w = np.full(2 * T, EVENT[fmt], np.int64)
    w[0] = th_word(fmt, 3)
    w[T - 1], w[T] = th_word(fmt, top), th_word(fmt, 0)
    dec.fresh()
    want, wi = dec.check(fmt, w.astype(R.word_dtype(fmt)))
    assert wi["wraps"] == 1
    # ... and the state carries the count: the next call's stamps lie behind the wrap, a second and third wrap in ONE call add up
    w2 = np.full(3 * T + 5, EVENT[fmt], np.int64)
    w2[10], w2[11] = th_word(fmt, top), th_word(fmt, 1)
    w2[2 * T + 100], w2[2 * T + 101], w2[2 * T + 102] = th_word(fmt, top - 1), OTHER[fmt], th_word(fmt, 0)
    want, wi = dec.check(fmt, w2.astype(R.word_dtype(fmt)))
    assert wi["wraps"] == 3


@pytest.mark.parametrize("fmt", FMTS)
def test_a_whole_middle_tile_of_other_words(dec, fmt):
    T = tile_words(fmt)
    rng = np.random.default_rng(11)
    w = stream(fmt, 3 * T + 50, rng).astype(np.int64)
    w[T:2 * T] = OTHER[fmt]
    dec.fresh()
    _, wi = dec.check(fmt, w.astype(R.word_dtype(fmt)), space="device")
    assert wi["other"] >= T and wi["events"] > 0


# ---- expansion ---------------------------------------------------------------------------------------------------------
def test_full_vectors_exact_room_one_short_then_room(dec):
    T = tile_words(R.EVT3)
    w = np.array([0x8001, 0x0003, 0x3000] + [0x4FFF] * (T + 5), "<u2")
    n = 12 * (T + 5)
    dec.fresh()
    dec.check(R.EVT3, w, exact_cap=True, dst_space=FE.DEVICE, tag="exact")
    # one short, with words that would move every field of the state if they were taken over: a wrap, TIME_LOW, ADDR_Y,
    # a vector base and its polarity, and bx behind the run
    w2 = np.array([0x8FFF, 0x8000, 0x6123, 0x0155, 0x3800 | 700] + [0x4FFF] * (T + 5), "<u2")
    rc, _, info = dec.call(R.EVT3, w2, dst_cap=n - 1)
    assert rc == -1 and info.events == n and info.bad == 0 and info.wraps == 0
    assert b"decoder state" in dec.L.esvio_fe_last_error(dec.h)
    # the restatement has not moved either: a probe without a setter of its own shows th, wraps, tl, y, bx and bp
    want, _ = dec.check(R.EVT3, np.array([0x2005, 0x4003, 0x5001], "<u2"), tag="probe from the state before the refusal")
    assert (want["y"] == 3).all() and want["nsec"][0] == 4096 * 1000 and want["x"][1] == (12 * (T + 5)) & 0xFFFF and want["polarity"][1] == 0
    # ... and the same words with room give the full answer, and now the state moves
    want, wi = dec.check(R.EVT3, w2, tag="room after the refusal")
    assert wi["events"] == n and wi["wraps"] == 1 and want["y"][0] == 0x155 and want["polarity"][0] == 1


def test_more_events_than_the_first_buffers_hold(dec):
    """72000 events from 6003 words: above the one-record-per-word (and 65536-record) buffers both entry points begin
    with — the emit launch is repeated into buffers of the reported size"""
    w = np.array([0x8001, 0x0003, 0x3000] + [0x4FFF] * 6000, "<u2")
    dec.fresh()
    want, wi = dec.check(R.EVT3, w, tag="host dst behind grown records")
    assert wi["events"] == 72000
    a, b = make_tracker(), make_tracker()
    try:
        rec, _ = R.decode(R.EVT3, w, R.fresh_state(), 5_000_000)
        small = np.array([0x8001, 0x0003, 0x2004], "<u2")
        a.trackEvent(float(event_times(rec[-1:])[0]), rec, rec[:1], True)
        info, raw = b.track_raw(R.EVT3, w, small, 5_000_000, True)
        assert (info.kept[0], info.kept[1], info.tracked, raw[0].events) == (72000, 1, 1, 72000)
        assert results(a) == results(b)
        info, raw = b.track_raw(R.EVT3, w, small, 5_000_000, True)  # (the second call of the size: nothing grows)
        assert info.kept[0] == 72000
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_no_time_high_at_all(dec, fmt):
    T = tile_words(fmt)
    w = np.full(T + 7, EVENT[fmt], np.int64)
    if fmt == R.EVT3:
        w[3], w[4], w[5], w[T + 1] = 0x0123, 0x6456, 0x3000 | 50, 0x40FF
    dec.fresh()
    want, wi = dec.check(fmt, w.astype(R.word_dtype(fmt)))
    assert wi["events"] == 0 and wi["untimed"] >= T and len(want) == 0
    # the state has advanced all the same: a time base and one event show y, tl, bx
    follow = [th_word(fmt, 2), EVENT[fmt]] + ([0x4001] if fmt == R.EVT3 else [])
    want, _ = dec.check(fmt, np.array(follow, R.word_dtype(fmt)))
    if fmt == R.EVT3:
        assert want["y"][0] == 0x123 and want["nsec"][0] == (2 * 4096 + 0x456) * 1000 and want["x"][1] == 50 + 12


# ---- carry across calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_a_stream_cut_in_two_calls_at_40_positions(dec, fmt):
    T = tile_words(fmt)
    rng = np.random.default_rng(21 + fmt)
    w = stream(fmt, 3 * T + 11, rng)
    if fmt == R.EVT3:
        w[T + 200:T + 206] = [0x3000 | 700, 0x4FFF, 0x4F0F, 0x4FFF, 0x50FF, 0x4FFF]  # a vector run to cut in the middle
    probe = stream(fmt, 40, np.random.default_rng(5))[1:]  # (no time base of its own: it shows the carried one)
    whole, _ = R.decode(fmt, w, R.fresh_state())
    s = R.fresh_state()
    R.decode(fmt, w, s)
    probe_want, _ = R.decode(fmt, probe, s)
    cuts = [0, 1, len(w) - 1, len(w)] + [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    cuts += [T + 201, T + 202, T + 203, T + 204] if fmt == R.EVT3 else [T + 201]
    cuts += [int(c) for c in rng.integers(2, len(w) - 1, 40 - len(cuts))]
    assert len(cuts) == 40
    for i, cut in enumerate(cuts):
        dec.fresh()
        space = ("host", "device")[i % 2]
        a, _ = dec.check(fmt, w[:cut], space=space, tag=(fmt, cut, "first"))
        b, _ = dec.check(fmt, w[cut:], space=space, tag=(fmt, cut, "second"))
        assert a.tobytes() + b.tobytes() == whole.tobytes(), cut
        p, _ = dec.check(fmt, probe, tag=(fmt, cut, "probe"))
        assert p.tobytes() == probe_want.tobytes(), cut


# ---- BAD, resets, arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_one_bad_event_in_the_last_tile(dec, fmt):
    T = tile_words(fmt)
    w = np.full(2 * T + 9, EVENT[fmt], np.int64)
    w[0] = th_word(fmt, 50)
    w[2 * T + 4] = th_word(fmt, 0)  # (a back-step to time 0 ..)
    w[2 * T + 6:] = OTHER[fmt]      # .. with one event behind it; the offset makes exactly that one negative
    tick = 4096 if fmt == R.EVT3 else 64
    off = -tick
    dec.fresh()
    dec.check(fmt, [th_word(fmt, 7), EVENT[fmt]], tag="before")
    before = copy.deepcopy(dec.st[0])
    _, wi = R.decode(fmt, w.astype(R.word_dtype(fmt)), copy.deepcopy(before), off)
    assert wi["bad"] == 1
    rc, _, info = dec.call(fmt, w.astype(R.word_dtype(fmt)), off=off)
    assert rc == -1 and info.bad == 1 and info.events == wi["events"] and info.wraps == before["wraps"]
    assert b"decoder state" in dec.L.esvio_fe_last_error(dec.h)
    dec.check(fmt, [EVENT[fmt], OTHER[fmt], EVENT[fmt]], tag="the next call is normal, from the state before the failure")


def test_decode_reset_and_reset_bring_back_the_fresh_state(dec):
    for how in ("decode_reset", "reset"):
        for cam in (0, 1):
            dec.check(R.EVT3, [0x8FFF, 0x6111, 0x0022, 0x3833, 0x8000, 0x2001], cam=cam, tag="dirty")
        getattr(dec.ft, how)()
        dec.st = [R.fresh_state(), R.fresh_state()]
        for cam in (0, 1):
            want, wi = dec.check(R.EVT3, [0x2001, 0x4001, 0x8000, 0x2001, 0x4001], cam=cam, tag=how)
            assert wi["untimed"] == 2 and wi["wraps"] == 0 and want["y"][0] == 0 and want["x"][1] == 12 and want["nsec"][0] == 0


def test_argument_errors_come_before_device_work(dec):
    L, h = dec.L, dec.h
    w = np.array([0x8000, 0x2001, 0x2002, 0x2003], "<u2")
    out = np.zeros(8, EVENT_DTYPE)
    info = FE.RawInfo()
    p, o = FE._p(w), FE._p(out)

    def call(cam=0, fmt=R.EVT3, words=p, nbytes=8, space=FE.HOST, off=0, dst=o, cap=8, dsp=FE.HOST):
        return L.esvio_fe_decode_raw(h, cam, fmt, words, nbytes, space, off, dst, cap, dsp, C.byref(info))
    dec.fresh()
    assert call(cam=2) == -1 and call(fmt=4) == -1 and call(space=5) == -1 and call(dsp=7) == -1
    assert call(words=None) == -1 and call(dst=None) == -1
    assert call(nbytes=7) == -1 and call(fmt=R.EVT2, nbytes=6) == -1
    assert call(off=(1 << 62) + 1) == -1 and call(off=-(1 << 62) - 1) == -1
    assert call(dst=C.c_void_p(out.ctypes.data + 8), dsp=FE.DEVICE) == -1  # misaligned device dst
    assert call(nbytes=0, words=None, dst=None, cap=0) == 0
    tr, binfo, raw = FE.Tracks(), FE.BatchInfo(), (FE.RawInfo * 2)()
    bad_prm = FE.FilterParams(0, 9, 0)
    for kw in (dict(fmt=9), dict(space=3), dict(lb=7), dict(left=None), dict(off=(1 << 62) + 1), dict(prm=C.byref(bad_prm))):
        a = dict(fmt=R.EVT3, left=p, lb=8, space=FE.HOST, off=0, prm=None)
        a.update(kw)
        assert L.esvio_fe_track_raw(h, a["fmt"], a["left"], a["lb"], None, 0, a["space"], a["off"], 1, a["prm"], None, C.byref(tr),
                                    C.byref(binfo), C.byref(raw)) == -1, kw
    # none of them moved the state: the first real call decodes from the fresh one
    dec.check(R.EVT3, w, tag="after the refusals")


# ---- end to end --------------------------------------------------------------------------------------------------------
W, H = 346, 260


@pytest.fixture(scope="module")
def frames():
    """6 frames of a scene stream at ~1 Mev/s, each camera's batch in read-out order inside equal stamps: per frame the
    records, and the words of both formats (stamps relative to `base`, which travels as t_offset_us)"""
    st = SceneStream(W=W, H=H, rate=1e6, seed=7)
    base = st.t_us - 1000
    out = []
    for _ in range(6):
        left, right, _ = st.next_batch()
        fr = dict(rec=[], words={f: [] for f in FMTS})
        for ev in (left, right):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
            o = R.readout_order(x, y, p, t)
            x, y, p, t = x[o], y[o], p[o], t[o]
            fr["rec"].append(make_events(x, y, t, p))
            for f in FMTS:
                fr["words"][f].append(R.encode(f, x, y, p, t - base))
        out.append(fr)
    assert any(((fr["words"][R.EVT3][0] >> 12) == 4).any() for fr in out), "no vector word in the stream"
    return base, out


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def make_tracker():
    return FE.FeatureTracker(FE.make_config(W, H, max_cnt=150))


@pytest.mark.parametrize("fmt", FMTS)
def test_track_raw_equals_track_event_on_the_same_events(frames, fmt):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    try:
        for i, fr in enumerate(frs):
            pub = i % 2 == 0 or i == 5
            L, Rr = fr["rec"]
            a.trackEvent(float(event_times(L[-1:])[0]), L, Rr, pub)
            info, raw = b.track_raw(fmt, fr["words"][fmt][0], fr["words"][fmt][1], base, pub)
            assert info.tracked == 1 and (info.kept[0], info.kept[1]) == (len(L), len(Rr)) and info.cur_time == float(event_times(L[-1:])[0])
            assert raw[0].events == len(L) and raw[1].events == len(Rr) and raw[0].untimed == raw[0].bad == 0
            assert results(a) == results(b), (fmt, i)
        assert len(a.ids) > 0 and len(a.ids_right) > 0
    finally:
        a.close()
        b.close()


def test_track_raw_with_a_filter_equals_track_batch_on_the_records(frames):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    prm = FE.FilterParams(5_000_000, 1, 200_000)
    try:
        for i, fr in enumerate(frs):
            L, Rr = fr["rec"]
            ia = a.track_batch(L, Rr, pub=True, params=prm)
            ib, raw = b.track_raw(R.EVT3, fr["words"][R.EVT3][0], fr["words"][R.EVT3][1], base, True, params=prm)
            assert (ia.kept[0], ia.kept[1], ia.rejected[0], ia.cur_time, ia.tracked) == (ib.kept[0], ib.kept[1], ib.rejected[0], ib.cur_time, ib.tracked)
            assert 0 < ib.kept[0] < raw[0].events == len(L)
            assert results(a) == results(b), i
    finally:
        a.close()
        b.close()


def test_track_raw_with_motion_equals_track_event_mc(frames):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    try:
        for i, fr in enumerate(frs[:4]):
            L, Rr = fr["rec"]
            t1 = float(event_times(L[-1:])[0])
            m = FE.make_motion(t1, (0.4, -0.2, 0.1), (0.1, 0.0, 0.0), (6.0, 2.0, -1.0), (0.3, -0.5, 0.2), 0.9 * W, 0.9 * W, W / 2.0, H / 2.0)
            a.trackEvent(t1, L, Rr, True, measurements=m)
            info, _ = b.track_raw(R.EVT2, fr["words"][R.EVT2][0], fr["words"][R.EVT2][1], base, True, measurements=m)
            assert info.tracked == 1
            assert results(a) == results(b), i
    finally:
        a.close()
        b.close()


def test_decode_raw_between_two_track_calls_changes_no_later_result(frames):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    try:
        for i, fr in enumerate(frs[:4]):
            L, Rr = fr["rec"]
            t = float(event_times(L[-1:])[0])
            a.trackEvent(t, L, Rr, True)
            b.trackEvent(t, L, Rr, True)
            rec, info = b.decode_raw(1, R.EVT3, fr["words"][R.EVT3][0], base)
            assert rec.tobytes() == L.tobytes() and info.events == len(L)
            dev, _ = b.decode_raw(0, R.EVT2, fr["words"][R.EVT2][1], base, device=True)
            dev.free()
            assert results(a) == results(b), i
    finally:
        a.close()
        b.close()


def test_track_raw_is_refused_while_batches_are_announced(frames):
    base, frs = frames
    ft = make_tracker()
    try:
        L, Rr = frs[0]["rec"]
        dl, dr = FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(Rr, FE.DEVICE)
        ft.set_next_batch(float(event_times(L[-1:])[0]), dl.arg, dr.arg, True)
        with pytest.raises(FE.FrontendError, match="announced"):
            ft.track_raw(R.EVT3, frs[0]["words"][R.EVT3][0], frs[0]["words"][R.EVT3][1], base)
        ft.trackEvent(float(event_times(L[-1:])[0]), dl.arg, dr.arg, True)
        dl.free()
        dr.free()
    finally:
        ft.close()
