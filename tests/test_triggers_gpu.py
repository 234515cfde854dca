"""GPU: esvio_fe_decode_triggers for EVT3, EVT2 and EVT2.1 words against the sequential restatement
tests/evt21_ref.py (decode_triggers).  Integers only: all 16 bytes of every trigger record and every
esvio_fe_trigger_info field are compared for equality.  The lengths and the carry cases lie around the lane (16 bytes),
the wave (1024) and the tile (4096)."""
import copy
import ctypes as C

import numpy as np
import pytest

import evt21_ref as E
from esvio_amd import frontend as FE
from raw21_harness import EVENT, FMTS, OTHER, TOP, Dec, as_words, stream, th_word, tile_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec():
    d = Dec()
    yield d
    d.close()


def trig(fmt, tid=3, value=1, tlow=11):
    return E.trigger_word(fmt, tid, value, tlow)


@pytest.mark.parametrize("fmt", FMTS)
def test_lengths_around_the_lane_the_wave_and_the_tile(dec, fmt):
    wb = E.word_dtype(fmt).itemsize
    rng = np.random.default_rng(30 + fmt)
    lengths = [wb] + [b + d for b in (16, 1024, 4096) for d in (-wb, 0, wb)] + [3 * 4096 + wb]
    for i, nbytes in enumerate(lengths):
        dec.fresh()
        w = stream(fmt, nbytes // wb, rng)
        want, wi = dec.tcheck(fmt, w, space=("host", "device", "pinned")[i % 3], tag=(fmt, nbytes))
        assert nbytes < 1024 or wi["triggers"] > 0
    dec.fresh()
    dec.tcheck(fmt, stream(fmt, tile_words(fmt) + 9, rng), space="device", skew=wb, tag=(fmt, "a device source that is not 16-byte aligned"))
    rc, _, info = dec.tcall(fmt, as_words(fmt, []))
    assert rc == 0 and info.triggers == 0


@pytest.mark.parametrize("fmt", FMTS)
def test_the_only_setter_lies_in_tile_0_and_the_triggers_in_tile_2(dec, fmt):
    T = tile_words(fmt)
    w = [OTHER[fmt]] * (2 * T + 20)
    w[5] = th_word(fmt, 0x123)
    if fmt == E.EVT3:
        w[9] = 0x6ABC  # TIME_LOW: the trigger's low bits come from the state
    w[T + 1] = EVENT[fmt]  # (event words change nothing here)
    w[2 * T + 2], w[2 * T + 3], w[2 * T + 7] = trig(fmt, 3, 1, 11), trig(fmt, 15, 0, 63), trig(fmt, 0, 1, 0)
    dec.fresh()
    want, wi = dec.tcheck(fmt, as_words(fmt, w))
    assert wi["triggers"] == 3 and want["id"].tolist() == [3, 15, 0] and want["value"].tolist() == [1, 0, 1]
    t0 = 0x123 * 4096 + 0xABC if fmt == E.EVT3 else 0x123 * 64 + 11
    assert int(want["sec"][0]) * 10 ** 6 + int(want["nsec"][0]) // 1000 == t0


@pytest.mark.parametrize("fmt", FMTS)
def test_a_wrap_whose_time_highs_sit_on_both_sides_of_a_tile_edge(dec, fmt):
    T = tile_words(fmt)
    w = [trig(fmt)] * (2 * T)
    w[0] = th_word(fmt, 3)
    w[T - 1], w[T] = th_word(fmt, TOP[fmt]), th_word(fmt, 0)
    dec.fresh()
    want, wi = dec.tcheck(fmt, as_words(fmt, w))
    assert wi["wraps"] == 1 and wi["triggers"] == 2 * T - 3
    w2 = [trig(fmt, 1, 0)] * (T + 5)
    w2[10], w2[11] = th_word(fmt, TOP[fmt]), th_word(fmt, 1)
    want, wi = dec.tcheck(fmt, as_words(fmt, w2), space="device")
    assert wi["wraps"] == 2  # (the state carries the count)


@pytest.mark.parametrize("fmt", FMTS)
def test_a_stream_cut_in_two_calls_at_40_positions(dec, fmt):
    T = tile_words(fmt)
    rng = np.random.default_rng(40 + fmt)
    n = 2 * T + 11
    w = stream(fmt, n, rng)
    probe = stream(fmt, 40, np.random.default_rng(5))[1:]  # (no time base of its own: it shows the carried one)
    whole, _ = E.decode_triggers(fmt, w, E.fresh_state())
    s = E.fresh_state()
    E.decode_triggers(fmt, w, s)
    probe_want, _ = E.decode_triggers(fmt, probe, s)
    cuts = [0, 1, n - 1, n] + [k * T + d for k in (1, 2) for d in (-1, 0, 1)]
    cuts += [int(c) for c in rng.integers(2, n - 1, 40 - len(cuts))]
    assert len(cuts) == 40 and len(whole) > 20
    for i, cut in enumerate(cuts):
        dec.fresh()
        space = ("host", "device")[i % 2]
        a, _ = dec.tcheck(fmt, w[:cut], space=space, tag=(fmt, cut, "first"))
        b, _ = dec.tcheck(fmt, w[cut:], space=space, tag=(fmt, cut, "second"))
        assert a.tobytes() + b.tobytes() == whole.tobytes(), cut
        p, _ = dec.tcheck(fmt, probe, tag=(fmt, cut, "probe"))
        assert p.tobytes() == probe_want.tobytes(), cut


@pytest.mark.parametrize("fmt", FMTS)
def test_dst_cap_exact_and_one_short_untimed_and_bad(dec, fmt):
    T = tile_words(fmt)
    w = as_words(fmt, [trig(fmt, 2, 1, 5), th_word(fmt, TOP[fmt]), th_word(fmt, 0)] + [trig(fmt, 7, 0, 1), OTHER[fmt]] * T)
    dec.fresh()
    dec.tcheck(fmt, as_words(fmt, [th_word(fmt, 9), trig(fmt)]), tag="before")
    before = copy.deepcopy(dec.tst[0])
    rc, _, info = dec.tcall(fmt, w, dst_cap=T)  # needs T + 1: the first trigger is timed by the carried state
    assert rc == -1 and info.triggers == T + 1 and info.bad == 0 and info.wraps == 0
    assert b"trigger-decoder state" in dec.L.esvio_fe_last_error(dec.h)
    assert dec.tst[0] == before
    dec.tcheck(fmt, as_words(fmt, [trig(fmt, 4, 0, 2)]), tag="probe from the state before the refusal")
    want, wi = dec.tcheck(fmt, w, exact_cap=True, tag="exact room")
    assert wi["triggers"] == T + 1 and wi["wraps"] == 1
    # untimed: a fresh decoder has no time base
    dec.fresh()
    want, wi = dec.tcheck(fmt, as_words(fmt, [trig(fmt), trig(fmt), th_word(fmt, 1), trig(fmt)]))
    assert (wi["untimed"], wi["triggers"]) == (2, 1)
    # BAD: the state stays, the count is exact
    before = copy.deepcopy(dec.tst[0])
    rc, _, info = dec.tcall(fmt, as_words(fmt, [th_word(fmt, 0), trig(fmt, 1, 1, 0), th_word(fmt, 5), trig(fmt)]), off=-1)
    assert rc == -1 and info.bad == 1 and info.triggers == 2
    dec.tcheck(fmt, as_words(fmt, [trig(fmt)]), tag="after BAD: from the state before it")


@pytest.mark.parametrize("fmt", FMTS)
def test_events_and_triggers_of_the_same_chunks_in_either_order_share_one_time_base(dec, fmt):
    T = tile_words(fmt)
    rng = np.random.default_rng(50 + fmt)
    w = stream(fmt, 2 * T + 30, rng)
    ev_whole, _ = E.decode(fmt, w, E.fresh_state(), 1234)
    tr_whole, _ = E.decode_triggers(fmt, w, E.fresh_state(), 1234)
    edges = [0, 17, T - 1, T + 200, 2 * T + 30]
    for order in (0, 1):
        dec.fresh()
        ev, tr = [], []
        for k in range(len(edges) - 1):
            chunk = w[edges[k]:edges[k + 1]]
            if (k + order) % 2 == 0:
                ev.append(dec.check(fmt, chunk, off=1234)[0])
                tr.append(dec.tcheck(fmt, chunk, off=1234)[0])
            else:
                tr.append(dec.tcheck(fmt, chunk, off=1234)[0])
                ev.append(dec.check(fmt, chunk, off=1234)[0])
        assert b"".join(c.tobytes() for c in ev) == ev_whole.tobytes() and b"".join(c.tobytes() for c in tr) == tr_whole.tobytes()
    # the two cameras' trigger decoders are two states
    dec.fresh()
    dec.tcheck(fmt, as_words(fmt, [th_word(fmt, 77), trig(fmt)]), cam=0)
    _, wi = dec.tcheck(fmt, as_words(fmt, [trig(fmt)]), cam=1)
    assert wi["untimed"] == 1


def test_more_triggers_than_the_stage_keeps_room_for(dec):
    """70 000 triggers in one chunk: above the 65 536 records the stage's device buffer begins with — it grows to the
    count the reduce pass reports and the emit launch alone is repeated"""
    w = np.full(70001, 0xA501, "<u2")
    w[0] = 0x8002
    w[1::7] ^= 1
    dec.fresh()
    want, wi = dec.tcheck(E.EVT3, w, cam=1)
    assert wi["triggers"] == 70000 and want["id"][0] == 5 and want["nsec"][-1] == 2 * 4096 * 1000
    rc, _, info = dec.tcall(E.EVT3, w, cam=1, dst_cap=69999)
    assert rc == -1 and info.triggers == 70000


@pytest.mark.parametrize("how", ["decode_reset", "reset"])
def test_decode_reset_and_reset_clear_both_states(dec, how):
    fmt = E.EVT3
    dirty = as_words(fmt, [0x8FFF, 0x6111, 0x8000, 0x2001, 0xA301])
    dec.fresh()
    for cam in (0, 1):
        dec.check(fmt, dirty, cam=cam)
        _, wi = dec.tcheck(fmt, dirty, cam=cam)
        assert wi["wraps"] == 1 and wi["triggers"] == 1
    getattr(dec.ft, how)()
    dec.st, dec.tst = [E.fresh_state(), E.fresh_state()], [E.fresh_state(), E.fresh_state()]
    for cam in (0, 1):
        _, wi = dec.tcheck(fmt, as_words(fmt, [0xA001, 0x8000, 0xA001]), cam=cam, tag=how)
        assert (wi["untimed"], wi["triggers"], wi["wraps"], wi["first_t_us"]) == (1, 1, 0, 0)
        _, wi = dec.check(fmt, as_words(fmt, [0x2001, 0x8000, 0x2001]), cam=cam, tag=how)
        assert (wi["untimed"], wi["events"], wi["wraps"]) == (1, 1, 0)


def test_argument_errors_come_before_device_work(dec):
    L, h = dec.L, dec.h
    w = as_words(E.EVT3, [0x8000, 0xA001, 0xA101, 0xA201])
    out = np.zeros(8, E.TRIGGER_DTYPE)
    info = FE.TriggerInfo()

    def call(cam=0, fmt=E.EVT3, words=FE._p(w), nbytes=8, space=FE.HOST, off=0, dst=FE._p(out), cap=8):
        return L.esvio_fe_decode_triggers(h, cam, fmt, words, nbytes, space, off, dst, cap, C.byref(info))
    dec.fresh()
    assert call(cam=2) == -1 and call(fmt=4) == -1 and call(space=5) == -1 and call(words=None) == -1 and call(dst=None) == -1
    assert call(nbytes=7) == -1 and call(fmt=E.EVT2, nbytes=6) == -1 and call(fmt=E.EVT21, nbytes=4) == -1
    assert call(off=(1 << 62) + 1) == -1
    assert call(nbytes=0, words=None, dst=None, cap=0) == 0
    dec.tcheck(E.EVT3, w, tag="after the refusals: from the fresh state")
    # the Python layer
    dec.fresh()
    rec, ti = dec.ft.decode_triggers(0, E.EVT3, w, 5)
    assert rec.dtype == FE.TRIGGER_DTYPE and rec["id"].tolist() == [0, 1, 2] and ti.triggers == 3 and ti.first_t_us == 5
    with pytest.raises(FE.FrontendError) as e:
        dec.ft.decode_triggers(0, E.EVT3, w, 0, dst_cap=2)
    assert e.value.info.triggers == 3
