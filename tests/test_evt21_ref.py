"""CPU: the sequential readings tests/evt21_ref.py (EVT2.1 events, triggers of the three formats) and
tests/slice_at_ref.py (windows at given stamps) against answers derived by hand from the text of include/esvio_fe.h.

One hand-derived word differs from the literal the feature's issue printed: POS, tlow 5, x 64, y 7, mask 0x80000001
is 1 << 60 | 5 << 54 | 64 << 43 | 7 << 32 | mask = 0x1142000780000001 by the layout (bx = (w >> 43) & 0x7FF); the issue's
0x1140200780000001 has bx = 4 under that same layout.  The layout is the specification, so the word below is the
layout's, and the issue's expected events — (64, 7, 1, 69) and (95, 7, 1, 69) — are what it yields."""
import copy

import numpy as np
import pytest

import evt21_ref as E
import slice_at_ref as SA
from esvio_amd.events import make_events


def xypt(rec):
    t = rec["sec"].astype(np.int64) * 10 ** 6 + rec["nsec"].astype(np.int64) // 1000
    return [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(rec["x"], rec["y"], rec["polarity"], t)]


def test_hand_derived_evt21_words():
    assert E.th_word(1) == 0x8000000100000000
    w = E.event_word(1, 5, 64, 7, 0x80000001)
    assert w == (1 << 60) | (5 << 54) | (64 << 43) | (7 << 32) | 0x80000001 == 0x1142000780000001
    rec, info = E.decode(E.EVT21, [0x8000000100000000, w], E.fresh_state())
    assert xypt(rec) == [(64, 7, 1, 69), (95, 7, 1, 69)]
    assert (info["events"], info["untimed"], info["other"], info["bad"], info["first_t_us"], info["last_t_us"]) == (2, 0, 0, 0, 69, 69)
    assert rec.view(np.uint8).reshape(-1, 16)[:, 13:].sum() == 0  # the padding bytes
    # NEG, a zero mask (nothing, counted nowhere), another type (other)
    rec, info = E.decode(E.EVT21, [E.th_word(2), E.event_word(0, 63, 10, 3, 0b101), E.event_word(1, 1, 1, 1, 0), 0xE << 60], E.fresh_state())
    assert xypt(rec) == [(10, 3, 0, 191), (12, 3, 0, 191)] and (info["events"], info["other"], info["untimed"]) == (2, 1, 0)


def test_evt21_wrap_back_step_untimed_and_the_widest_x():
    top = 0x0FFFFFFF
    ev = E.event_word(1, 0, 0, 0, 1)
    s = E.fresh_state()
    rec, info = E.decode(E.EVT21, [ev, E.event_word(0, 0, 5, 5, 0xF0), E.th_word(top), ev, E.th_word(0), ev], s)
    assert info["untimed"] == 1 + 4 and info["wraps"] == 1 and info["events"] == 2
    assert [t for *_, t in xypt(rec)] == [top * 64, 1 << 34]
    # a back-step below the half range is a back-step: time goes back, no wrap
    rec, info = E.decode(E.EVT21, [E.th_word(1 << 27), ev, E.th_word(1), ev, E.th_word((1 << 27) + 1), E.th_word(1), ev], s)
    assert info["wraps"] == 1 + 1 and [t for *_, t in xypt(rec)] == [(1 << 34) + (1 << 33), (1 << 34) + 64, (2 << 34) + 64]
    # bx need not be 32-aligned and x may leave 11 bits: 2047 + 31
    rec, _ = E.decode(E.EVT21, [E.th_word(0), E.event_word(1, 0, 2047, 9, 1 << 31)], E.fresh_state())
    assert xypt(rec) == [(2078, 9, 1, 0)]
    # BAD: ticks < 0 or sec >= 2^32, in exact integers
    _, info = E.decode(E.EVT21, [E.th_word(0), ev], E.fresh_state(), -1)
    assert info["bad"] == 1
    _, info = E.decode(E.EVT21, [E.th_word(0), ev], E.fresh_state(), (1 << 32) * 10 ** 6)
    assert info["bad"] == 1


def test_hand_derived_triggers():
    rec, info = E.decode_triggers(E.EVT3, [0x8001, 0x6005, 0xA301], E.fresh_state())
    assert [tuple(int(v) for v in (r["sec"], r["nsec"], r["id"], r["value"])) for r in rec] == [(0, 4101000, 3, 1)]
    assert info == dict(triggers=1, untimed=0, bad=0, wraps=0, first_t_us=4101, last_t_us=4101)
    assert rec.dtype.itemsize == 16 and rec["_pad"].sum() == 0
    # EVT2: tlow 9, id 17, value 0 behind TIME_HIGH 3; an event word and an OTHERS word between change nothing
    w = [0x80000003, (1 << 28) | 5, 0xE0000000, E.trigger_word(E.EVT2, 17, 0, 9)]
    assert w[3] == (0xA << 28) | (9 << 22) | (17 << 8)
    rec, info = E.decode_triggers(E.EVT2, w, E.fresh_state(), 1_000_000)
    assert (int(rec["sec"][0]), int(rec["nsec"][0]), int(rec["id"][0]), int(rec["value"][0])) == (1, (3 * 64 + 9) * 1000, 17, 0)
    # EVT2.1: id at bit 40, value at bit 32, tlow at bit 54
    w = [E.th_word(2), E.trigger_word(E.EVT21, 31, 1, 63)]
    assert w[1] == (0xA << 60) | (63 << 54) | (31 << 40) | (1 << 32)
    rec, info = E.decode_triggers(E.EVT21, w, E.fresh_state())
    assert (int(rec["nsec"][0]), int(rec["id"][0]), int(rec["value"][0])) == (191000, 31, 1)
    # untimed, a wrap, BAD
    s = E.fresh_state()
    rec, info = E.decode_triggers(E.EVT3, [0xA001, 0x8FFF, 0xA100, 0x8000, 0x6001, 0xA201], s)
    assert (info["untimed"], info["triggers"], info["wraps"]) == (1, 2, 1)
    assert (info["first_t_us"], info["last_t_us"]) == (0xFFF * 4096, (1 << 24) + 1)
    _, info = E.decode_triggers(E.EVT3, [0xA001], copy.deepcopy(s), -(1 << 24) - 2)
    assert info["bad"] == 1


@pytest.mark.parametrize("fmt", [E.EVT21, E.EVT3, E.EVT2])
def test_decode_whole_equals_decode_parts_at_every_word(fmt):
    rng = np.random.default_rng(fmt)
    n = 60
    if fmt == E.EVT21:
        typ = rng.choice([0, 1, 1, 8, 0xA, 0xE], n)
        w = [(int(t) << 60) | int(rng.integers(0, 1 << 60)) for t in typ]
    elif fmt == E.EVT2:
        typ = rng.choice([0, 1, 8, 0xA, 0xA, 0xE], n)
        w = [(int(t) << 28) | int(rng.integers(0, 1 << 28)) for t in typ]
    else:
        typ = rng.choice([0x0, 0x2, 0x3, 0x4, 0x6, 0x8, 0xA, 0xA], n)
        w = [(int(t) << 12) | int(rng.integers(0, 4096)) for t in typ]
    whole_e, ie = E.decode(fmt, w, E.fresh_state(), 7)
    whole_t, it = E.decode_triggers(fmt, w, E.fresh_state(), 7)
    assert it["triggers"] + it["untimed"] == int((np.asarray(typ) == 0xA).sum()) and it["triggers"] > 0
    for cut in range(n + 1):
        se, st = E.fresh_state(), E.fresh_state()
        a, ia = E.decode(fmt, w[:cut], se, 7)
        b, ib = E.decode(fmt, w[cut:], se, 7)
        assert a.tobytes() + b.tobytes() == whole_e.tobytes() and ib["wraps"] == ie["wraps"]
        assert ia["untimed"] + ib["untimed"] == ie["untimed"] and ia["other"] + ib["other"] == ie["other"]
        a, ia = E.decode_triggers(fmt, w[:cut], st, 7)
        b, ib = E.decode_triggers(fmt, w[cut:], st, 7)
        assert a.tobytes() + b.tobytes() == whole_t.tobytes() and ib["wraps"] == it["wraps"]
        assert ia["untimed"] + ib["untimed"] == it["untimed"]


def test_the_encoder_round_trips_and_uses_vectors():
    rng = np.random.default_rng(3)
    n = 500
    t = np.sort(rng.integers(0, 5000, n))
    x, y, p = rng.integers(0, 1280, n), rng.integers(0, 8, n), rng.integers(0, 2, n)
    o = E.R.readout_order(x, y, p, t)
    x, y, p, t = x[o], y[o], p[o], t[o]
    w = E.encode_evt21(x, y, p, t)
    rec, info = E.decode(E.EVT21, w, E.fresh_state(), 123)
    assert rec.tobytes() == make_events(x, y, t + 123, p).tobytes()
    assert info["events"] == n and info["untimed"] == 0


def test_slice_at_hand_derived():
    sec = [10, 10, 11, 11, 10, 12, 12, 20]
    nsec = [0, 500, 0, 1, 900, 0, 5, 0]
    bounds = [(10, 500), (11, 0), (11, 0), (12, 5), (30, 0)]
    cuts, windows, tail = SA.slice_at(sec, nsec, bounds)
    # event 1 lies ON the first boundary and closes window 0; event 2 on the duplicated one closes windows 1 and 2 (2 is
    # empty); event 4 steps back and stays in the open window; event 6 on (12, 5) closes window 3; event 7 is in front of
    # (30, 0): it stays in the open window 4
    assert cuts == [1, 2, 2, 6] and windows == [[0], [1], [], [2, 3, 4, 5]] and tail == [6, 7]
    s = SA.SlicerAt()
    cuts, info = s.push(sec, nsec, bounds)
    assert info == dict(closed=4, first_window=0, count=4, open_events=2, first=(10, 500), last=(12, 5))
    # events behind the last given boundary are no failure: they wait in the open window for newer boundaries
    cuts, info = s.push([31, 40], [0, 0], bounds[4:])
    assert cuts == [0] and info["count"] == 5 and info["open_events"] == 2
    assert s.flush() == dict(closed=1, first_window=5, count=6, open_events=0)
    with pytest.raises(ValueError):
        SA.SlicerAt().push([1], [0], [(2, 0), (1, 999999999)])
    assert SA.SlicerAt().push([1, 2], [0, 0], [])[0] == []


def test_slice_at_is_associative_at_every_cut():
    rng = np.random.default_rng(9)
    n = 80
    t = np.sort(rng.integers(0, 4_000_000_000, n)) + 5_000_000_000
    t[rng.integers(1, n, 6)] -= 300_000_000  # back-steps
    sec, nsec = t // 10 ** 9, t % 10 ** 9
    b = np.sort(rng.integers(4_900_000_000, 9_500_000_000, 25))
    b[7] = b[6]
    b[10] = t[20]  # an event exactly on a boundary
    b = np.sort(b)
    bounds = [(int(v // 10 ** 9), int(v % 10 ** 9)) for v in b]
    whole, wi = SA.SlicerAt().push(sec, nsec, bounds)
    assert 5 < wi["closed"] < 25
    for cut in range(n + 1):
        s = SA.SlicerAt()
        c1, i1 = s.push(sec[:cut], nsec[:cut], bounds)
        c2, i2 = s.push(sec[cut:], nsec[cut:], bounds[i1["closed"]:])
        assert c1 + [c + cut for c in c2] == whole and i2["count"] == wi["count"] and i2["open_events"] == wi["open_events"], cut
