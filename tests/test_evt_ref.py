"""CPU: the raw-stream rule of include/esvio_fe.h as tests/evt_ref.py reads it — hand-derived known answers, the words
written out in hex with the events they stand for; the rule composes over a cut at any word; the test-side encoders
round-trip a scene batch."""

import numpy as np

import evt_ref as R
from esvio_amd.events import make_events
from esvio_amd.synth import SceneStream


def ev3(words, state=None, off=0):
    s = R.fresh_state() if state is None else state
    rec, info = R.decode_evt3(np.array(words, "<u2"), s, off)
    return rec, info, s


def ev2(words, state=None, off=0):
    s = R.fresh_state() if state is None else state
    rec, info = R.decode_evt2(np.array(words, "<u4"), s, off)
    return rec, info, s


def tuples(rec):
    return [(int(e["x"]), int(e["y"]), int(e["polarity"]), int(e["sec"]) * 10 ** 6 + int(e["nsec"]) // 1000) for e in rec]


def test_addr_x_before_and_after_the_first_time_high():
    # ADDR_X x=5 p=0 (untimed) | TIME_HIGH 1 | ADDR_X x=5 p=1
    rec, info, s = ev3([0x2005, 0x8001, 0x2805])
    assert tuples(rec) == [(5, 0, 1, 4096)]
    assert (info["events"], info["untimed"], info["other"], info["bad"], info["wraps"]) == (1, 1, 0, 0, 0)
    assert info["first_t_us"] == info["last_t_us"] == 4096 and s["seen"] == 1


def test_time_high_fff_to_000_is_a_wrap():
    rec, info, s = ev3([0x8FFF, 0x2001, 0x8000, 0x2002])
    assert tuples(rec) == [(1, 0, 0, 0xFFF * 4096), (2, 0, 0, 1 << 24)]
    assert info["wraps"] == 1 and s["wraps"] == 1 and s["th"] == 0


def test_small_back_step_is_no_wrap():
    rec, info, _ = ev3([0x8010, 0x2001, 0x800F, 0x2001])
    assert tuples(rec) == [(1, 0, 0, 0x10 * 4096), (1, 0, 0, 0xF * 4096)] and info["wraps"] == 0
    assert info["first_t_us"] == 65536 and info["last_t_us"] == 61440  # time goes back


def test_exactly_2048_wraps_and_2047_does_not():
    rec, info, _ = ev3([0x8800, 0x8000, 0x2003])  # 2048 -> 0
    assert info["wraps"] == 1 and tuples(rec) == [(3, 0, 0, 1 << 24)]
    rec, info, _ = ev3([0x87FF, 0x8000, 0x2003])  # 2047 -> 0
    assert info["wraps"] == 0 and tuples(rec) == [(3, 0, 0, 0)]


def test_time_high_keeps_time_low():
    rec, _, s = ev3([0x8001, 0x6123, 0x8002, 0x2000])
    assert tuples(rec) == [(0, 0, 0, 2 * 4096 + 0x123)] and s["tl"] == 0x123


def test_vectors_run_past_2047_unmasked_and_bx_wraps_mod_65536():
    # TIME_HIGH 1 | ADDR_Y 7 | VECT_BASE_X x=2040 p=0 | VECT_12 all | VECT_12 all | VECT_8 all
    rec, info, s = ev3([0x8001, 0x0007, 0x37F8, 0x4FFF, 0x4FFF, 0x50FF])
    assert tuples(rec) == [(x, 7, 0, 4096) for x in range(2040, 2072)] and s["bx"] == 2072
    # ... 5291 empty VECT_12 later bx = 2040 + 12 * 5291 = 65532: a full VECT_12 gives x = 65532..65535, 0..7
    rec, info, s = ev3([0x8001, 0x37F8] + [0x4000] * 5291 + [0x4FFF])
    assert [t[0] for t in tuples(rec)] == [65532, 65533, 65534, 65535, 0, 1, 2, 3, 4, 5, 6, 7] and s["bx"] == 8
    # a mask with holes: ascending i, only the set bits
    rec, _, _ = ev3([0x8001, 0x3010, 0x4A05])  # base 16, bits 0, 2, 9, 11
    assert [t[0] for t in tuples(rec)] == [16, 18, 25, 27]


def test_a_vectors_polarity_is_the_base_words():
    rec, _, s = ev3([0x8000, 0x0003, 0x3805, 0x4001, 0x3005, 0x5001])
    assert tuples(rec) == [(5, 3, 1, 0), (5, 3, 0, 0)] and s["bp"] == 0


def test_addr_y_ignores_bit_11_and_other_types_are_counted():
    rec, info, s = ev3([0x8000, 0x0805, 0x2001, 0x1000, 0x7000, 0x9000, 0xA123, 0xE000, 0xF000])
    assert tuples(rec) == [(1, 5, 0, 0)] and info["other"] == 6 and s["y"] == 5


def test_a_negative_offset_makes_a_bad_event():
    rec, info, _ = ev3([0x8000, 0x2001, 0x6005, 0x2001], off=-1)
    assert info["events"] == 2 and info["bad"] == 1 and info["first_t_us"] == -1 and info["last_t_us"] == 4
    _, info, _ = ev3([0x8000, 0x2001], off=(1 << 32) * 10 ** 6)
    assert info["bad"] == 1
    _, info, _ = ev3([0x8000, 0x2001], off=(1 << 32) * 10 ** 6 - 1)
    assert info["bad"] == 0


def test_evt2_bit_fields_and_its_wrap():
    cd_on = (1 << 28) | (5 << 22) | (100 << 11) | 200   # CD_ON, t low 5, x 100, y 200
    cd_off = (0 << 28) | (63 << 22) | (2047 << 11) | 2047
    rec, info, s = ev2([cd_on, 0x80000001, cd_on, cd_off, 0x70000000, 0xA0000000])
    assert tuples(rec) == [(100, 200, 1, 64 + 5), (2047, 2047, 0, 64 + 63)]
    assert (info["untimed"], info["other"], info["wraps"]) == (1, 2, 0)
    rec, info, _ = ev2([0x88000000, 0x80000000, cd_on])  # 2^27 -> 0: a wrap
    assert info["wraps"] == 1 and tuples(rec) == [(100, 200, 1, (1 << 34) + 5)]
    rec, info, _ = ev2([0x87FFFFFF, 0x80000000, cd_on])  # 2^27 - 1 -> 0: a back-step
    assert info["wraps"] == 0 and tuples(rec) == [(100, 200, 1, 5)]


def random_evt3(rng, n):
    """adversarial words: every type, small time-high ranges (back-steps and wraps both occur)"""
    typ = rng.choice([0x0, 0x2, 0x3, 0x4, 0x5, 0x6, 0x8, 0x8, 0xA, 0xE], n)
    w = (typ << 12) | rng.integers(0, 4096, n)
    th = typ == 0x8
    w[th] = 0x8000 | rng.choice([0, 1, 2, 2047, 2048, 2049, 4094, 4095], int(th.sum()))
    return w.astype("<u2")


def test_the_rule_composes_over_a_cut_at_any_word():
    rng = np.random.default_rng(3)
    for trial in range(40):
        w = random_evt3(rng, int(rng.integers(3, 120)))
        if trial % 2:
            w[:3] = [0x0001, 0x6001, 0x3001]  # (no TIME_HIGH for a while: untimed events)
        s0 = R.fresh_state()
        whole, iw = R.decode_evt3(w, s0)
        cut = int(rng.integers(0, len(w) + 1))
        s1 = R.fresh_state()
        a, ia = R.decode_evt3(w[:cut], s1)
        b, ib = R.decode_evt3(w[cut:], s1)
        assert a.tobytes() + b.tobytes() == whole.tobytes() and s1 == s0
        for k in ("events", "untimed", "other"):
            assert ia[k] + ib[k] == iw[k]


def scene_batch(W=346, H=260, rate=1e6):
    st = SceneStream(W=W, H=H, rate=rate, seed=5)
    left, _, _ = st.next_batch()
    t = left["sec"].astype(np.int64) * 10 ** 6 + left["nsec"].astype(np.int64) // 1000
    return left["x"].astype(np.int64), left["y"].astype(np.int64), left["polarity"].astype(np.int64), t


def test_encoders_round_trip_a_scene_batch():
    x, y, p, t = scene_batch()
    base = int(t[0]) - 100
    order = R.readout_order(x, y, p, t)
    for xs, ys, ps, ts in ((x, y, p, t), tuple(a[order] for a in (x, y, p, t))):
        want = make_events(xs, ys, ts, ps)
        for fmt, vect in ((R.EVT3, True), (R.EVT3, False), (R.EVT2, True)):
            w = R.encode(fmt, xs, ys, ps, ts - base, vect)
            rec, info = R.decode(fmt, w, R.fresh_state(), base)
            assert rec.tobytes() == want.tobytes(), (fmt, vect)
            assert info["events"] == len(want) and info["untimed"] == info["other"] == info["bad"] == 0
            print("format %d vect %d: %.2f bytes per event" % (fmt, vect, w.nbytes / len(want)))
    w = R.encode_evt3(*(a[order] for a in (x, y, p)), t[order] - base)
    assert ((w >> 12) == 4).any(), "the read-out order gives no vector word: the vector path is not covered"
