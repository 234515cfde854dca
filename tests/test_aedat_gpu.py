"""GPU: esvio_fe_decode_aedat, esvio_fe_aedat_side, esvio_fe_track_aedat and esvio_fe_feed_push_aedat against the
sequential reading tests/aedat_ref.py.  Integers only: every byte of every record and every info field are compared for
equality (the IMU samples' doubles bit for bit), with guard bytes behind dst_cap records.  T = the chain's tile."""
import ctypes as C
import struct

import numpy as np
import pytest

import aedat_ref as A
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times, make_events
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def tile():
    return FE.load_library().esvio_fe_aedat_tile_events()


def records(x, y, p, ts, valid=None):
    """n polarity records as one byte string"""
    x, y, p, ts = (np.asarray(a, np.int64) for a in (x, y, p, ts))
    v = np.ones(len(x), np.int64) if valid is None else np.asarray(valid, np.int64)
    r = np.zeros((len(x), 2), "<u4")
    r[:, 0] = v | p << 1 | y << 2 | x << 17
    r[:, 1] = ts & 0xFFFFFFFF
    return r.tobytes()


def packets(rec, per, overflow=0, capacity_extra=0):
    """the records cut into polarity packets of `per` events"""
    n = len(rec) // 8
    return b"".join(A.packet(A.POLARITY, [rec[8 * i:8 * min(i + per, n)]], overflow, number=min(per, n - i),
                             capacity=min(per, n - i) + capacity_extra) for i in range(0, n, per))


def random_records(n, rng, invalid_one_in=0, t0=1000):
    ts = t0 + np.sort(rng.integers(0, 50_000, n))
    valid = None if not invalid_one_in else (rng.integers(0, invalid_one_in, n) != 0)
    return records(rng.integers(0, 346, n), rng.integers(0, 260, n), rng.integers(0, 2, n), ts, valid)


class Ae:
    """a handle and the reading's walkers of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.hip = C.CDLL("libamdhip64.so")
        self.fresh()

    def fresh(self):
        self.ft.decode_reset()
        self.ev = [A.Walker("events"), A.Walker("events")]
        self.side = [A.Walker("side"), A.Walker("side")]

    def close(self):
        self.ft.close()

    def call(self, data, cam=0, off=0, flags=0, dst_cap=None, dst_space=FE.HOST):
        """one esvio_fe_decode_aedat call -> (rc, the dst_cap records as bytes, AedatInfo); the reading does not move"""
        buf = np.frombuffer(data, np.uint8)
        if dst_cap is None:
            dst_cap = len(data) // 8 + 1
        info = FE.AedatInfo(first_t_us=-77, last_t_us=-78)
        back = np.full(16 * (dst_cap + 2), GUARD, np.uint8)
        ddst = None
        if dst_space == FE.DEVICE:
            ddst = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, len(back), C.byref(ddst)) == 0
            assert self.L.esvio_fe_mem_upload(ddst, C.c_void_p(back.ctypes.data), len(back)) == 0
            dst = ddst
        else:
            dst = C.c_void_p(back.ctypes.data)
        rc = self.L.esvio_fe_decode_aedat(self.h, cam, FE._p(buf) if len(buf) else None, len(buf), off, flags, dst, dst_cap, dst_space,
                                          C.byref(info))
        if ddst is not None:
            assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(len(back)), 2) == 0
            self.L.esvio_fe_mem_free(FE.DEVICE, ddst)
        assert (back[16 * dst_cap:] == GUARD).all(), "bytes beyond dst_cap records touched"
        return rc, back[:16 * dst_cap], info

    def check(self, data, cam=0, off=0, flags=0, dst_space=FE.HOST, tag=None, exact_cap=False):
        """a call that succeeds equals the reading, which advances with it -> (records, the reading's result)"""
        w, o = self.ev[cam].feed(data, off, flags)
        want = A.events_array(o["events"])
        rc, got, info = self.call(data, cam, off, flags, len(want) if exact_cap else None, dst_space)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        self.ev[cam] = w
        assert (info.events, info.invalid, info.bad, info.polarity_packets, info.other_packets) == \
            (len(want), o["invalid"], 0, o["polarity_packets"], o["other_packets"]), tag
        if len(want):
            assert (info.first_t_us, info.last_t_us) == (o["ticks"][0] // 1000, o["ticks"][-1] // 1000), tag
        else:
            assert (info.first_t_us, info.last_t_us) == (-77, -78), (tag, "untouched if none")
        n = len(want)
        if got[:16 * n].tobytes() != want.tobytes():
            g = got[:16 * n].view(EVENT_DTYPE)
            i = int(np.flatnonzero((g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16)).any(axis=1))[0])
            raise AssertionError((tag, "first differing record", i, g[i], want[i], n))
        return want, o

    def side_check(self, data, cam=0, off=0, flags=0, tag=None):
        w, o = self.side[cam].feed(data, off, flags)
        imu, trig, info = self.ft.aedat_side(cam, data, off, flags, imu_cap=len(o["imu"]), trig_cap=len(o["triggers"]))
        self.side[cam] = w
        assert imu.tobytes() == A.imu_array(o["imu"]).tobytes(), tag
        assert trig.tobytes() == A.trigger_array(o["triggers"]).tobytes(), tag
        for k, name in (("resets", "resets"), ("other_specials", "other_specials"), ("invalid", "invalid"), ("special_packets", "special_packets"),
                        ("imu_packets", "imu_packets"), ("other_packets", "other_packets")):
            assert getattr(info, k) == o[name], (tag, k)
        assert (info.imu, info.triggers, info.bad) == (len(o["imu"]), len(o["triggers"]), 0)
        return o


@pytest.fixture(scope="module")
def ae():
    d = Ae()
    yield d
    d.close()


def mixed_stream(n, per, rng, invalid_one_in=5):
    """n polarity events in packets of `per` with specials, IMU6 samples, a type-2 packet and padding between them"""
    rec = random_records(n, rng, invalid_one_in)
    out, k = [], 0
    for i in range(0, n, per):
        out.append(A.packet(A.POLARITY, [rec[8 * i:8 * min(i + per, n)]], 0, number=min(per, n - i), capacity=min(per, n - i) + (k % 3)))
        if k % 2 == 0:
            out.append(A.packet(A.IMU6, [A.imu6(1000 + 7 * k + j, rng.normal(0, 1, 3), rng.normal(0, 90, 3), valid=int(j != 2)) for j in range(3)]))
        if k % 3 == 0:
            out.append(A.packet(A.SPECIAL, [A.special(t, 1001 + k, valid=int(t != 5)) for t in (1, 2, 3, 4, 5, 9)], capacity=8))
        if k % 4 == 1:
            out.append(A.packet(A.FRAME, [bytes(rng.integers(0, 256, 52, dtype=np.uint8))], size=52, capacity=2))
        k += 1
    return b"".join(out)


# ---- tile edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", ["one packet", 1, 7, "T-1"])
def test_lengths_around_the_tile(ae, per):
    T = tile()
    rng = np.random.default_rng(11)
    for i, n in enumerate((T - 1, T, T + 1, 2 * T + 1)):
        ae.fresh()
        rec = random_records(n, rng, invalid_one_in=4 if i % 2 else 0)
        k = n if per == "one packet" else T - 1 if per == "T-1" else per
        want, o = ae.check(packets(rec, k), dst_space=(FE.HOST, FE.DEVICE)[i % 2], tag=(per, n), exact_cap=i == 3)
        assert o["polarity_packets"] == -(-n // k) and (len(want) == n) == (i % 2 == 0)


def test_a_packet_edge_on_a_tile_edge_and_one_event_to_either_side(ae):
    T = tile()
    rng = np.random.default_rng(12)
    for first in (T - 1, T, T + 1):
        ae.fresh()
        a, b = random_records(first, rng, 6), random_records(T + 3, rng, 6, t0=900)
        data = packets(a, first, overflow=0) + packets(b, T + 3, overflow=1)
        want, o = ae.check(data, tag=first)
        assert o["invalid"] > 0 and len(want) + o["invalid"] == first + T + 3


def test_specials_imu_a_type_2_packet_and_padding_interleaved(ae):
    T = tile()
    rng = np.random.default_rng(13)
    ae.fresh()
    data = mixed_stream(2 * T + 50, 300, rng)
    want, o = ae.check(data, tag="mixed")
    assert o["other_packets"] > 0 and o["invalid"] > 0 and len(want) > T
    s = ae.side_check(data, tag="mixed")
    assert len(s["imu"]) > 0 and len(s["triggers"]) > 0 and s["resets"] > 0 and s["invalid"] > 0


def test_event_number_zero_and_an_all_invalid_packet(ae):
    rng = np.random.default_rng(14)
    ae.fresh()
    empty = A.packet(A.POLARITY, [], capacity=4)  # eventNumber 0: 32 bytes of padding
    dead = packets(records([1, 2, 3], [4, 5, 6], [0, 1, 0], [10, 11, 12], [0, 0, 0]), 3)
    live = packets(random_records(5, rng), 5)
    want, o = ae.check(empty, tag="eventNumber 0")
    assert len(want) == 0 and o["polarity_packets"] == 1
    want, o = ae.check(dead, tag="all invalid")
    assert len(want) == 0 and o["invalid"] == 3
    want, o = ae.check(empty + dead + live + dead + empty, tag="around live events")
    assert len(want) == 5 and o["invalid"] == 6
    want, o = ae.check(dead, flags=A.KEEP_INVALID, tag="all invalid, kept")
    assert len(want) == 3 and o["invalid"] == 0
    rc, _, info = ae.call(b"")
    assert rc == 0 and (info.events, info.first_t_us) == (0, -77)


# ---- run lookup ----------------------------------------------------------------------------------------------------------
def test_overflow_changes_between_three_event_packets_inside_one_tile(ae):
    rng = np.random.default_rng(15)
    ae.fresh()
    n = 3 * 40
    rec = random_records(n, rng, 7)
    data = b"".join(packets(rec[24 * k:24 * (k + 1)], 3, overflow=k % 3) for k in range(40))
    want, o = ae.check(data, off=123_456_789, tag="0 -> 1 -> 2")
    assert sorted(set(int(s) // 2147 for s in want["sec"])) == [0, 1, 2]  # 2^31 us = 2147.48 s per overflow step
    want, o = ae.check(data, flags=A.KEEP_INVALID, dst_space=FE.DEVICE, tag="kept")
    assert len(want) == n


# ---- cuts ----------------------------------------------------------------------------------------------------------------
def test_the_small_stream_at_every_byte_cut_in_two_calls(ae):
    s = A.small_stream()
    whole = A.events_array(A.decode(s, 5_000_000_123)["events"])
    ae.fresh()
    one, _ = ae.check(s, off=5_000_000_123, tag="one call")
    assert one.tobytes() == whole.tobytes() and len(whole) == 11
    for cut in range(len(s) + 1):
        ae.fresh()
        a, oa = ae.check(s[:cut], off=5_000_000_123, tag=(cut, "first"))
        b, ob = ae.check(s[cut:], off=5_000_000_123, tag=(cut, "second"), dst_space=FE.DEVICE if cut % 7 == 0 else FE.HOST)
        assert a.tobytes() + b.tobytes() == whole.tobytes(), cut
        assert oa["polarity_packets"] + ob["polarity_packets"] == 3 and oa["invalid"] + ob["invalid"] == 1


def test_a_three_tile_stream_at_64_seeded_multi_cuts(ae):
    T = tile()
    rng = np.random.default_rng(16)
    data = mixed_stream(3 * T, 500, rng)
    whole, info = A.decode_fast(data, 77)
    ae.fresh()
    rc, got, gi = ae.call(data, off=77)
    assert rc == 0 and got[:16 * len(whole)].tobytes() == whole.tobytes() and gi.events == len(whole) and gi.invalid == info["invalid"]
    for it in range(64):
        ae.fresh()
        cuts = sorted(rng.integers(0, len(data) + 1, int(rng.integers(1, 6))).tolist())
        parts, n_inv, n_pp = [], 0, 0
        for lo, hi in zip([0] + cuts, cuts + [len(data)]):
            rc, got, gi = ae.call(data[lo:hi], off=77, dst_space=FE.DEVICE if it % 2 else FE.HOST)
            assert rc == 0, (cuts, ae.L.esvio_fe_last_error(ae.h))
            parts.append(got[:16 * gi.events].tobytes())
            n_inv, n_pp = n_inv + gi.invalid, n_pp + gi.polarity_packets
        assert b"".join(parts) == whole.tobytes(), cuts
        assert (n_inv, n_pp) == (info["invalid"], info["polarity_packets"]), cuts


# ---- flags ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_space", [FE.HOST, FE.DEVICE])
def test_drop_against_keep_invalid(ae, dst_space):
    T = tile()
    rng = np.random.default_rng(17)
    data = packets(random_records(T + 200, rng, invalid_one_in=5), 257)
    ae.fresh()
    dropped, od = ae.check(data, dst_space=dst_space, tag="drop")
    ae.fresh()
    kept, ok = ae.check(data, flags=A.KEEP_INVALID, dst_space=dst_space, tag="keep")
    assert len(kept) == T + 200 and od["invalid"] == T + 200 - len(dropped) and 100 < od["invalid"] < 400 and ok["invalid"] == 0


# ---- failures ------------------------------------------------------------------------------------------------------------
def test_every_bad_cause_counts_exactly_and_leaves_the_state(ae):
    T = tile()
    rng = np.random.default_rng(18)
    n = T + 30
    good = random_records(n, rng)
    r = np.frombuffer(good, "<u4").reshape(n, 2).copy()
    r[[3, T - 1, T, n - 1], 1] = 0x80000000 | 5  # ts < 0, on both sides of the tile edge
    r[9, 0] &= ~np.uint32(1)                       # an invalid event with ts < 0: dropped, never BAD
    r[9, 1] = 0xFFFFFFFF
    lead_full = packets(random_records(10, rng), 10)
    lead, tail = lead_full[:-3], lead_full[-3:]    # a record cut by the chunk's end waits in the state
    t20 = int(np.frombuffer(good, "<u4").reshape(n, 2)[20, 1])
    cases = [("ts < 0", packets(r.tobytes(), 400), 0, 4),
             ("overflow < 0", packets(good, 400, overflow=-1), 0, n),
             ("ticks < 0", packets(good, 400), -(t20 * 1000 + 1), None),
             ("sec >= 2^32", packets(good, 400, overflow=2000), 2 ** 62, n + 1),
             ("ts64 >= 2^53", packets(good, 400, overflow=1 << 22), -(2 ** 62), n + 1)]
    for name, data, off, bad in cases:
        ae.fresh()
        ae.check(lead, tag="lead")
        for flags in (0, A.KEEP_INVALID):
            with pytest.raises(A.Bad) as e:
                ae.ev[0].feed(tail + data, off, flags)
            if bad is not None:
                assert e.value.bad == bad + (1 if flags and name == "ts < 0" else 0), name
            assert 0 < e.value.bad <= n + 1
            rc, _, info = ae.call(tail + data, off=off, flags=flags, dst_space=FE.DEVICE if flags else FE.HOST)
            assert rc == -1 and info.bad == e.value.bad, (name, flags, info.bad, e.value.bad)
        # the fault removed: what a run that never failed gives, the waiting record included
        want, _ = ae.check(tail + packets(good, 400), off=0, tag=(name, "after the failure"))
        assert len(want) == n + 1


def test_dst_cap_one_too_small_reports_the_count_and_stores_nothing(ae):
    T = tile()
    rng = np.random.default_rng(19)
    data = packets(random_records(T + 77, rng, invalid_one_in=5), 300)
    need = len(A.decode(data)["events"])
    for dst_space in (FE.HOST, FE.DEVICE):
        for flags, k in ((0, need), (A.KEEP_INVALID, T + 77)):
            ae.fresh()
            rc, got, info = ae.call(data, dst_cap=k - 1, dst_space=dst_space, flags=flags)
            assert rc == -1 and info.events == k and info.bad == 0
            if dst_space == FE.DEVICE:
                assert (got == GUARD).all()  # the emit stores nothing
            ae.check(data, dst_space=dst_space, flags=flags, exact_cap=True, tag="exact room")


def test_a_malformed_header_in_the_second_of_three_packets(ae):
    rng = np.random.default_rng(20)
    p = [packets(random_records(50, rng), 50) for _ in range(3)]
    for field, value in ((4, 0), (16, -1), (20, 51), (8, 0), (4, 12)):  # eventSize, eventCapacity, eventNumber, eventTSOffset
        broken = bytearray(p[1])
        struct.pack_into("<i", broken, field, value)
        ae.fresh()
        ae.check(p[0][:100], tag="lead")
        rc, got, info = ae.call(p[0][100:] + bytes(broken) + p[2])
        assert rc == -1 and info.events == 0 and (got == GUARD).all(), (field, value)
        assert b"malformed" in ae.L.esvio_fe_last_error(ae.h)
        want, _ = ae.check(p[0][100:] + p[1] + p[2], tag="the header mended")
        assert len(want) == 141  # (28 header bytes and 9 records went with the lead)
    ae.fresh()
    L, h = ae.L, ae.h
    info, buf = FE.AedatInfo(), np.frombuffer(p[0], np.uint8)
    dst = np.zeros(64, EVENT_DTYPE)
    args = lambda **k: [k.get("cam", 0), FE._p(buf), len(buf), k.get("off", 0), k.get("flags", 0), k.get("dst", FE._p(dst)), 64,
                        k.get("space", FE.HOST), C.byref(info)]
    for bad in (dict(cam=2), dict(off=2 ** 62 + 1), dict(flags=2), dict(dst=None), dict(space=7), dict(dst=C.c_void_p(dst.ctypes.data + 8), space=FE.DEVICE)):
        assert L.esvio_fe_decode_aedat(h, *args(**bad)) == -1, bad
    assert L.esvio_fe_decode_aedat(h, 0, None, 8, 0, 0, FE._p(dst), 64, FE.HOST, C.byref(info)) == -1
    ae.check(p[0], tag="after the argument errors")


# ---- the side call -------------------------------------------------------------------------------------------------------
def test_side_call_samples_triggers_resets_in_either_order_with_the_event_call(ae):
    rng = np.random.default_rng(21)
    data = mixed_stream(700, 90, rng)
    off = 1_700_000_000_123_456_789
    whole_e, whole_s = A.decode(data, off), A.decode(data, off, mode="side")
    cuts = [0, 333, 334, 1000, 2222, 5000, len(data)]
    for order in ("events first", "side first"):
        ae.fresh()
        ev, imu, trig = [], [], []
        for lo, hi in zip(cuts, cuts[1:]):
            for which in (("e", "s") if order == "events first" else ("s", "e")):
                if which == "e":
                    ev.append(ae.check(data[lo:hi], off=off, tag=(order, lo))[0])
                else:
                    o = ae.side_check(data[lo:hi], off=off, tag=(order, lo))
                    imu += o["imu"]
                    trig += o["triggers"]
        assert b"".join(e.tobytes() for e in ev) == A.events_array(whole_e["events"]).tobytes()  # (tobytes: the padding too)
        assert imu == whole_s["imu"] and trig == whole_s["triggers"] and len(imu) > 5 and len(trig) > 5
    # a capacity one too small, a BAD sample: the numbers come back, the state stays
    ae.fresh()
    with pytest.raises(FE.FrontendError) as e:
        ae.ft.aedat_side(0, data, off, imu_cap=len(whole_s["imu"]) - 1, trig_cap=len(whole_s["triggers"]))
    assert (e.value.info.imu, e.value.info.triggers) == (len(whole_s["imu"]), len(whole_s["triggers"]))
    with pytest.raises(FE.FrontendError) as e:
        ae.ft.aedat_side(0, data, -(2 ** 62))
    assert e.value.info.bad == len(whole_s["imu"]) + len(whole_s["triggers"])
    ae.side_check(data, off=off, tag="after the failures")


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H = 346, 260


@pytest.fixture(scope="module")
def frames():
    """4 frames of a scene stream at the DAVIS346's size, each camera's batch as polarity packets of 4096 events with an
    IMU6 packet behind every packet that crosses a millisecond: per frame the records, the bytes, and the byte offset
    behind each event (stamps relative to `base`, which travels as t_offset_ns)"""
    st = SceneStream(W=W, H=H, rate=1e6, seed=7)
    base = st.t_us - 1000
    rng = np.random.default_rng(3)
    out = []
    for _ in range(4):
        left, right, _ = st.next_batch()
        fr = dict(rec=[], data=[], ends=[])
        for ev in (left, right):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
            rec = records(x, y, p, t - base)
            parts, ends, pos = [], [], 0
            for i in range(0, len(t), 4096):
                j = min(i + 4096, len(t))
                parts.append(A.packet(A.POLARITY, [rec[8 * i:8 * j]], number=j - i, capacity=4096))
                ends.append(pos + 28 + 8 * np.arange(1, j - i + 1))
                pos += len(parts[-1])
                for ms in range(int(t[i] - base) // 1000, int(t[j - 1] - base) // 1000 + 1):
                    parts.append(A.packet(A.IMU6, [A.imu6(ms * 1000, rng.normal(0, 1, 3), rng.normal(0, 50, 3))]))
                    pos += len(parts[-1])
            fr["rec"].append(make_events(x, y, t, p))
            fr["data"].append(b"".join(parts))
            fr["ends"].append(np.concatenate(ends))
        out.append(fr)
    # the loop's records are the generator's
    ev, _ = A.decode_fast(out[0]["data"][0], base * 1000)
    assert ev.tobytes() == out[0]["rec"][0].tobytes()
    return base, out


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def make_tracker(max_cnt=150):
    return FE.FeatureTracker(FE.make_config(W, H, max_cnt=max_cnt))


@pytest.mark.parametrize("how", ["plain", "filter", "motion"])
def test_track_aedat_equals_track_event_on_the_loops_records(frames, how):
    base, frs = frames
    a, b = make_tracker(), make_tracker()
    prm = FE.FilterParams(5_000_000, 1, 200_000) if how == "filter" else None
    try:
        for i, fr in enumerate(frs):
            pub = i % 2 == 0 or how != "plain"
            L, Rr = fr["rec"]
            t1 = float(event_times(L[-1:])[0])
            m = FE.make_motion(t1, (0.4, -0.2, 0.1), (0.1, 0.0, 0.0), (6.0, 2.0, -1.0), (0.3, -0.5, 0.2), 0.9 * W, 0.9 * W, W / 2.0, H / 2.0) \
                if how == "motion" else None
            if how == "filter":
                ia = a.track_batch(L, Rr, pub=pub, params=prm)
            else:
                a.trackEvent(t1, L, Rr, pub, measurements=m)
            info, ae2 = b.track_aedat(fr["data"][0], fr["data"][1], base * 1000, 0, pub, params=prm, measurements=m)
            assert info.tracked == 1 and (ae2[0].events, ae2[1].events) == (len(L), len(Rr)) and ae2[0].bad == ae2[0].invalid == 0
            if how == "filter":
                assert (ia.kept[0], ia.kept[1], ia.rejected[0], ia.cur_time) == (info.kept[0], info.kept[1], info.rejected[0], info.cur_time)
                assert 0 < info.kept[0] < len(L)
            else:
                assert (info.kept[0], info.kept[1], info.cur_time) == (len(L), len(Rr), t1)
            # a decode and a side call between two track calls change no later result
            rec, di = b.decode_aedat(1, fr["data"][0], base * 1000)
            assert rec.tobytes() == L.tobytes()
            imu, _, si = b.aedat_side(0, fr["data"][0], base * 1000)
            assert len(imu) == si.imu_packets > 0
            assert results(a) == results(b), (how, i)
        assert len(a.ids) > 0 and len(a.ids_right) > 0
    finally:
        a.close()
        b.close()


def test_track_aedat_failures_move_no_state_and_are_refused_while_announced(frames):
    base, frs = frames
    ft = make_tracker()
    try:
        L, Rr = frs[0]["rec"]
        dl, dr = FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(Rr, FE.DEVICE)
        ft.set_next_batch(float(event_times(L[-1:])[0]), dl.arg, dr.arg, True)
        with pytest.raises(FE.FrontendError, match="announced"):
            ft.track_aedat(frs[0]["data"][0], frs[0]["data"][1], base * 1000)
        ft.trackEvent(float(event_times(L[-1:])[0]), dl.arg, dr.arg, True)
        dl.free()
        dr.free()
        with pytest.raises(FE.FrontendError) as e:  # BAD in the right camera: both cameras' states stay
            ft.track_aedat(frs[1]["data"][0][:5000], frs[1]["data"][1], -(2 ** 62))
        assert e.value.info.bad[0] > 0 and e.value.info.bad[1] == len(frs[1]["rec"][1])
        rec, _ = ft.decode_aedat(0, frs[1]["data"][0], base * 1000)
        assert rec.tobytes() == frs[1]["rec"][0].tobytes()
    finally:
        ft.close()


def test_a_feed_fed_4099_byte_chunks_equals_the_feed_fed_the_loops_records(frames):
    base, frs = frames
    a, b = make_tracker(40), make_tracker(40)
    try:
        a.feed_open(200.0)
        b.feed_open(200.0)
        tracked = 0
        for fr in frs[:3]:
            for cam in range(2):
                data, ends, rec = fr["data"][cam], fr["ends"][cam], fr["rec"][cam]
                for lo in range(0, len(data), 4099):
                    hi = min(lo + 4099, len(data))
                    r0, r1 = int(np.searchsorted(ends, lo, "right")), int(np.searchsorted(ends, hi, "right"))  # records that end in (lo, hi]
                    ia = a.feed_push_aedat(cam, data[lo:hi], base * 1000)
                    ib = b.feed_push_events(cam, rec[r0:r1])
                    assert (ia.appended, ia.closed, ia.queued, ia.bad) == (ib.appended, ib.closed, ib.queued, 0) and ia.appended == r1 - r0
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
        with pytest.raises(FE.FrontendError) as e:  # a malformed header: nothing appended
            a.feed_push_aedat(0, A.HEADER.pack(1, 1, 8, 4, 0, 1, 2, 0))
        assert e.value.info.appended == 0
    finally:
        a.close()
        b.close()


def test_reserve_covers_the_scratch_and_a_second_call_allocates_nothing(frames):
    base, frs = frames
    ft = make_tracker()
    L, h = ft._hd.L, ft._hd.h
    try:
        n = max(len(fr["rec"][c]) for fr in frs for c in range(2))
        ft.decode_aedat(0, frs[0]["data"][0][:3000], base * 1000)  # a handle that has decoded AEDAT before
        ft.decode_reset()
        ft._hd.check(L.esvio_fe_reserve(h, n, n, 0))
        dst = FE.EventBuffer(np.zeros(n, EVENT_DTYPE), FE.DEVICE)
        a0, mem0 = ft.latency_stats()["allocs"], ft.device_memory()[0]
        for cam in range(2):
            for fr in frs[:2]:
                buf, info = np.frombuffer(fr["data"][cam], np.uint8), FE.AedatInfo()
                assert L.esvio_fe_decode_aedat(h, cam, FE._p(buf), len(buf), base * 1000, 0, C.c_void_p(dst.arg[0]), n, FE.DEVICE, C.byref(info)) == 0
                assert info.events == len(fr["rec"][cam])
        assert ft.latency_stats()["allocs"] == a0 and ft.device_memory()[0] == mem0
        dst.free()
        # a host dst's records grow on first use; the second call of the size allocates nothing
        ft.decode_reset()
        ft.decode_aedat(0, frs[0]["data"][0], base * 1000)
        mem0 = ft.device_memory()[0]
        ft.decode_reset()
        ft.decode_aedat(0, frs[0]["data"][0], base * 1000)
        assert ft.device_memory()[0] == mem0
    finally:
        ft.close()
