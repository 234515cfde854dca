"""GPU: esvio_fe_decode_bag, esvio_fe_bag_side and esvio_fe_feed_push_bag against the sequential reading
tests/bag_ref.py.  Integers only: every byte of every record, every row of the message table and every info field are
compared for equality (the IMU samples' doubles bit for bit), with guard bytes behind dst_cap records.  T = the kernel's
tile.  The decode cases run once: k_bag_emit has one form of its load."""
import ctypes as C
import struct

import numpy as np
import pytest

import bag_ref as B
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
IMAGE = "/davis/left/image_raw"


def tile():
    return FE.load_library().esvio_fe_bag_tile_events()


def rand_wire(n, rng, t0=1000):
    """n wire events with ascending stamps; polarity bytes 0, 1, 2 and 255"""
    t = t0 + np.sort(rng.integers(0, 50_000_000, n))
    return B.wire_events(rng.integers(0, 346, n), rng.integers(0, 260, n), 7 + t // 10 ** 9, t % 10 ** 9, rng.choice([0, 1, 2, 255], n))


def msg(topic, k, wire, sec=7):
    return (topic, (sec, 1000 + k), B.event_array(k, (sec, 10 * k), wire))


def body(messages, **kw):
    """a bag's bytes behind the magic"""
    return B.write_bag(messages, **kw)[13:]


class Bg:
    """a handle and the reading's two walkers, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.hip = C.CDLL("libamdhip64.so")
        self.fresh()

    def fresh(self, topics=B.TOPICS):
        self.ft.bag_set_topics(*topics)
        self.ev, self.side = B.Walker("events", topics), B.Walker("side", topics)

    def close(self):
        self.ft.close()

    def error(self):
        return self.L.esvio_fe_last_error(self.h)

    def call(self, data, dst_cap=None, msgs_cap=None, dst_space=FE.HOST, flags=0):
        """one esvio_fe_decode_bag call -> (rc, per camera the dst_cap records as bytes, the message rows written,
        BagInfo); the reading does not move"""
        buf = np.frombuffer(data, np.uint8)
        caps = [len(data) // 13 + 1] * 2 if dst_cap is None else list(dst_cap)
        msgs_cap = len(data) // 28 + 1 if msgs_cap is None else msgs_cap
        info = FE.BagInfo()
        for cam in range(2):
            info.cam[cam].first_sec, info.cam[cam].last_nsec = 0x77777777, 0x78787878
        back = [np.full(16 * (caps[cam] + 2), GUARD, np.uint8) for cam in range(2)]
        msgs = np.zeros(msgs_cap + 1, FE.BAG_MESSAGE_DTYPE)
        msgs.view(np.uint8)[:] = GUARD
        ptrs, dev = (C.c_void_p * 2)(), []
        for cam in range(2):
            if dst_space == FE.DEVICE:
                d = C.c_void_p()
                assert self.L.esvio_fe_mem_alloc(FE.DEVICE, len(back[cam]), C.byref(d)) == 0
                assert self.L.esvio_fe_mem_upload(d, C.c_void_p(back[cam].ctypes.data), len(back[cam])) == 0
                dev.append(d)
                ptrs[cam] = d.value
            else:
                ptrs[cam] = back[cam].ctypes.data
        rc = self.L.esvio_fe_decode_bag(self.h, FE._p(buf) if len(buf) else None, len(buf), flags, C.byref(ptrs), C.byref((C.c_size_t * 2)(*caps)),
                                        dst_space, FE._p(msgs), msgs_cap, C.byref(info))
        for cam, d in enumerate(dev):
            assert self.hip.hipMemcpy(C.c_void_p(back[cam].ctypes.data), d, C.c_size_t(len(back[cam])), 2) == 0
            self.L.esvio_fe_mem_free(FE.DEVICE, d)
        for cam in range(2):
            assert (back[cam][16 * caps[cam]:] == GUARD).all(), "bytes beyond dst_cap records touched"
        assert (msgs[msgs_cap:].view(np.uint8) == GUARD).all(), "rows beyond msgs_cap touched"
        return rc, [back[cam][:16 * caps[cam]] for cam in range(2)], msgs[:msgs_cap], info

    def check(self, data, dst_space=FE.HOST, tag=None, exact_cap=False):
        """a call that succeeds equals the reading, which advances with it -> the reading's result"""
        w, o = self.ev.feed(data)
        want = o["events"]
        cap = [len(want[0]), len(want[1])] if exact_cap else None
        rc, got, msgs, info = self.call(data, cap, len(o["messages"]) if exact_cap else None, dst_space)
        assert rc == 0, (tag, rc, self.error())
        self.ev = w
        for cam in range(2):
            ci, n = info.cam[cam], len(want[cam])
            assert (ci.events, ci.bad, ci.messages) == (n, 0, o["cam_messages"][cam]), (tag, cam)
            if n:
                assert (ci.first_sec, ci.first_nsec, ci.last_sec, ci.last_nsec) == \
                    (want[cam]["sec"][0], want[cam]["nsec"][0], want[cam]["sec"][-1], want[cam]["nsec"][-1]), (tag, cam)
            else:
                assert (ci.first_sec, ci.last_nsec) == (0x77777777, 0x78787878), (tag, "untouched if none")
            if got[cam][:16 * n].tobytes() != want[cam].tobytes():
                g = got[cam][:16 * n].view(EVENT_DTYPE)
                i = int(np.flatnonzero((g.view(np.uint8).reshape(-1, 16) != want[cam].view(np.uint8).reshape(-1, 16)).any(axis=1))[0])
                raise AssertionError((tag, cam, "first differing record", i, g[i], want[cam][i], n))
        assert msgs[:len(o["messages"])].tobytes() == o["messages"].tobytes(), tag
        assert (info.other_messages, info.other_records, info.chunks, info.connections) == \
            (o["other_messages"], o["other_records"], o["chunks"], o["connections"]), tag
        return o

    def side_check(self, data, tag=None):
        w, o = self.side.feed(data)
        imu, info = self.ft.bag_side(data, imu_cap=len(o["imu"]))
        self.side = w
        assert imu.tobytes() == o["imu"].tobytes(), tag
        assert (info.imu, info.bad, info.other_messages, info.other_records, info.chunks, info.connections) == \
            (len(o["imu"]), 0, o["other_messages"], o["other_records"], o["chunks"], o["connections"]), tag
        return o


@pytest.fixture(scope="module")
def bg():
    d = Bg()
    yield d
    d.close()


# ---- tile edges ----------------------------------------------------------------------------------------------------------
def test_counts_around_the_wave_and_the_tile_with_the_other_camera_at_another(bg):
    T = tile()
    rng = np.random.default_rng(31)
    counts = [0, 1, 63, 64, 65, T - 1, T, T + 1]
    for i, (nl, nr) in enumerate(zip(counts, counts[3:] + counts[:3])):
        bg.fresh()
        first, second = (msg(B.RIGHT, 1, rand_wire(nr, rng)), msg(B.LEFT, 1, rand_wire(nl, rng)))[::1 if i % 2 else -1]
        o = bg.check(body([first, second]), dst_space=(FE.HOST, FE.DEVICE)[i % 2], tag=(nl, nr), exact_cap=i % 3 == 0)
        assert [len(e) for e in o["events"]] == [nl, nr] and o["cam_messages"] == [1, 1]  # (an empty EventArray is a message)


def test_a_message_edge_on_a_tile_edge_and_one_event_to_either_side(bg):
    T = tile()
    rng = np.random.default_rng(32)
    for first in (T - 1, T, T + 1):
        bg.fresh()
        data = body([msg(B.LEFT, 1, rand_wire(first, rng)), msg(B.RIGHT, 1, rand_wire(first + 1, rng)), msg(B.LEFT, 2, rand_wire(T + 3, rng, 2000)),
                     msg(B.RIGHT, 2, rand_wire(5, rng, 2000))], per_chunk=3)
        o = bg.check(data, tag=first)
        assert o["messages"]["first"].tolist() == [0, 0, first, first + 1]


def test_right_events_before_the_first_left_ones_and_a_foreign_90_kb_message_between(bg):
    rng = np.random.default_rng(33)
    bg.fresh()
    image = B.ros_header(1, (7, 5), b"cam") + bytes(rng.integers(0, 256, 346 * 260, dtype=np.uint8))
    data = body([msg(B.RIGHT, 1, rand_wire(70, rng)), (IMAGE, (7, 2), image), msg(B.LEFT, 1, rand_wire(90, rng)), (IMAGE, (7, 3), image),
                 msg(B.RIGHT, 2, rand_wire(3, rng, 3000))], per_chunk=2)
    o = bg.check(data, dst_space=FE.DEVICE, tag="whole")
    assert o["messages"]["cam"].tolist() == [1, 0, 1] and o["other_messages"] == 2 and len(data) > 180_000
    s = bg.side_check(data)
    assert len(s["imu"]) == 0 and s["other_messages"] == 2


# ---- cuts ----------------------------------------------------------------------------------------------------------------
def joined(parts):
    return [b"".join(p[0][cam] for p in parts) for cam in range(2)], np.concatenate([p[1] for p in parts])


def test_small_bag_at_every_byte_cut_in_two_calls(bg):
    s = B.small_bag()[13:]
    whole = B.Walker("events").feed(s)[1]
    bg.fresh()
    o = bg.check(s, tag="one call")
    assert [len(e) for e in o["events"]] == [5, 4]
    for cut in range(len(s) + 1):
        bg.fresh()
        parts = []
        for k, piece in enumerate((s[:cut], s[cut:])):
            rc, got, msgs, info = bg.call(piece, dst_space=FE.DEVICE if (cut + k) % 7 == 0 else FE.HOST)
            assert rc == 0, (cut, bg.error())
            n = [info.cam[0].events, info.cam[1].events]
            parts.append(([got[cam][:16 * n[cam]].tobytes() for cam in range(2)], msgs[:info.cam[0].messages + info.cam[1].messages]))
        ev, msgs = joined(parts)
        assert ev == [whole["events"][0].tobytes(), whole["events"][1].tobytes()], cut
        assert msgs.tobytes() == whole["messages"].tobytes(), cut
    # ... and call by call against the reading at a few cuts of every kind of place
    for cut in range(0, len(s) + 1, 41):
        bg.fresh()
        bg.check(s[:cut], tag=(cut, "first"))
        bg.check(s[cut:], tag=(cut, "second"), dst_space=FE.DEVICE)


def spans(bag):
    """kind -> the (lo, hi) byte ranges of a bag (magic included) that are of that kind"""
    out = {k: [] for k in ("record header", "connection data", "message header", "event", "index record", "bag-header padding")}

    def walk(lo, hi, inside):
        pos = lo
        while pos < hi:
            hl = struct.unpack_from("<I", bag, pos)[0]
            f = B.parse_fields(bag[pos + 4:pos + 4 + hl], "header")
            dl = struct.unpack_from("<I", bag, pos + 4 + hl)[0]
            d0 = pos + 8 + hl
            op = f[b"op"][0]
            if op != 4:
                out["record header"].append((pos + 1, d0))
            if op == 3:
                out["bag-header padding"].append((d0 + 1, d0 + dl))
            elif op == 4:
                out["index record"].append((pos + 1, d0 + dl))
            elif op == 7:
                out["connection data"].append((d0 + 1, d0 + dl))
            elif op == 2 and dl >= 28 and b"cam" == bag[d0 + 16:d0 + 19]:  # (this file's event messages: frame_id "cam")
                out["message header"].append((d0 + 1, d0 + 31))
                if dl > 31:
                    out["event"].append((d0 + 32, d0 + dl))
            if op == 5:
                walk(d0, d0 + dl, True)
            pos = d0 + dl

    walk(13, len(bag), False)
    return out


def test_a_three_tile_bag_at_64_seeded_multi_cuts_each_inside_another_structure(bg):
    T = tile()
    rng = np.random.default_rng(34)
    messages, k = [], 0
    for i in range(0, 3 * T, 700):
        n = min(700, 3 * T - i)
        messages += [msg(B.LEFT, k, rand_wire(n, rng, 1000 + i)), (B.IMU, (7, k), B.imu_message(k, (7, k), (k, 1, 2), (3, 4, k))),
                     msg(B.RIGHT, k, rand_wire(n - 3, rng, 1000 + i)), (IMAGE, (7, k), B.ros_header(k, (7, k), b"img") + b"\x55" * 500)]
        k += 1
    bag = B.write_bag(messages, per_chunk=3)
    places = spans(bag)
    assert all(len(v) > 0 for v in places.values()), {k: len(v) for k, v in places.items()}
    s = bag[13:]
    whole = B.Walker("events").feed(s)[1]
    assert len(whole["events"][0]) == 3 * T
    kinds = sorted(places)
    for it in range(64):
        bg.fresh()
        chosen = rng.choice(len(kinds), int(rng.integers(1, 6)), replace=False)
        cuts = []
        for c in chosen:
            lo, hi = places[kinds[c]][int(rng.integers(0, len(places[kinds[c]])))]
            cuts.append(int(rng.integers(lo, hi)) - 13)
        cuts = sorted(cuts)
        parts = []
        for lo, hi in zip([0] + cuts, cuts + [len(s)]):
            rc, got, msgs, info = bg.call(s[lo:hi], dst_space=FE.DEVICE if it % 2 else FE.HOST)
            assert rc == 0, (cuts, bg.error())
            n = [info.cam[0].events, info.cam[1].events]
            parts.append(([got[cam][:16 * n[cam]].tobytes() for cam in range(2)], msgs[:info.cam[0].messages + info.cam[1].messages]))
        ev, msgs = joined(parts)
        assert ev == [whole["events"][0].tobytes(), whole["events"][1].tobytes()], ([kinds[c] for c in chosen], cuts)
        assert msgs.tobytes() == whole["messages"].tobytes(), cuts


# ---- failures ------------------------------------------------------------------------------------------------------------
def lead_chunk(rng):
    """a whole chunk that makes both event connections and the IMU's known and emits 3 left events and 2 right ones"""
    return B.chunk_record(B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5) + B.connection_record(1, B.RIGHT, B.EVENT_TYPE, B.EVENT_MD5) +
                          B.connection_record(2, B.IMU, B.IMU_TYPE, B.IMU_MD5) +
                          B.message_record(0, (7, 1), B.event_array(1, (7, 1), rand_wire(3, rng))) +
                          B.message_record(1, (7, 2), B.event_array(1, (7, 1), rand_wire(2, rng))))


def after(conn, k, wire):
    return B.chunk_record(B.message_record(conn, (8, k), B.event_array(k, (8, k), wire)))


def test_every_bad_cause_counts_exactly_and_leaves_the_state(bg):
    T = tile()
    rng = np.random.default_rng(35)
    n = T + 30
    good = np.frombuffer(rand_wire(n, rng), B.WIRE_DTYPE)
    cases = {"nsec == 10^9": ([3], 10 ** 9), "nsec all ones": ([0, n - 1], 0xFFFFFFFF), "both sides of the tile edge": ([T - 1, T], 10 ** 9 + 1),
             "every event": (list(range(n)), 2 * 10 ** 9)}
    for name, (where, value) in cases.items():
        for cams in ((0,), (1,), (0, 1)):
            bg.fresh()
            lead = lead_chunk(rng)
            bg.check(lead[:-5], tag="lead")  # an event cut by the call's end waits in the state
            wire = good.copy()
            wire["nsec"][where] = value
            data = lead[-5:] + after(0, 2, wire.tobytes() if 0 in cams else good.tobytes()) + after(1, 2, wire.tobytes() if 1 in cams else good.tobytes())
            with pytest.raises(B.Bad) as e:
                bg.ev.feed(data)
            assert e.value.bad == [len(where) * (0 in cams), len(where) * (1 in cams)]
            rc, _, _, info = bg.call(data, dst_space=FE.DEVICE if len(cams) == 2 else FE.HOST)
            assert rc == -1 and [info.cam[0].bad, info.cam[1].bad] == e.value.bad, (name, cams)
            assert (info.cam[0].events, info.cam[1].events) == (n, n + 1) and b"10^9" in bg.error()
            # the fault removed: what a run that never failed gives, the waiting event included
            o = bg.check(lead[-5:] + after(0, 2, good.tobytes()) + after(1, 2, good.tobytes()), tag=(name, "after the failure"))
            assert o["messages"]["first"].tolist() == [0, 3, 2]
    # a stamp with nsec >= 10^9 in an Imu message: the side call's BAD
    bg.fresh()
    lead = lead_chunk(rng)
    bg.side_check(lead)
    imu = lambda k, nsec: B.chunk_record(B.message_record(2, (8, k), B.imu_message(k, (8, nsec), (1, 2, 3), (4, 5, 6))))
    with pytest.raises(FE.FrontendError) as e:
        bg.ft.bag_side(imu(1, 5) + imu(2, 10 ** 9) + imu(3, 0xFFFFFFFF))
    assert (e.value.info.imu, e.value.info.bad) == (1, 2)
    assert len(bg.side_check(imu(1, 5) + imu(2, 999_999_999))["imu"]) == 2
    bg.check(lead + imu(2, 10 ** 9), tag="a BAD sample is not the event call's business")


def test_every_malformed_cause_is_refused_before_any_device_work_with_the_state_as_it_was(bg):
    rng = np.random.default_rng(36)
    three = [B.message_record(0, (8, k), B.event_array(k, (8, k), rand_wire(40, rng))) for k in range(3)]
    cut = bytearray(three[1])
    struct.pack_into("<I", cut, len(cut) - 40 * 13 - 4, 41)  # n says 41, data_len says 40
    streams = dict(B.malformed_streams())
    streams["a length mismatch in the second of three messages"] = B.chunk_record(three[0] + bytes(cut) + three[2])
    streams["an md5 mismatch on a selected topic, behind good messages"] = B.chunk_record(three[0]) + B.chunk_record(
        B.connection_record(9, B.RIGHT, B.EVENT_TYPE, b"0" * 32) + three[1])
    for name, data in streams.items():
        bg.fresh()
        lead = lead_chunk(rng)
        bg.check(lead, tag="lead")
        bg.side_check(lead)
        with pytest.raises(B.Malformed):
            bg.ev.feed(data)
        rc, got, msgs, info = bg.call(data, dst_space=FE.DEVICE)
        assert rc == -1 and b"malformed" in bg.error(), name
        assert (got[0] == GUARD).all() and (got[1] == GUARD).all() and (msgs.view(np.uint8) == GUARD).all(), name
        assert (info.cam[0].events, info.cam[1].events, info.cam[0].messages, info.chunks) == (0, 0, 0, 0), name
        with pytest.raises(FE.FrontendError, match="malformed"):
            bg.ft.bag_side(data)
        o = bg.check(B.chunk_record(three[0] + three[1]), tag=(name, "after the failure"))
        assert o["messages"]["first"].tolist() == [3, 43]
        bg.side_check(B.chunk_record(three[0]))
    rc, _, _, _ = bg.call(streams["a compressed chunk"])
    assert rc == -1 and b"rosbag decompress" in bg.error()
    rc, _, _, _ = bg.call(streams["another md5 on an event topic"])
    assert rc == -1 and B.LEFT.encode() in bg.error()
    # argument errors
    bg.fresh()
    L, h = bg.L, bg.h
    info, buf = FE.BagInfo(), np.frombuffer(lead_chunk(rng), np.uint8)
    dst = [np.zeros(64, EVENT_DTYPE), np.zeros(64, EVENT_DTYPE)]
    msgs = np.zeros(8, FE.BAG_MESSAGE_DTYPE)

    def args(**k):
        p = (C.c_void_p * 2)(k.get("d0", dst[0].ctypes.data), dst[1].ctypes.data)
        return [FE._p(buf), len(buf), k.get("flags", 0), C.byref(p), C.byref((C.c_size_t * 2)(64, 64)), k.get("space", FE.HOST),
                k.get("msgs", FE._p(msgs)), 8, C.byref(info)]
    for bad in (dict(flags=1), dict(d0=None), dict(space=7), dict(d0=dst[0].ctypes.data + 8, space=FE.DEVICE), dict(msgs=None)):
        assert L.esvio_fe_decode_bag(h, *args(**bad)) == -1, bad
    assert L.esvio_fe_decode_bag(h, None, 8, 0, None, None, FE.HOST, None, 0, C.byref(info)) == -1
    for bad in ((B.LEFT, B.LEFT, None), ("", None, None), (None, None, "/" + "t" * 255)):
        with pytest.raises(FE.FrontendError):
            bg.ft.bag_set_topics(*bad)
    bg.check(bytes(buf), tag="after the argument errors")


def test_dst_cap_and_msgs_cap_one_too_small_report_the_counts_and_store_nothing(bg):
    T = tile()
    rng = np.random.default_rng(37)
    data = body([msg(B.LEFT, 1, rand_wire(T + 77, rng)), msg(B.RIGHT, 1, rand_wire(90, rng)), msg(B.LEFT, 2, rand_wire(5, rng, 3000))])
    nl, nr = T + 82, 90
    for dst_space in (FE.HOST, FE.DEVICE):
        for caps, mcap in (((nl - 1, nr), 3), ((nl, nr - 1), 3), ((nl, nr), 2)):
            bg.fresh()
            rc, got, msgs, info = bg.call(data, caps, mcap, dst_space)
            assert rc == -1 and (info.cam[0].events, info.cam[1].events, info.cam[0].messages, info.cam[1].messages) == (nl, nr, 2, 1)
            for cam in range(2):
                if caps[cam] < (nl, nr)[cam] and dst_space == FE.DEVICE:
                    assert (got[cam] == GUARD).all()  # the kernel stores nothing into a dst that is too small
            bg.check(data, dst_space=dst_space, exact_cap=True, tag="exact room")
    bg.fresh()
    rc, _, _, info = bg.call(b"")
    assert rc == 0 and info.cam[0].events == 0 and info.cam[0].first_sec == 0x77777777


# ---- the side call -------------------------------------------------------------------------------------------------------
def test_the_side_call_in_either_order_with_the_event_call(bg):
    rng = np.random.default_rng(38)
    messages = []
    for k in range(12):
        messages += [msg(B.LEFT, k, rand_wire(50 + k, rng, 1000 * k)), (B.IMU, (7, k), B.imu_message(k, (7, 3 * k), rng.normal(0, 1, 3), rng.normal(0, 9, 3))),
                     (B.IMU, (7, k), B.imu_message(k, (1_700_000_000, k), rng.normal(0, 1, 3), rng.normal(0, 9, 3), frame_id=b"")),
                     msg(B.RIGHT, k, rand_wire(40, rng, 1000 * k))]
    data = body(messages, per_chunk=5)
    whole_e, whole_s = B.Walker("events").feed(data)[1], B.Walker("side").feed(data)[1]
    cuts = [0, 333, 334, 4200, 4433, 9000, len(data)]
    for order in ("events first", "side first"):
        bg.fresh()
        ev, imu = [[], []], []
        for lo, hi in zip(cuts, cuts[1:]):
            for which in (("e", "s") if order == "events first" else ("s", "e")):
                if which == "e":
                    o = bg.check(data[lo:hi], tag=(order, lo))
                    for cam in range(2):
                        ev[cam].append(o["events"][cam].tobytes())
                else:
                    imu.append(bg.side_check(data[lo:hi], tag=(order, lo))["imu"])
        assert [b"".join(e) for e in ev] == [whole_e["events"][0].tobytes(), whole_e["events"][1].tobytes()]
        assert np.concatenate(imu).tobytes() == whole_s["imu"].tobytes() and len(whole_s["imu"]) == 24
    bg.fresh()
    with pytest.raises(FE.FrontendError) as e:  # a capacity one too small: the number comes back, the state stays
        bg.ft.bag_side(data, imu_cap=23)
    assert e.value.info.imu == 24
    bg.side_check(data, tag="after the failure")
    bg.ft.decode_reset()  # the states are cleared, the topics stay
    bg.ev, bg.side = B.Walker("events"), B.Walker("side")
    bg.check(data[:5000], tag="after decode_reset")
    bg.side_check(data[:5000])


# ---- end to end ----------------------------------------------------------------------------------------------------------
W, H = 346, 260


@pytest.fixture(scope="module")
def frames():
    """4 frames of a scene stream at the DAVIS346's size as one bag: per frame a left and a right EventArray message with
    one header stamp, the right one first in every other frame, an Imu message and an image-like message between them"""
    st = SceneStream(W=W, H=H, rate=1e6, seed=7)
    rng = np.random.default_rng(3)
    recs, messages = [], []
    for k in range(4):
        left, right, _ = st.next_batch()
        stamp = (int(left["sec"][-1]), int(left["nsec"][-1]))
        pair = []
        for topic, ev in ((B.LEFT, left), (B.RIGHT, right)):
            wire = B.wire_events(ev["x"], ev["y"], ev["sec"], ev["nsec"], ev["polarity"])
            pair.append((topic, stamp, B.event_array(k, stamp, wire, height=H, width=W)))
        messages += pair[::-1 if k % 2 else 1]
        messages += [(B.IMU, stamp, B.imu_message(k, stamp, rng.normal(0, 1, 3), rng.normal(0, 9, 3))),
                     (IMAGE, stamp, B.ros_header(k, stamp, b"cam") + b"\x33" * 2000)]
        recs.append((left, right))
    bag = B.write_bag(messages, per_chunk=3)
    o = B.decode(bag)
    assert o["events"][0].tobytes() == b"".join(l.tobytes() for l, _ in recs)  # the loop's records are the generator's
    return bag, recs


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def make_tracker(max_cnt=150):
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=max_cnt))
    ft.bag_set_topics(*B.TOPICS)
    return ft


def test_tracking_message_pairs_from_the_device_slices_equals_track_event_on_the_loops_records(frames):
    bag, recs = frames
    hdr = FE.bag_header(bag)
    assert (hdr.complete, hdr.version, hdr.conn_count) == (1, 20, 4)
    a, b = make_tracker(), make_tracker()
    try:
        (dl, dr), msgs, info = b.decode_bag(bag[int(hdr.payload_offset):], device=True)
        loop = B.decode(bag)
        assert msgs.tobytes() == loop["messages"].tobytes() and (info.cam[0].events, info.cam[1].events) == tuple(len(e) for e in loop["events"])
        left = {(int(m["stamp_sec"]), int(m["stamp_nsec"])): m for m in msgs if m["cam"] == 0}
        pairs = [(left[(int(m["stamp_sec"]), int(m["stamp_nsec"]))], m) for m in msgs if m["cam"] == 1]  # paired by header stamp
        assert len(pairs) == 4
        for i, (ml, mr) in enumerate(sorted(pairs, key=lambda p: int(p[0]["first"]))):
            L, Rr = recs[i]
            assert (int(ml["count"]), int(mr["count"])) == (len(L), len(Rr))
            t1 = float(event_times(L[-1:])[0])  # cur_time: the last left event's stamp
            a.trackEvent(t1, L, Rr, i % 2 == 0)
            b.trackEvent(t1, (dl.ptr.value + 16 * int(ml["first"]), int(ml["count"])), (dr.ptr.value + 16 * int(mr["first"]), int(mr["count"])), i % 2 == 0)
            # a decode and a side call between two track calls change no later result
            b.decode_reset()
            b.decode_bag(bag[13:200_000])
            b.bag_side(bag[13:200_000])
            assert results(a) == results(b), i
        assert len(a.ids) > 0 and len(a.ids_right) > 0
        dl.free()
        dr.free()
    finally:
        a.close()
        b.close()


def test_a_feed_fed_4099_byte_chunks_equals_the_feed_fed_the_loops_records(frames):
    bag, recs = frames
    data = bag[13:]
    a, b = make_tracker(40), make_tracker(40)
    try:
        a.feed_open(200.0)
        b.feed_open(200.0)
        tracked, w, appended = 0, B.Walker("events"), [0, 0]
        stop = 2_600_000  # a frame and a half: a dozen windows at 200 Hz
        for lo in range(0, stop, 4099):
            hi = min(lo + 4099, stop)
            w, o = w.feed(data[lo:hi])
            ia = a.feed_push_bag(data[lo:hi])
            for cam in range(2):  # left before right
                ib = b.feed_push_events(cam, o["events"][cam])
                assert (ia[cam].appended, ia[cam].closed, ia[cam].queued, ia[cam].bad) == (ib.appended, ib.closed, ib.queued, 0), (lo, cam)
                assert ia[cam].appended == len(o["events"][cam])
                appended[cam] += ia[cam].appended
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
        assert tracked >= 5 and len(a.ids) > 0 and min(appended) > 1000
        a.decode_reset()  # (the last chunk ended inside a message: from the fresh state the next bytes are a record's)
        with pytest.raises(FE.FrontendError, match="malformed") as e:  # a malformed stream: nothing appended
            a.feed_push_bag(b"\x01\x10\x00\x00")
        assert e.value.info[0].appended == e.value.info[1].appended == 0
    finally:
        a.close()
        b.close()


def test_the_feeds_no_origin_refusal_leaves_the_walker_as_it_was():
    rng = np.random.default_rng(39)
    conns = B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5) + B.connection_record(1, B.RIGHT, B.EVENT_TYPE, B.EVENT_MD5)
    right = B.chunk_record(conns + B.message_record(1, (7, 1), B.event_array(1, (7, 1), rand_wire(30, rng))))
    left = B.chunk_record(B.message_record(0, (7, 2), B.event_array(1, (7, 1), rand_wire(20, rng))))
    ft = make_tracker(40)
    try:
        ft.feed_open(200.0)
        info = ft.feed_push_bag(right[:100])  # no event yet: fine
        assert (info[0].appended, info[1].appended) == (0, 0)
        with pytest.raises(FE.FrontendError, match="origin") as e:
            ft.feed_push_bag(right[100:])
        assert e.value.info[1].appended == 0
        with pytest.raises(FE.FrontendError, match="origin"):
            ft.feed_push_bag(right[100:] + left[:60])  # (a left message whose events have not arrived is no left event)
        info = ft.feed_push_bag(right[100:] + left)  # the longer chunk: the connections of the first call are still known
        assert (info[0].appended, info[1].appended) == (20, 30)
        info = ft.feed_push_bag(B.chunk_record(B.message_record(1, (7, 3), B.event_array(2, (7, 3), rand_wire(4, rng, 60_000_000)))))
        assert (info[0].appended, info[1].appended) == (0, 4)
        ft.feed_close()
        # with an explicit origin right events alone are taken
        ft.decode_reset()
        ft.feed_open(200.0, origin=(7, 0))
        info = ft.feed_push_bag(right)
        assert (info[0].appended, info[1].appended) == (0, 30)
    finally:
        ft.close()


def test_reserve_covers_the_scratch_and_a_second_call_allocates_nothing(frames):
    bag, recs = frames
    data = np.frombuffer(bag[13:], np.uint8)
    ft = make_tracker()
    L, h = ft._hd.L, ft._hd.h
    try:
        n = [sum(len(r[cam]) for r in recs) for cam in range(2)]
        (first, _), _, _ = ft.decode_bag(bag[13:300_000])  # a handle that has decoded a bag before: the kernel has run once
        assert len(first) > 1000
        ft.decode_reset()
        ft._hd.check(L.esvio_fe_reserve(h, n[0], n[1], 0))
        dst = [FE.EventBuffer(np.zeros(n[cam], EVENT_DTYPE), FE.DEVICE) for cam in range(2)]
        msgs, info = np.zeros(16, FE.BAG_MESSAGE_DTYPE), FE.BagInfo()
        a0, mem0 = ft.latency_stats()["allocs"], ft.device_memory()[0]
        for _ in range(2):
            ptrs = (C.c_void_p * 2)(dst[0].arg[0], dst[1].arg[0])
            assert L.esvio_fe_decode_bag(h, FE._p(data), len(data), 0, C.byref(ptrs), C.byref((C.c_size_t * 2)(*n)), FE.DEVICE, FE._p(msgs), 16,
                                         C.byref(info)) == 0
            assert [info.cam[0].events, info.cam[1].events] == n
            ft.decode_reset()
        assert ft.latency_stats()["allocs"] == a0 and ft.device_memory()[0] == mem0
        for d in dst:
            d.free()
        # a host dst's records grow on first use; the second call of the size allocates nothing
        ft.decode_bag(bag[13:])
        mem0 = ft.device_memory()[0]
        ft.decode_reset()
        ft.decode_bag(bag[13:])
        assert ft.device_memory()[0] == mem0
    finally:
        ft.close()
