"""GPU: esvio_fe_convert_image, esvio_fe_decode_bag_images and esvio_fe_track_image_space against the sequential reading
tests/bag_image_ref.py.  Integers only: every byte of every gray image, every row of the image table and every info field
are compared for equality, with guard bytes around every destination.  The conversion and decode cases run once: k_image_emit
has one form of its load."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bag_image_ref as I
import bag_ref as B
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times
from esvio_amd.node import StereoImageTrackerNode
from esvio_amd.synth import ImageStream, SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
W0, H0 = 43, 42  # the smallest handle there is, with an odd width: 1806 pixels, so a call's second image begins off a dword
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


class Mem:
    """memory of the library's runtime: device, or page-locked host"""

    def __init__(self, L, space, n):
        self.L, self.space, self.n, self.p = L, space, n, C.c_void_p()
        assert L.esvio_fe_mem_alloc(space, max(n, 1), C.byref(self.p)) == 0
        self.hip = C.CDLL("libamdhip64.so")

    def put(self, a):
        a = np.ascontiguousarray(a, np.uint8)
        if self.space == FE.DEVICE:
            assert self.L.esvio_fe_mem_upload(self.p, C.c_void_p(a.ctypes.data), a.nbytes) == 0
        else:
            C.memmove(self.p, a.ctypes.data, a.nbytes)
        return self

    def get(self):
        out = np.zeros(self.n, np.uint8)
        if self.space == FE.DEVICE:
            assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.n), 2) == 0
        else:
            C.memmove(out.ctypes.data, self.p, self.n)
        return out

    def free(self):
        self.L.esvio_fe_mem_free(self.space, self.p)


class Im:
    """a handle and the reading's image walker, advanced together"""

    def __init__(self, W=W0, H=H0, **kw):
        self.ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=kw.pop("max_cnt", 40), **kw))
        self.W, self.H, self.L, self.h = W, H, self.ft._hd.L, self.ft._hd.h
        self.fresh()

    def fresh(self, topics=I.IMAGE_TOPICS):
        self.ft.bag_set_image_topics(*topics)
        self.w = I.ImageWalker(topics, (self.W, self.H))

    def close(self):
        self.ft.close()

    def error(self):
        return self.L.esvio_fe_last_error(self.h).decode()

    def call(self, data, dst_cap=None, msgs_cap=None, dst_space=FE.HOST, flags=0, lead=(0, 0)):
        """one esvio_fe_decode_bag_images call -> (rc, per camera the dst_cap images as bytes, the table rows, the info);
        dst[cam] lies lead[cam] bytes behind a 16-byte boundary; the reading does not move"""
        wh = self.W * self.H
        buf = np.frombuffer(data, np.uint8)
        most = len(data) // (38 + self.H) + 1
        caps = [most] * 2 if dst_cap is None else list(dst_cap)
        msgs_cap = most if msgs_cap is None else msgs_cap
        info = FE.BagImageInfo()
        back = [np.full(lead[cam] + wh * caps[cam] + 32, GUARD, np.uint8) for cam in range(2)]
        msgs = np.zeros(msgs_cap + 1, FE.BAG_IMAGE_DTYPE)
        msgs.view(np.uint8)[:] = GUARD
        ptrs, dev = (C.c_void_p * 2)(), []
        for cam in range(2):
            if dst_space == FE.DEVICE:
                dev.append(Mem(self.L, FE.DEVICE, len(back[cam])).put(back[cam]))
                ptrs[cam] = dev[cam].p.value + lead[cam]
            else:
                ptrs[cam] = back[cam].ctypes.data + lead[cam]
        rc = self.L.esvio_fe_decode_bag_images(self.h, FE._p(buf) if len(buf) else None, len(buf), flags, C.byref(ptrs), C.byref((C.c_size_t * 2)(*caps)),
                                               dst_space, FE._p(msgs), msgs_cap, C.byref(info))
        for cam, d in enumerate(dev):
            back[cam] = d.get()
            d.free()
        for cam in range(2):
            assert (back[cam][:lead[cam]] == GUARD).all() and (back[cam][lead[cam] + wh * caps[cam]:] == GUARD).all(), "bytes around dst touched"
        assert (msgs[msgs_cap:].view(np.uint8) == GUARD).all(), "rows beyond msgs_cap touched"
        return rc, [back[cam][lead[cam]:lead[cam] + wh * caps[cam]] for cam in range(2)], msgs[:msgs_cap], info

    def check(self, data, dst_space=FE.HOST, tag=None, exact_cap=False, lead=(0, 0)):
        """a call that succeeds equals the reading, which advances with it -> the reading's result"""
        w, o = self.w.feed(data)
        n = [len(o["images"][0]), len(o["images"][1])]
        rc, got, msgs, info = self.call(data, n if exact_cap else None, len(o["table"]) if exact_cap else None, dst_space, lead=lead)
        assert rc == 0, (tag, rc, self.error())
        self.w = w
        wh = self.W * self.H
        for cam in range(2):
            ci = info.cam[cam]
            assert ci.images == n[cam], (tag, cam)
            mine = o["table"][o["table"]["cam"] == cam]
            want = (int(mine["stamp_sec"][0]), int(mine["stamp_nsec"][0]), int(mine["stamp_sec"][-1]), int(mine["stamp_nsec"][-1])) if n[cam] else (0, 0, 0, 0)
            assert (ci.first_sec, ci.first_nsec, ci.last_sec, ci.last_nsec) == want, (tag, cam)
            for k, img in enumerate(o["images"][cam]):
                g = got[cam][k * wh:(k + 1) * wh].reshape(self.H, self.W)
                if not np.array_equal(g, img):
                    y, x = np.argwhere(g != img)[0]
                    raise AssertionError((tag, cam, k, "first differing pixel", int(x), int(y), int(g[y, x]), int(img[y, x])))
            assert (got[cam][n[cam] * wh:] == GUARD).all(), (tag, cam, "bytes behind the last image touched")
        assert msgs[:len(o["table"])].tobytes() == o["table"].tobytes(), tag
        assert (info.other_messages, info.other_records, info.chunks, info.connections) == tuple(o[k] for k in I.COUNTERS), tag
        return o


@pytest.fixture(scope="module")
def im():
    d = Im()
    yield d
    d.close()


# ---- the conversion alone --------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (5, 1), (3, 2), (63, 3), (64, 3), (65, 3), (257, 3), (1030, 2))  # (width, height); the last: whole waves of one row


def test_convert_image_equals_the_loop_at_every_shape_class_step_offset_and_space(im):
    L, h = im.L, im.h
    sources = []
    for (w, hh), cls, pad in itertools.product(SHAPES, (1, 2, 3), (0, 1, 5, 16)):
        step = w * I.BPP[cls] + pad
        data = I.rows(I.test_image(hh, w, cls, 100 + w + cls), step)
        sources.append((w, hh, cls, step, np.frombuffer(data, np.uint8), I.convert_rows(data, hh, w, step, cls)))
    assert np.array_equal(sources[8][5], I.convert(sources[8][4].tobytes(), 1, 1, sources[8][3], sources[8][2]))  # (the loops themselves, once)
    room = max(len(s[4]) for s in sources) + 64
    src_mem = {"device": Mem(L, FE.DEVICE, room), "page-locked": Mem(L, FE.HOST, room)}
    dst_mem = Mem(L, FE.DEVICE, max(s[0] * s[1] for s in sources) + 64)
    host_src = np.zeros(room + 16, np.uint8)
    base = (-host_src.ctypes.data) & 15
    n = 0
    for (w, hh, cls, step, data, want), off in itertools.product(sources, (0, 1, 2, 3)):
        for where, dst_dev in itertools.product(("host", "page-locked", "device"), (False, True)):
            n += 1
            if where == "host":
                host_src[base + off:base + off + len(data)] = data
                sp, space = host_src.ctypes.data + base + off, FE.HOST
            else:
                m = src_mem[where]
                staged = np.full(room, 0xEE, np.uint8)
                staged[off:off + len(data)] = data
                m.put(staged)
                sp, space = m.p.value + off, FE.DEVICE if where == "device" else FE.HOST
            tag = (w, hh, cls, step, off, where, dst_dev)
            if dst_dev:
                dst_mem.put(np.full(dst_mem.n, GUARD, np.uint8))
                rc = L.esvio_fe_convert_image(h, C.c_void_p(sp), space, hh, w, step, cls, C.c_void_p(dst_mem.p.value + 16 + off), FE.DEVICE)
                back = dst_mem.get()
            else:
                back = np.full(dst_mem.n, GUARD, np.uint8)
                rc = L.esvio_fe_convert_image(h, C.c_void_p(sp), space, hh, w, step, cls, C.c_void_p(back.ctypes.data + 16 + off), FE.HOST)
            assert rc == 0, (tag, im.error())
            got = back[16 + off:16 + off + w * hh].reshape(hh, w)
            if not np.array_equal(got, want):
                y, x = np.argwhere(got != want)[0]
                raise AssertionError((tag, "first differing pixel", int(x), int(y), int(got[y, x]), int(want[y, x])))
            assert (back[:16 + off] == GUARD).all() and (back[16 + off + w * hh:] == GUARD).all(), (tag, "bytes around dst touched")
    assert n == len(SHAPES) * 3 * 4 * 4 * 3 * 2
    # the Python mirror: host in, host out and device out
    w, hh, cls, step, data, want = sources[-1]
    assert np.array_equal(im.ft.convert_image(data, hh, w, step, cls), want)
    dev = im.ft.convert_image(data, hh, w, step, cls, device=True)
    assert np.array_equal(dev.download()[0], want) and dev.image(0) == dev.ptr.value
    dev.free()
    # the argument errors, before any device work
    px = np.zeros(64, np.uint8)
    ok = dict(src=FE._p(px), ss=FE.HOST, h=2, w=3, step=9, enc=3, dst=FE._p(px), ds=FE.HOST)
    for bad in (dict(src=None), dict(dst=None), dict(ss=5), dict(ds=-1), dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(enc=0), dict(enc=4),
                dict(step=8), dict(enc=1, step=2)):
        a = dict(ok, **bad)
        assert L.esvio_fe_convert_image(h, a["src"], a["ss"], a["h"], a["w"], a["step"], a["enc"], a["dst"], a["ds"]) == -1, bad
    for m in list(src_mem.values()) + [dst_mem]:
        m.free()


# ---- the decode call -------------------------------------------------------------------------------------------------------
def image_msg(topic, k, cls, name, w, h, pad, seed, sec=7):
    step = w * I.BPP[cls] + pad
    return (topic, (sec, 1000 + k), I.image_message(k, (sec, 10 * k), h, w, name, step, I.rows(I.test_image(h, w, cls, seed), step)))


def lean_bag(w=W0, h=H0):
    """three images — left 8UC1 with an odd step, right rgb8, left mono8 alone in its chunk — between events, IMU and a
    foreign topic"""
    ev = B.wire_events([1, 2], [3, 4], [10, 10], [100, 200], [1, 0])
    msgs = [(B.LEFT, (7, 1), B.event_array(1, (7, 1), ev)), image_msg(I.LEFT_IMAGE, 1, 1, "8UC1", w, h, 1, 61),
            (B.IMU, (7, 2), B.imu_message(7, (7, 2), (0.1, -0.2, 0.3), (9.5, 0.25, -1.5))), image_msg(I.RIGHT_IMAGE, 1, 3, "rgb8", w, h, 5, 62),
            ("/odometry", (7, 3), B.ros_header(4, (7, 3), b"odom") + bytes(40)), image_msg(I.LEFT_IMAGE, 2, 1, "mono8", w, h, 0, 63)]
    return I.write_bag(msgs, per_chunk=5, header_total=None)


def test_left_rgb8_right_mono8_and_a_bgr8_message_at_346x260_in_one_launch():
    d = Im(346, 260)
    try:
        msgs = [image_msg(I.LEFT_IMAGE, 1, 3, "rgb8", 346, 260, 2, 71), image_msg(I.RIGHT_IMAGE, 1, 1, "mono8", 346, 260, 0, 72),
                image_msg(I.LEFT_IMAGE, 2, 2, "bgr8", 346, 260, 7, 73), image_msg(I.RIGHT_IMAGE, 2, 2, "8UC3", 346, 260, 0, 74)]
        data = I.write_bag(msgs, per_chunk=3)[13:]
        d.ft.set_profiling(True)
        d.ft.reset_kernel_stats()
        o = d.check(data, dst_space=FE.DEVICE, tag="mixed classes", exact_cap=True, lead=(3, 1))
        assert o["table"]["encoding"].tolist() == [3, 1, 2, 2] and (346 * 260) % 16 != 0
        names = [d.L.esvio_fe_kernel_name(k).decode() for k in range(d.L.esvio_fe_ingest_kernel_count())]
        ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        d.ft._hd.check(d.L.esvio_fe_get_kernel_stats(d.h, names.index("k_image_emit"), C.byref(ms), C.byref(n), C.byref(b)))
        assert n.value == 1  # one launch for all four images of both cameras
        d.ft.set_profiling(False)
        d.fresh()
        d.check(data, dst_space=FE.HOST, tag="mixed classes, host dst")
    finally:
        d.close()


def test_the_lean_bag_at_every_byte_cut_in_two_calls(im):
    s = lean_bag()[13:]
    done, _ = I.read_stream(s, size=(W0, H0))
    want = [I.convert_rows(m["data"], H0, W0, m["step"], m["encoding"]).tobytes() for m in done]
    im.fresh()
    o = im.check(s, tag="one call")
    assert [len(v) for v in o["images"]] == [2, 1]
    wh = W0 * H0
    for cut in range(len(s) + 1):
        im.fresh()
        got = []
        for k, piece in enumerate((s[:cut], s[cut:])):
            expect = [m for m in done if (m["end"] <= cut) == (k == 0)]  # the messages whose last byte the piece brings
            rc, img, msgs, info = im.call(piece, dst_cap=(2, 1), msgs_cap=3, dst_space=FE.DEVICE if (cut + k) % 5 == 0 else FE.HOST)
            assert rc == 0, (cut, im.error())
            assert [int(c) for c in msgs["cam"][:len(expect)]] == [m["cam"] for m in expect] and info.cam[0].images + info.cam[1].images == len(expect), cut
            got += [img[int(m["cam"])][int(m["index"]) * wh:(int(m["index"]) + 1) * wh].tobytes() for m in msgs[:len(expect)]]
        assert got == want, cut
    for cut in range(0, len(s) + 1, 397):  # ... and call by call against the reading at a few cuts
        im.fresh()
        im.check(s[:cut], tag=(cut, "first"))
        im.check(s[cut:], tag=(cut, "second"), dst_space=FE.DEVICE, exact_cap=True)


def test_a_three_image_bag_at_32_seeded_multi_cuts_with_device_destinations(im):
    s = lean_bag()[13:]
    done, _ = I.read_stream(s, size=(W0, H0))
    rng = np.random.default_rng(12)
    places = [(m["end"] - m["step"] * m["height"], m["end"]) for m in done] + [(m["end"] - m["step"] * m["height"] - 60, m["end"] - m["step"] * m["height"]) for m in done]
    for it in range(32):
        im.fresh()
        cuts = sorted(int(rng.integers(*places[int(c)])) for c in rng.choice(len(places), int(rng.integers(1, 5)), replace=False))
        n = 0
        for lo, hi in zip([0] + cuts, cuts + [len(s)]):
            n += len(im.check(s[lo:hi], dst_space=FE.DEVICE, tag=(cuts, lo), exact_cap=it % 2 == 0, lead=(it % 4, (it + 1) % 4))["table"])
        assert n == 3


def test_the_caps_one_too_small_report_the_counts_and_store_nothing(im):
    s = lean_bag()[13:]
    for dst_space in (FE.HOST, FE.DEVICE):
        for caps, mcap in (((1, 1), 3), ((2, 0), 3), ((2, 1), 2)):
            im.fresh()
            rc, got, msgs, info = im.call(s, caps, mcap, dst_space)
            assert rc == -1 and (info.cam[0].images, info.cam[1].images) == (2, 1) and "as it was" in im.error()
            assert all((g == GUARD).all() for g in got) and (msgs.view(np.uint8) == GUARD).all()
            im.check(s, dst_space=dst_space, exact_cap=True, tag="exact room")
    im.fresh()
    rc, _, _, info = im.call(b"")
    assert rc == 0 and info.cam[0].images == 0


def test_each_refusal_leaves_the_state_so_that_the_corrected_continuation_gives_the_loops_result(im):
    s = lean_bag()[13:]
    end = I.read_stream(s, size=(W0, H0))[0][-1]["end"]
    lead, rest = s[:end - 700], s[end - 700:end]  # the last image waits but for 700 bytes
    for name, (data, names) in I.bad_streams(W0, H0).items():
        im.fresh()
        im.check(lead, tag="lead")
        with pytest.raises(B.Malformed):
            im.w.feed(rest + data)
        rc, got, msgs, info = im.call(rest + data, dst_space=FE.DEVICE)
        assert rc == -1 and names in im.error() and "as it was" in im.error(), (name, im.error())
        assert all((g == GUARD).all() for g in got) and (msgs.view(np.uint8) == GUARD).all() and info.cam[0].images == 0, name
        o = im.check(rest, tag=(name, "after the refusal"))
        assert len(o["images"][0]) == 1
    # the topic rules, the clash with an event topic among them; a refused call leaves the topics as they were
    im.fresh()
    im.ft.bag_set_topics(*B.TOPICS)
    for bad in ((B.LEFT, None), (I.LEFT_IMAGE, B.IMU), ("/a", "/a"), ("", None), (None, "/" + "t" * 255)):
        with pytest.raises(FE.FrontendError):
            im.ft.bag_set_image_topics(*bad)
    im.check(s, tag="after the refused topics")
    # the argument errors
    info, buf = FE.BagImageInfo(), np.frombuffer(s, np.uint8)
    dst, msgs = [np.zeros(2 * W0 * H0, np.uint8), np.zeros(2 * W0 * H0, np.uint8)], np.zeros(8, FE.BAG_IMAGE_DTYPE)

    def args(**k):
        p = (C.c_void_p * 2)(k.get("d0", dst[0].ctypes.data), dst[1].ctypes.data)
        return [FE._p(buf), len(buf), k.get("flags", 0), C.byref(p), C.byref((C.c_size_t * 2)(2, 2)), k.get("space", FE.HOST), k.get("msgs", FE._p(msgs)), 8,
                C.byref(info)]
    im.fresh()
    for bad in (dict(flags=1), dict(d0=None), dict(space=7), dict(msgs=None)):
        assert im.L.esvio_fe_decode_bag_images(im.h, *args(**bad)) == -1, bad
    assert im.L.esvio_fe_decode_bag_images(im.h, None, 8, 0, None, None, FE.HOST, None, 0, C.byref(info)) == -1
    tr, px = (C.c_uint8 * 512)(), np.zeros(W0 * H0, np.uint8)
    assert im.L.esvio_fe_track_image_space(im.h, 1.0, FE._p(px), None, 5, 1, C.byref(tr)) == -1
    assert im.L.esvio_fe_track_image_space(im.h, 1.0, None, None, FE.DEVICE, 1, C.byref(tr)) == -1
    im.check(s, tag="after the argument errors")


def test_the_image_call_the_event_call_and_the_side_call_on_the_same_bytes_in_all_orders(im):
    rng = np.random.default_rng(13)
    messages = []
    for k in range(4):
        t = 1000 * k + np.sort(rng.integers(0, 900, 30))
        wire = B.wire_events(rng.integers(0, W0, 30), rng.integers(0, H0, 30), np.full(30, 7), t, rng.choice([0, 1], 30))
        messages += [(B.LEFT, (7, k), B.event_array(k, (7, 10 * k), wire)), image_msg(I.LEFT_IMAGE, k, 1 + k % 3, ("mono8", "bgr8", "rgb8")[k % 3], W0, H0, k, 80 + k),
                     (B.IMU, (7, k), B.imu_message(k, (7, 3 * k), rng.normal(0, 1, 3), rng.normal(0, 9, 3))),
                     (B.RIGHT, (7, k), B.event_array(k, (7, 10 * k), wire[:13 * 20])), image_msg(I.RIGHT_IMAGE, k, 3, "rgb8", W0, H0, 3, 90 + k)]
    data = I.write_bag(messages, per_chunk=4)[13:]
    whole_i, whole_e, whole_s = I.ImageWalker(size=(W0, H0)).feed(data)[1], B.Walker("events").feed(data)[1], B.Walker("side").feed(data)[1]
    cuts = [0, 1500, 1501, 9000, 16000, len(data)]
    for order in itertools.permutations("ies"):
        im.fresh()
        im.ft.bag_set_topics(*B.TOPICS)
        ev, imu, images = [[], []], [], [[], []]
        for lo, hi in zip(cuts, cuts[1:]):
            for which in order:
                if which == "i":
                    o = im.check(data[lo:hi], tag=(order, lo))
                    for cam in range(2):
                        images[cam] += [g.tobytes() for g in o["images"][cam]]
                elif which == "e":
                    (l, r), _, _ = im.ft.decode_bag(data[lo:hi])
                    ev[0].append(l.tobytes()), ev[1].append(r.tobytes())
                else:
                    imu.append(im.ft.bag_side(data[lo:hi])[0])
        assert [b"".join(e) for e in ev] == [whole_e["events"][0].tobytes(), whole_e["events"][1].tobytes()], order
        assert np.concatenate(imu).tobytes() == whole_s["imu"].tobytes() and len(whole_s["imu"]) == 4, order
        assert images == [[g.tobytes() for g in whole_i["images"][cam]] for cam in range(2)] and len(images[0]) == 4, order
    # decode_reset clears the image state too; the topics stay
    im.fresh()
    im.check(data[:9000], tag="a payload waits")
    im.ft.decode_reset()
    im.w = I.ImageWalker(size=(W0, H0))
    im.check(data, tag="after decode_reset")
    im.ft.bag_set_topics()


def test_reserve_covers_the_scratch_and_a_second_call_allocates_nothing():
    W, H = 346, 260
    d = Im(W, H)
    try:
        pair = I.write_bag([image_msg(I.LEFT_IMAGE, 1, 3, "rgb8", W, H, 0, 75), image_msg(I.RIGHT_IMAGE, 1, 3, "rgb8", W, H, 0, 76)], per_chunk=2)[13:]
        tiny = I.write_bag([image_msg(I.LEFT_IMAGE, 1, 1, "mono8", W, H, 0, 77)])[13:]
        d.check(tiny, tag="first use", dst_space=FE.DEVICE)  # a handle that has decoded images before
        d.ft._hd.check(d.L.esvio_fe_reserve(d.h, 0, 0, 0))
        dst = [Mem(d.L, FE.DEVICE, W * H), Mem(d.L, FE.DEVICE, W * H)]
        msgs, info, buf = np.zeros(4, FE.BAG_IMAGE_DTYPE), FE.BagImageInfo(), np.frombuffer(pair, np.uint8)
        a0, mem0 = d.ft.latency_stats()["allocs"], d.ft.device_memory()[0]
        for _ in range(2):
            ptrs = (C.c_void_p * 2)(dst[0].p.value, dst[1].p.value)
            assert d.L.esvio_fe_decode_bag_images(d.h, FE._p(buf), len(buf), 0, C.byref(ptrs), C.byref((C.c_size_t * 2)(1, 1)), FE.DEVICE, FE._p(msgs), 4,
                                                  C.byref(info)) == 0
            assert (info.cam[0].images, info.cam[1].images) == (1, 1)
        assert d.ft.latency_stats()["allocs"] == a0 and d.ft.device_memory()[0] == mem0
        for m in dst:
            m.free()
        d.fresh()
        d.ft.decode_bag_images(pair)  # a host dst's images grow on first use; the second call of the size allocates nothing
        a1 = d.ft.latency_stats()["allocs"]
        d.ft.decode_bag_images(pair)
        assert d.ft.latency_stats()["allocs"] == a1
    finally:
        d.close()


# ---- tracking --------------------------------------------------------------------------------------------------------------
W, H = 346, 260


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


@pytest.fixture(scope="module")
def frames():
    s = ImageStream(W, H, velocity=(3, -2), disparity=9, seed=8)
    return [s.next_frame() for _ in range(5)]


@pytest.mark.parametrize("equalize", [0, 1])
def test_device_images_track_bit_identically_to_the_host_call(frames, equalize):
    kw = dict(max_cnt=120, min_dist=20, flow_back=1, equalize=equalize)
    a, b = FE.FeatureTracker(FE.make_config(W, H, **kw)), FE.FeatureTracker(FE.make_config(W, H, **kw))
    pool = Mem(b._hd.L, FE.DEVICE, 2 * W * H + 8)
    try:
        for k, (left, right, t) in enumerate(frames):
            pool.put(np.concatenate([np.zeros(3, np.uint8), left.reshape(-1), right.reshape(-1)]))  # (the images lie off every boundary)
            mono = k == 3  # img_right NULL
            a.trackImage(t, left, None if mono else right, k % 3 != 2)
            b.trackImage(t, pool.p.value + 3, None if mono else pool.p.value + 3 + W * H, k % 3 != 2, device=True)
            assert results(a) == results(b), (equalize, k)
        assert len(a.ids) > 30 and len(a.ids_right) > 10
    finally:
        pool.free()
        a.close()
        b.close()


def test_a_bag_of_5_stereo_rgb8_frames_decoded_paired_and_tracked_on_the_device_equals_the_oracle_on_the_loops_images(oracle, frames):
    messages = []
    for k, (left, right, t) in enumerate(frames):
        stamp = (int(t), int(round((t - int(t)) * 1e9)))
        for topic, g, pad in ((I.LEFT_IMAGE, left, 7), (I.RIGHT_IMAGE, right, 1)):
            rgb = np.repeat(g.reshape(H, W, 1), 3, axis=2).astype(np.int16)  # a colour image whose gray is not one of its channels
            rgb[..., 0] = np.clip(rgb[..., 0] + 9, 0, 255)
            rgb[..., 2] = np.clip(rgb[..., 2] - 11, 0, 255)
            data = I.rows(rgb.astype(np.uint8).reshape(H, 3 * W), 3 * W + pad)
            messages.append((topic, stamp, I.image_message(k, stamp if topic == I.LEFT_IMAGE else (stamp[0], stamp[1] + 500), H, W, "rgb8", 3 * W + pad, data)))
    messages[2], messages[3] = messages[3], messages[2]  # the right image first once
    bag = I.write_bag(messages, per_chunk=3)
    loop = I.decode(bag, size=(W, H))
    kw = dict(max_cnt=120, min_dist=20, flow_back=1)
    ft = FE.FeatureTracker(FE.make_config(W, H, **kw))
    tr = oracle.Tracker(oracle.make_config(W, H, **kw))
    try:
        ft.bag_set_image_topics(*I.IMAGE_TOPICS)
        (dl, dr), table, info = ft.decode_bag_images(bag[13:], device=True)
        assert table.tobytes() == loop["table"].tobytes() and (info.cam[0].images, info.cam[1].images) == (5, 5)
        pairs = StereoImageTrackerNode.pair_images(table)
        assert len(pairs) == 5
        for k, (ml, mr, t) in enumerate(pairs):
            assert t == float(ml["stamp_sec"]) + 1e-9 * float(ml["stamp_nsec"])
            ft.trackImage(t, dl.image(int(ml["index"])), dr.image(int(mr["index"])), k % 3 != 2, device=True)
            r = tr.track_image(t, loop["images"][0][int(ml["index"])], loop["images"][1][int(mr["index"])], k % 3 != 2)
            assert np.array_equal(ft.ids, r.ids) and np.array_equal(ft.track_cnt, r.track_cnt) and np.array_equal(ft.ids_right, r.ids_right), k
            for name in ("cur_pts", "cur_un_pts", "pts_velocity", "cur_right_pts", "cur_un_right_pts", "right_pts_velocity"):
                assert np.array_equal(getattr(ft, name), getattr(r, name)), (k, name)
        assert len(ft.ids) > 30 and len(ft.ids_right) > 10
        assert np.array_equal(dl.download(), np.stack(loop["images"][0]))
        dl.free()
        dr.free()
    finally:
        ft.close()


def test_esvio_mode_an_event_handle_and_an_image_handle_fed_the_same_4099_byte_chunks(frames):
    """one bag with events on two topics, IMU and images on two topics; every modality equals what its loop gives"""
    st = SceneStream(W=W, H=H, rate=3e5, seed=7)
    rng = np.random.default_rng(5)
    messages, recs = [], []
    for k, (left, right, t) in enumerate(frames[:3]):
        el, er, _ = st.next_batch()
        stamp = (int(el["sec"][-1]), int(el["nsec"][-1]))
        recs.append((el, er))
        for topic, ev in ((B.LEFT, el), (B.RIGHT, er)):
            messages.append((topic, stamp, B.event_array(k, stamp, B.wire_events(ev["x"], ev["y"], ev["sec"], ev["nsec"], ev["polarity"]), height=H, width=W)))
        messages.append((B.IMU, stamp, B.imu_message(k, stamp, rng.normal(0, 1, 3), rng.normal(0, 9, 3))))
        messages.append((I.LEFT_IMAGE, stamp, I.image_message(k, stamp, H, W, "mono8", W + 2, I.rows(left, W + 2))))
        messages.append((I.RIGHT_IMAGE, stamp, I.image_message(k, stamp, H, W, "8UC1", W, I.rows(right, W))))
    bag = I.write_bag(messages, per_chunk=3)
    data = bag[13:]
    loop_e, loop_s, loop_i = B.decode(bag), B.decode(bag, "side"), I.decode(bag, size=(W, H))
    assert loop_e["events"][0].tobytes() == b"".join(l.tobytes() for l, _ in recs) and len(loop_s["imu"]) == 3
    assert np.array_equal(loop_i["images"][0][1], frames[1][0]) and np.array_equal(loop_i["images"][1][2], frames[2][1])
    kw = dict(max_cnt=120, min_dist=20)
    ev_h, im_h = FE.FeatureTracker(FE.make_config(W, H, **kw)), FE.FeatureTracker(FE.make_config(W, H, flow_back=1, **kw))
    ev_a, im_a = FE.FeatureTracker(FE.make_config(W, H, **kw)), FE.FeatureTracker(FE.make_config(W, H, flow_back=1, **kw))
    try:
        ev_h.bag_set_topics(*B.TOPICS)
        im_h.bag_set_image_topics(*I.IMAGE_TOPICS)  # (no event topic is set on the image handle)
        ev, imu, images, rows, table = [[], []], [], [[], []], [], []
        for lo in range(0, len(data), 4099):
            chunk = data[lo:lo + 4099]
            (l, r), m, _ = ev_h.decode_bag(chunk)
            ev[0].append(l), ev[1].append(r), rows.append(m)
            imu.append(ev_h.bag_side(chunk)[0])
            (gl, gr), t, _ = im_h.decode_bag_images(chunk)
            images[0] += list(gl)
            images[1] += list(gr)
            table.append(t)
        ev = [np.frombuffer(b"".join(e.tobytes() for e in cam_ev), EVENT_DTYPE) for cam_ev in ev]  # (bytes: concatenate drops the records' padding)
        assert [e.tobytes() for e in ev] == [e.tobytes() for e in loop_e["events"]]
        assert np.concatenate(rows).tobytes() == loop_e["messages"].tobytes() and np.concatenate(imu).tobytes() == loop_s["imu"].tobytes()
        t_all = np.concatenate(table)
        assert [tuple(int(r[n]) for n in t_all.dtype.names[:-1]) for r in t_all] == [tuple(int(r[n]) for n in t_all.dtype.names[:-1]) for r in loop_i["table"]]
        for cam in range(2):
            assert len(images[cam]) == 3 and all(np.array_equal(g, w) for g, w in zip(images[cam], loop_i["images"][cam]))
        # each tracker on what its handle decoded equals a tracker on the loops' records and images alone
        msgs = np.concatenate(rows)
        for k in range(3):
            ml, mr = msgs[msgs["cam"] == 0][k], msgs[msgs["cam"] == 1][k]
            mine = [ev[0][int(ml["first"]):int(ml["first"] + ml["count"])], ev[1][int(mr["first"]):int(mr["first"] + mr["count"])]]
            t1 = float(event_times(recs[k][0][-1:])[0])
            ev_h.trackEvent(t1, mine[0], mine[1], True)
            ev_a.trackEvent(t1, recs[k][0], recs[k][1], True)
            assert results(ev_h) == results(ev_a), k
            im_h.trackImage(frames[k][2], images[0][k], images[1][k], True)
            im_a.trackImage(frames[k][2], frames[k][0], frames[k][1], True)
            assert results(im_h) == results(im_a), k
        assert len(ev_a.ids) > 0 and len(im_a.ids) > 30
    finally:
        for f in (ev_h, im_h, ev_a, im_a):
            f.close()
