"""GPU: esvio_fe_decode_aedat_frames and esvio_fe_convert_frame16 against the sequential reading tests/aedat_frame_ref.py.
Integers only: every byte of every gray image, every row of the frame table and every info field are compared for
equality, with guard bytes around every destination and behind the last table row."""
import ctypes as C
import itertools

import numpy as np
import pytest

import aedat_frame_ref as F
import aedat_ref as A
from esvio_amd import frontend as FE
from esvio_amd.node import StereoImageTrackerNode
from esvio_amd.synth import ImageStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
W0, H0 = 43, 42  # the smallest handle there is, with an odd width: 1806 pixels, so a call's second image begins off a dword
INFO = ("frames", "invalid", "bad", "frame_packets", "other_packets")


class Mem:
    """memory of the library's runtime: device, or page-locked host"""

    def __init__(self, L, space, n):
        self.L, self.space, self.n, self.p = L, space, n, C.c_void_p()
        assert L.esvio_fe_mem_alloc(space, max(n, 1), C.byref(self.p)) == 0
        self.hip = C.CDLL("libamdhip64.so")

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8)
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


class Fr:
    """a handle and the reading's frame walkers, one per camera, advanced together"""

    def __init__(self, W=W0, H=H0, **kw):
        self.ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=kw.pop("max_cnt", 40), **kw))
        self.W, self.H, self.L, self.h = W, H, self.ft._hd.L, self.ft._hd.h
        self.fresh()

    def fresh(self):
        self.ft.decode_reset()
        self.w = [F.FrameWalker((self.W, self.H)), F.FrameWalker((self.W, self.H))]

    def close(self):
        self.ft.close()

    def error(self):
        return self.L.esvio_fe_last_error(self.h).decode()

    def call(self, data, cam=0, dst_cap=None, frames_cap=None, dst_space=FE.HOST, flags=0, lead=0, t_offset_ns=0):
        """one esvio_fe_decode_aedat_frames call -> (rc, the dst_cap images as bytes, the table rows, the info); dst lies
        `lead` bytes behind a 16-byte boundary; the reading does not move"""
        wh = self.W * self.H
        buf = np.frombuffer(data, np.uint8)
        most = len(data) // (2 * wh) + 1
        dst_cap = most if dst_cap is None else dst_cap
        frames_cap = most if frames_cap is None else frames_cap
        info = FE.AedatFrameInfo()
        room = np.full(16 + lead + wh * dst_cap + 32, GUARD, np.uint8)
        at = ((-room.ctypes.data) & 15) + lead
        rows = np.zeros(frames_cap + 1, FE.AEDAT_FRAME_DTYPE)
        rows.view(np.uint8)[:] = GUARD
        dev = None
        if dst_space == FE.DEVICE:
            dev = Mem(self.L, FE.DEVICE, len(room)).put(room)
            at = lead  # (the runtime's allocations are 16-byte aligned)
            assert dev.p.value % 16 == 0
            ptr = dev.p.value + at
        else:
            ptr = room.ctypes.data + at
        rc = self.L.esvio_fe_decode_aedat_frames(self.h, cam, FE._p(buf) if len(buf) else None, len(buf), t_offset_ns, flags, C.c_void_p(ptr), dst_cap,
                                                 dst_space, FE._p(rows), frames_cap, C.byref(info))
        if dev:
            room = dev.get()
            dev.free()
        assert (room[:at] == GUARD).all() and (room[at + wh * dst_cap:] == GUARD).all(), "bytes around dst touched"
        assert (rows[frames_cap:].view(np.uint8) == GUARD).all(), "rows beyond frames_cap touched"
        return rc, room[at:at + wh * dst_cap], rows[:frames_cap], info

    def check(self, data, cam=0, dst_space=FE.HOST, tag=None, exact_cap=False, lead=0, flags=0, t_offset_ns=0):
        """a call that succeeds equals the reading, which advances with it -> the reading's result"""
        w, o = self.w[cam].feed(data, t_offset_ns, flags)
        n = len(o["images"])
        rc, got, rows, info = self.call(data, cam, n if exact_cap else None, n if exact_cap else None, dst_space, flags, lead, t_offset_ns)
        assert rc == 0, (tag, rc, self.error())
        self.w[cam] = w
        wh = self.W * self.H
        assert tuple(getattr(info, k) for k in INFO) == (n,) + tuple(o[k] for k in INFO[1:]), tag
        t = o["table"]
        want = (int(t["stamp_sec"][0]), int(t["stamp_nsec"][0]), int(t["stamp_sec"][-1]), int(t["stamp_nsec"][-1])) if n else (0, 0, 0, 0)
        assert (info.first_sec, info.first_nsec, info.last_sec, info.last_nsec) == want, tag
        for k, img in enumerate(o["images"]):
            g = got[k * wh:(k + 1) * wh].reshape(self.H, self.W)
            if not np.array_equal(g, img):
                y, x = np.argwhere(g != img)[0]
                raise AssertionError((tag, k, "first differing pixel", int(x), int(y), int(g[y, x]), int(img[y, x])))
        assert (got[n * wh:] == GUARD).all(), (tag, "bytes behind the last image touched")
        assert rows[:n].tobytes() == t.tobytes(), tag
        assert (rows[n:].view(np.uint8) == GUARD).all(), (tag, "rows behind the last frame touched")
        return o


@pytest.fixture(scope="module")
def fr():
    d = Fr()
    yield d
    d.close()


def frame(k, channels, w=W0, h=H0, **kw):
    return F.frame_event(F.test_pixels(w, h, channels, 40 + k), w, h, channels, ts=kw.pop("ts", (1000 * k, 1000 * k + 900, 1000 * k + 100, 1000 * k + 601)), **kw)


def stream(n, w=W0, h=H0, first=0):
    """n frames, mono and colour in turn, each in a packet of its own between a polarity and an IMU6 packet"""
    parts = []
    for k in range(first, first + n):
        parts += [A.packet(A.POLARITY, [A.polarity(k, k, k & 1, 1000 * k)]), F.frame_packet([frame(k, 1 if k % 2 == 0 else 3, w, h)], overflow=k % 2),
                  A.packet(A.IMU6, [A.imu6(1000 * k + 5, (0.1, 0.2, 0.3), (1, 2, 3))])]
    return b"".join(parts)


# ---- the conversion alone --------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (3, 5), (43, 42), (8192, 2))  # (width, height)


def test_convert_frame16_equals_the_reading_at_every_shape_channel_count_offset_and_space(fr):
    L, h = fr.L, fr.h
    sources = []
    for (w, hh), ch in itertools.product(SHAPES, (1, 3)):
        v = F.test_pixels(w, hh, ch, 100 + w + ch)
        sources.append((w, hh, ch, v, F.convert_fast(v, hh, w, ch)))
    for w, hh, ch, v, want in sources[:4]:  # (the loop itself, where it is short)
        assert np.array_equal(want, F.convert(v, hh, w, ch))
    room = max(s[3].nbytes for s in sources) + 64
    src_mem = Mem(L, FE.DEVICE, room)
    dst_mem = Mem(L, FE.DEVICE, max(s[0] * s[1] for s in sources) + 64)
    n = 0
    for (w, hh, ch, v, want), off in itertools.product(sources, range(8)):
        staged = np.full(room, 0xEE, np.uint8)
        staged[2 * off:2 * off + v.nbytes] = v.view(np.uint8)
        src_mem.put(staged)
        for src_dev, dst_dev in ((True, True), (True, False), (False, True), (False, False)):
            if not src_dev and off > 1:
                continue  # (a host source is copied first: its place does not reach the kernel)
            n += 1
            host = staged[2 * off:2 * off + v.nbytes].copy().view("<u2")
            sp, space = (src_mem.p.value + 2 * off, FE.DEVICE) if src_dev else (host.ctypes.data, FE.HOST)
            tag = (w, hh, ch, off, src_dev, dst_dev)
            lead = 16 + off % 4
            if dst_dev:
                dst_mem.put(np.full(dst_mem.n, GUARD, np.uint8))
                rc = L.esvio_fe_convert_frame16(h, C.c_void_p(sp), space, hh, w, ch, C.c_void_p(dst_mem.p.value + lead), FE.DEVICE)
                back = dst_mem.get()
            else:
                back = np.full(dst_mem.n, GUARD, np.uint8)
                rc = L.esvio_fe_convert_frame16(h, C.c_void_p(sp), space, hh, w, ch, C.c_void_p(back.ctypes.data + lead), FE.HOST)
            assert rc == 0, (tag, fr.error())
            got = back[lead:lead + w * hh].reshape(hh, w)
            if not np.array_equal(got, want):
                y, x = np.argwhere(got != want)[0]
                raise AssertionError((tag, "first differing pixel", int(x), int(y), int(got[y, x]), int(want[y, x])))
            assert (back[:lead] == GUARD).all() and (back[lead + w * hh:] == GUARD).all(), (tag, "bytes around dst touched")
    assert n == len(SHAPES) * 2 * (8 * 2 + 2 * 2)
    # the Python mirror: host in, host out and device out
    w, hh, ch, v, want = sources[5]
    assert np.array_equal(fr.ft.convert_frame16(v, hh, w, ch), want)
    dev = fr.ft.convert_frame16(v, hh, w, ch, device=True)
    assert np.array_equal(dev.download()[0], want) and dev.image(0) == dev.ptr.value
    dev.free()
    # the argument errors, before any device work
    px = np.zeros(64, np.uint16)
    ok = dict(src=px.ctypes.data, ss=FE.HOST, h=2, w=3, ch=3, dst=px.ctypes.data, ds=FE.HOST)
    for bad in (dict(src=None), dict(dst=None), dict(ss=5), dict(ds=-1), dict(h=0), dict(w=0), dict(h=8193), dict(w=8193), dict(ch=0), dict(ch=2),
                dict(ch=4), dict(src=px.ctypes.data + 1)):
        a = dict(ok, **bad)
        assert L.esvio_fe_convert_frame16(h, a["src"], a["ss"], a["h"], a["w"], a["ch"], a["dst"], a["ds"]) == -1, bad
    src_mem.free()
    dst_mem.free()


# ---- the frame call --------------------------------------------------------------------------------------------------------
def test_one_two_and_three_frames_per_call_at_every_dst_offset_in_device_and_host_memory(fr):
    for n, lead, dst_space in itertools.product((1, 2, 3), range(4), (FE.DEVICE, FE.HOST)):
        fr.fresh()
        o = fr.check(stream(n), cam=n % 2, dst_space=dst_space, tag=(n, lead, dst_space), exact_cap=lead % 2 == 0, lead=lead)
        assert [r["channels"] for r in o["rows"]] == [1, 3, 1][:n] and (W0 * H0) % 4 != 0
    # the Python mirror
    fr.fresh()
    img, table, info = fr.ft.decode_aedat_frames(0, stream(3))
    want = F.decode(stream(3), size=(W0, H0))
    assert np.array_equal(img, np.stack(want["images"])) and table.tobytes() == want["table"].tobytes() and info.frames == 3
    fr.fresh()
    dev, table, info = fr.ft.decode_aedat_frames(1, stream(2), device=True)
    assert np.array_equal(dev.download(), np.stack(want["images"][:2])) and dev.n == 2
    dev.free()


def test_a_mono_and_a_colour_frame_at_346x260_in_one_launch():
    d = Fr(346, 260)
    try:
        data = stream(2, 346, 260)
        d.ft.set_profiling(True)
        d.ft.reset_kernel_stats()
        o = d.check(data, dst_space=FE.DEVICE, tag="346x260", exact_cap=True, lead=3)
        assert [r["channels"] for r in o["rows"]] == [1, 3] and (346 * 260) % 16 != 0
        ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        d.ft._hd.check(d.L.esvio_fe_aedat_frame_kernel_stats(d.h, C.byref(ms), C.byref(n), C.byref(b)))
        assert n.value == 1 and b.value == 346 * 260 * (3 + 7)  # one launch for both frames
        d.ft.set_profiling(False)
        d.fresh()
        d.check(data, dst_space=FE.HOST, tag="346x260, host dst")
    finally:
        d.close()


def test_a_frame_cut_across_two_and_across_three_calls(fr):
    s = stream(3)
    whole = F.decode(s, size=(W0, H0))
    ends = whole["ends"]
    first_pixel = [e - W0 * H0 * 2 * int(r["channels"]) for e, r in zip(ends, whole["rows"])]
    rng = np.random.default_rng(14)
    for it in range(12):
        k = it % 3
        inside = sorted(int(c) for c in rng.integers(first_pixel[k] - 40, ends[k], 2 if it % 2 else 1))  # in the head or in the pixels
        cuts = [0] + inside + [len(s)]
        fr.fresh()
        n = 0
        for lo, hi in zip(cuts, cuts[1:]):
            n += len(fr.check(s[lo:hi], dst_space=FE.DEVICE if it % 4 < 2 else FE.HOST, tag=(it, cuts, lo), exact_cap=it % 3 == 0, lead=it % 4)["rows"])
        assert n == 3
    # the two cameras' walkers and carries are apart: each cut inside a frame, the calls interleaved
    fr.fresh()
    a, b = stream(2), stream(2, first=1)
    ca, cb = F.decode(a)["ends"][0] - 100, F.decode(b)["ends"][0] - 3000
    fr.check(a[:ca], cam=0, tag="left, first")
    fr.check(b[:cb], cam=1, tag="right, first")
    assert len(fr.check(a[ca:], cam=0, tag="left, second", dst_space=FE.DEVICE)["rows"]) == 2
    assert len(fr.check(b[cb:], cam=1, tag="right, second", dst_space=FE.DEVICE)["rows"]) == 2
    # decode_reset clears the frame walker too
    fr.check(a[:ca], cam=0, tag="a frame waits")
    fr.fresh()
    assert len(fr.check(a, cam=0, tag="after decode_reset")["rows"]) == 2


def test_validity_in_both_modes_with_an_invalid_frame_between_valid_ones(fr):
    s = F.frame_packet([frame(0, 1), frame(1, 3, valid=0), frame(2, 1)], capacity=4) + F.frame_packet([frame(3, 3, valid=0)]) + stream(1, first=4)
    for flags, slots, dst_space in ((0, [0, 2, 0], FE.DEVICE), (F.KEEP_INVALID, [0, 1, 2, 0, 0], FE.DEVICE), (F.KEEP_INVALID, [0, 1, 2, 0, 0], FE.HOST)):
        fr.fresh()
        o = fr.check(s, dst_space=dst_space, flags=flags, tag=("validity", flags), exact_cap=True, lead=1, t_offset_ns=10 ** 12 + 1)
        assert [r["slot"] for r in o["rows"]] == slots and o["invalid"] == (0 if flags else 2)


def test_the_caps_one_too_small_report_the_need_store_nothing_and_leave_the_state(fr):
    s = stream(3)
    cut = F.decode(s, size=(W0, H0))["ends"][0] - 500  # the first frame waits but for 500 bytes: the failed calls must leave it waiting
    for dst_space, (dst_cap, frames_cap) in itertools.product((FE.HOST, FE.DEVICE), ((2, 3), (3, 2))):
        fr.fresh()
        fr.check(s[:cut], tag="lead")
        rc, got, rows, info = fr.call(s[cut:], 0, dst_cap, frames_cap, dst_space)
        assert rc == -1 and info.frames == 3 and "as it was" in fr.error() and " 3 frames" in fr.error()
        assert (got == GUARD).all() and (rows.view(np.uint8) == GUARD).all()
        assert len(fr.check(s[cut:], dst_space=dst_space, exact_cap=True, tag="exact room")["rows"]) == 3
    fr.fresh()
    rc, _, _, info = fr.call(b"")
    assert rc == 0 and info.frames == 0


def test_a_bad_stamp_a_refused_channel_number_and_a_refused_size_in_the_middle_of_a_chunk(fr):
    good = stream(3)
    cut = F.decode(good, size=(W0, H0))["ends"][1] - 700  # the second frame waits but for 700 bytes
    two = F.decode(good, size=(W0, H0))["ends"][1]
    cases = {
        "a BAD stamp": (F.frame_packet([frame(7, 1, ts=(0, 0, -50, 10))]), "stamp outside"),
        "2 channels": (F.frame_packet([F.frame_event(F.test_pixels(W0, H0, 2, 1), W0, H0, 2)]), "2 channels"),
        "another size": (F.frame_packet([F.frame_event(F.test_pixels(W0 + 1, H0, 1, 1), W0 + 1, H0, 1)]), "%d x %d" % (W0 + 1, H0)),
        "a type-2 header with eventTSOffset 4": (F.frame_packet([frame(7, 1)], ts_offset=4), "eventTSOffset"),
    }
    for (name, (data, names)), dst_space in itertools.product(cases.items(), (FE.DEVICE, FE.HOST)):
        fr.fresh()
        fr.check(good[:cut], tag="lead")
        chunk = good[cut:two] + data + good[two:]  # the failure between the second and the third frame
        with pytest.raises((F.Malformed, F.Bad)):
            fr.w[0].feed(chunk)
        rc, got, rows, info = fr.call(chunk, dst_space=dst_space)
        assert rc == -1 and names in fr.error() and "as it was" in fr.error(), (name, fr.error())
        assert (got == GUARD).all() and (rows.view(np.uint8) == GUARD).all(), name
        assert info.bad == (1 if name == "a BAD stamp" else 0), name
        o = fr.check(good[cut:], dst_space=dst_space, tag=(name, "after the failure"))  # the correct bytes behind it give the whole
        assert len(o["rows"]) == 2
    # the argument errors, before any device work
    info, buf = FE.AedatFrameInfo(), np.frombuffer(good, np.uint8)
    dst, rows = np.zeros(3 * W0 * H0, np.uint8), np.zeros(4, FE.AEDAT_FRAME_DTYPE)

    def call(**k):
        return fr.L.esvio_fe_decode_aedat_frames(fr.h, k.get("cam", 0), k.get("bytes", FE._p(buf)), len(buf), k.get("off", 0), k.get("flags", 0),
                                                 k.get("dst", FE._p(dst)), 3, k.get("space", FE.HOST), k.get("rows", FE._p(rows)), 4, C.byref(info))
    fr.fresh()
    for bad in (dict(cam=2), dict(cam=-1), dict(flags=2), dict(bytes=None), dict(dst=None), dict(rows=None), dict(space=7), dict(off=2 ** 62 + 1)):
        assert call(**bad) == -1, bad
    assert call() == 0 and info.frames == 3
    fr.fresh()
    fr.check(good, tag="after the argument errors")


def test_reserve_covers_the_scratch_and_a_second_call_allocates_nothing():
    W, H = 346, 260
    d = Fr(W, H)
    try:
        rgb = F.frame_packet([frame(1, 3, W, H)])
        d.check(F.frame_packet([frame(0, 1, W, H)]), tag="first use", dst_space=FE.DEVICE)  # a handle that has decoded frames before
        d.ft._hd.check(d.L.esvio_fe_reserve(d.h, 0, 0, 0))
        dst = Mem(d.L, FE.DEVICE, W * H)
        rows, info, buf = np.zeros(2, FE.AEDAT_FRAME_DTYPE), FE.AedatFrameInfo(), np.frombuffer(rgb, np.uint8)
        a0, mem0 = d.ft.latency_stats()["allocs"], d.ft.device_memory()[0]
        for _ in range(2):
            assert d.L.esvio_fe_decode_aedat_frames(d.h, 0, FE._p(buf), len(buf), 0, 0, dst.p, 1, FE.DEVICE, FE._p(rows), 2, C.byref(info)) == 0
            assert info.frames == 1
        assert d.ft.latency_stats()["allocs"] == a0 and d.ft.device_memory()[0] == mem0
        dst.free()
        two = stream(2, W, H)
        d.fresh()
        d.ft.decode_aedat_frames(0, two)  # two frames and a host dst grow the scratch on first use; the second call of the size allocates nothing
        a1 = d.ft.latency_stats()["allocs"]
        d.ft.decode_aedat_frames(0, two)
        assert d.ft.latency_stats()["allocs"] == a1
    finally:
        d.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def polarity_records(x, y, p, ts):
    x, y, p, ts = (np.asarray(a, np.int64) for a in (x, y, p, ts))
    r = np.zeros((len(x), 2), "<u4")
    r[:, 0] = 1 | p << 1 | y << 2 | x << 17
    r[:, 1] = ts
    return r.tobytes()


def test_a_davis_stream_per_camera_events_on_an_event_handle_frames_decoded_paired_and_tracked_on_the_device(oracle):
    """one synthetic stream per camera at 43x42 — polarity, IMU6 and frame packets interleaved —: the event call on an event
    handle equals tests/aedat_ref.py's reading as before, the frame call on an image handle equals the frame reading, and
    the frames tracked where they lie on the device equal the oracle on the reading's images"""
    src = ImageStream(W0, H0, velocity=(1, 1), disparity=2, seed=8)
    rng = np.random.default_rng(21)
    base_ns = 100 * 10 ** 9
    streams = [[], []]
    for k in range(6):
        left, right, t = src.next_frame()
        t_us = int(round((t - 100.0) * 10 ** 6))
        for cam, g in enumerate((left, right)):
            wide = (g.astype(np.uint16) << 8) | rng.integers(1, 256, g.shape).astype(np.uint16)  # non-zero low bytes
            if k % 2:  # a colour frame whose gray is not one of its channels' high bytes
                hi = np.repeat(g.reshape(H0, W0, 1), 3, axis=2).astype(np.int16)
                hi[..., 0] = np.clip(hi[..., 0] + 9, 0, 255)
                hi[..., 2] = np.clip(hi[..., 2] - 11, 0, 255)
                wide = (hi.astype(np.uint16) << 8) | rng.integers(1, 256, hi.shape).astype(np.uint16)
            n = 50
            ts = t_us + np.sort(rng.integers(0, 40_000, n))
            ev = polarity_records(rng.integers(0, W0, n), rng.integers(0, H0, n), rng.integers(0, 2, n), ts)
            # the exposure around t_us (+ 400 us for the right camera: the node pairs within 1 s and takes the left stamp)
            mid = t_us + 400 * cam
            streams[cam] += [A.packet(A.POLARITY, [ev], number=n, capacity=n + 3),
                             A.packet(A.IMU6, [A.imu6(int(ts[-1]), rng.normal(0, 1, 3), rng.normal(0, 50, 3))]),
                             F.frame_packet([F.frame_event(wide.reshape(-1), W0, H0, 3 if k % 2 else 1, ts=(mid - 3000, mid + 3000, mid - 2000, mid + 2000))])]
    data = [b"".join(s) for s in streams]
    kw = dict(max_cnt=40, min_dist=4, flow_back=1)
    ev_h, im_h = FE.FeatureTracker(FE.make_config(W0, H0, max_cnt=40)), FE.FeatureTracker(FE.make_config(W0, H0, **kw))
    tr = oracle.Tracker(oracle.make_config(W0, H0, **kw))
    held = []
    try:
        tables, images, want = [], [], []
        for cam in range(2):
            # the event call and the side call as today, in 4099-byte chunks that also go through the frame call
            ev, imu, rows, imgs = [], [], [], []
            for lo in range(0, len(data[cam]), 4099):
                chunk = data[cam][lo:lo + 4099]
                ev.append(ev_h.decode_aedat(cam, chunk, t_offset_ns=base_ns)[0].tobytes())
                imu.append(ev_h.aedat_side(cam, chunk, t_offset_ns=base_ns)[0])
                dev, t, info = im_h.decode_aedat_frames(cam, chunk, t_offset_ns=base_ns, device=True)
                held.append(dev)
                rows += [(r, dev) for r in t]
            loop_e, _ = A.decode_fast(data[cam], base_ns)
            assert b"".join(ev) == loop_e.tobytes() and len(loop_e) == 300 and sum(len(i) for i in imu) == 6
            loop_f = F.decode(data[cam], size=(W0, H0), t_offset_ns=base_ns)
            assert len(rows) == 6 and [r.tobytes()[:-8] for r, _ in rows] == [r.tobytes()[:-8] for r in loop_f["table"]]
            tables.append(rows)
            want.append(loop_f["images"])
        # pair as the node does: one table per camera, merged with a cam column; `index` there is the row's place in its camera's list
        per_cam = []
        for rows in tables:
            t = np.zeros(len(rows), FE.AEDAT_FRAME_DTYPE)
            for k, (r, _) in enumerate(rows):
                t[k] = r
            t["index"] = np.arange(len(t))
            per_cam.append(t)
        pairs = StereoImageTrackerNode.pair_images(StereoImageTrackerNode.merge_frame_tables(*per_cam))
        assert len(pairs) == 6
        for k, (ml, mr, t) in enumerate(pairs):
            il, ir = int(ml["index"]), int(mr["index"])
            assert (il, ir) == (k, k) and t == float(ml["stamp_sec"]) + 1e-9 * float(ml["stamp_nsec"])
            (rl, dl), (rr, dr) = tables[0][il], tables[1][ir]
            assert np.array_equal(dl.download()[int(rl["index"])], want[0][il]) and np.array_equal(dr.download()[int(rr["index"])], want[1][ir])
            im_h.trackImage(t, dl.image(int(rl["index"])), dr.image(int(rr["index"])), k % 3 != 2, device=True)
            r = tr.track_image(t, want[0][il], want[1][ir], k % 3 != 2)
            assert np.array_equal(im_h.ids, r.ids) and np.array_equal(im_h.track_cnt, r.track_cnt) and np.array_equal(im_h.ids_right, r.ids_right), k
            for name in ("cur_pts", "cur_un_pts", "pts_velocity", "cur_right_pts", "cur_un_right_pts", "right_pts_velocity"):
                assert np.array_equal(getattr(im_h, name), getattr(r, name)), (k, name)
        assert len(im_h.ids) > 0
    finally:
        for dev in held:
            dev.free()
        ev_h.close()
        im_h.close()
