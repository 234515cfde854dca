"""The sequential reading of the "AEDAT 3.1 frames" rule in include/esvio_fe.h, written from that text alone: plain loops
over Python integers, one byte string in, frames out — and a writer of frame packets on top of tests/aedat_ref.py's packet
writer.  Not part of the library.

A FrameWalker is one frame walker state of the rule (a handle has one per camera): feed() takes a chunk that may end
anywhere and returns what the chunk completes."""
import struct

import numpy as np

import aedat_ref as A
from esvio_amd.frontend import AEDAT_FRAME_DTYPE

FRAME = A.FRAME
KEEP_INVALID = A.KEEP_INVALID
HEAD = struct.Struct("<I8i")  # info, ts_startframe, ts_endframe, ts_startexposure, ts_endexposure, lengthX, lengthY, positionX, positionY
Malformed, Bad = A.Malformed, A.Bad


class Refused(A.Malformed):
    """refused by name: .value is what the message must name"""

    def __init__(self, what, value):
        super().__init__(what)
        self.value = value


# ---- the writer --------------------------------------------------------------------------------------------------------
def frame_event(pixels, length_x, length_y, channels=1, ts=(10, 40, 20, 30), valid=1, position=(0, 0), color_filter=0, roi=0, size=None):
    """one frame event: the head, the uint16 pixels (an array-like of length_x * length_y * channels values, or raw bytes),
    and 0xCD bytes up to `size` (None: none)"""
    info = (valid & 1) | (channels & 7) << 1 | (color_filter & 15) << 4 | (roi & 127) << 8
    body = pixels if isinstance(pixels, (bytes, bytearray)) else np.asarray(pixels, "<u2").tobytes()
    ev = HEAD.pack(info, ts[0], ts[1], ts[2], ts[3], length_x, length_y, position[0], position[1]) + bytes(body)
    if size is not None:
        ev = ev[:size] + b"\xcd" * max(size - len(ev), 0)
    return ev


def frame_packet(events, overflow=0, capacity=None, size=None, ts_offset=12, number=None):
    """a type-2 packet of frame events of one size (the largest event's, shorter ones padded with 0xCD)"""
    size = max(len(e) for e in events) if size is None else size
    events = [e[:size] + b"\xcd" * max(size - len(e), 0) for e in events]
    return A.packet(FRAME, events, overflow=overflow, capacity=capacity, size=size, ts_offset=ts_offset, number=number)


def test_pixels(length_x, length_y, channels, seed):
    """uint16 values whose low bytes are not zero and whose high bytes cover 0 and 255"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 65536, length_x * length_y * channels).astype("<u2")
    v[:4] = (0xFFFF, 0x00FF, 0x0100, 0xFF00)[:len(v[:4])]
    return v


# ---- the rule ----------------------------------------------------------------------------------------------------------
def gray(r, g, b):
    return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15


def convert(values, height, width, channels):
    """the pixel rule: uint16 values, row-major with the channels interleaved -> the gray image, pixel by pixel"""
    v = [int(x) >> 8 for x in values]
    out = np.zeros((height, width), np.uint8)
    for p in range(height * width):
        out[p // width, p % width] = v[p] if channels == 1 else gray(v[3 * p], v[3 * p + 1], v[3 * p + 2])
    return out


def convert_fast(values, height, width, channels):
    """the same integers with numpy, for images too large for the loop (checked against it in the tests)"""
    v = (np.asarray(values, "<u2").astype(np.int64) >> 8)
    if channels == 1:
        return v.reshape(height, width).astype(np.uint8)
    v = v.reshape(height * width, 3)
    return ((v[:, 0] * 9798 + v[:, 1] * 19235 + v[:, 2] * 3735 + (1 << 14)) >> 15).reshape(height, width).astype(np.uint8)


def mid_exposure(start, end):
    """ts_startexposure + (ts_endexposure - ts_startexposure) / 2, the division truncating toward zero"""
    d = end - start
    half = abs(d) // 2
    return start + (half if d >= 0 else -half)


class FrameWalker:
    def __init__(self, size=(0, 0)):
        self.size = size        # (width, height) the only size taken; (0, 0): any
        self.hdr = b""
        self.ev_size = self.overflow = 0
        self.events_left = 0    # frame events of the open type-2 packet still to come
        self.payload_left = 0
        self.slot = 0
        self.ev = b""           # the bytes of the open frame event that have come: the head, then the pixels
        self.ev_off = 0         # how many of the event's bytes have come
        self.emit = None        # the open event's row once its head is complete and it is emitted, else None
        self.pix_need = 0

    def copy(self):
        w = FrameWalker(self.size)
        w.__dict__.update(self.__dict__)
        return w

    def feed(self, chunk, t_offset_ns=0, flags=0):
        """the chunk through a COPY of the state; returns (state after, result dict).  Raises Malformed / Refused / Bad:
        the caller's state is then as it was."""
        w = self.copy()
        out = {"images": [], "rows": [], "pixels": [], "invalid": 0, "bad": 0, "frame_packets": 0, "other_packets": 0, "ends": []}
        pos, n = 0, len(chunk)
        while pos < n:
            if w.payload_left == 0:
                take = min(28 - len(w.hdr), n - pos)
                w.hdr += chunk[pos:pos + take]
                pos += take
                if len(w.hdr) < 28:
                    break
                etype, _, size, ts_offset, overflow, capacity, number, _ = A.HEADER.unpack(w.hdr)
                A.check_header(etype, size, ts_offset, capacity, number)
                if etype == FRAME and (size < 36 or (size - 36) % 2 or ts_offset != 12):
                    raise Malformed("a type-2 header")
                w.hdr = b""
                w.ev_size, w.overflow = size, overflow
                w.events_left = number if etype == FRAME else 0
                w.payload_left = capacity * size
                w.slot = 0
                if etype == FRAME:
                    out["frame_packets"] += 1
                elif etype not in A.SIZES:
                    out["other_packets"] += 1
            elif w.events_left:
                # the head's last byte decides the event, the last pixel byte emits it, the rest is passed over
                in_head, in_pixels = w.ev_off < 36, w.emit is not None and w.ev_off < 36 + w.pix_need
                upto = 36 if in_head else 36 + w.pix_need if in_pixels else w.ev_size
                take = min(upto - w.ev_off, n - pos)
                if in_head or in_pixels:
                    w.ev += chunk[pos:pos + take]
                w.ev_off += take
                w.payload_left -= take
                pos += take
                if in_head and w.ev_off == 36:
                    w._head(t_offset_ns, flags, out)
                if in_pixels and w.ev_off == 36 + w.pix_need:
                    row = dict(w.emit, index=len(out["rows"]))
                    values = np.frombuffer(w.ev, "<u2", w.pix_need // 2, 36)
                    out["rows"].append(row)
                    out["pixels"].append(w.ev[36:])
                    out["images"].append(convert_fast(values, row["length_y"], row["length_x"], row["channels"]))
                    out["ends"].append(pos)
                    w.emit = None
                if w.ev_off == w.ev_size:
                    w.ev, w.ev_off, w.emit, w.pix_need = b"", 0, None, 0
                    w.events_left -= 1
                    w.slot += 1
            else:
                skip = min(w.payload_left, n - pos)
                pos += skip
                w.payload_left -= skip
        if out["bad"]:
            raise Bad(out["bad"])
        out["table"] = table(out["rows"])
        return w, out

    def _head(self, t_offset_ns, flags, out):
        info, ts_sf, ts_ef, ts_se, ts_ee, lx, ly, px, py = HEAD.unpack(self.ev)
        self.emit, self.pix_need = None, 0
        if not (info & 1) and not (flags & KEEP_INVALID):
            out["invalid"] += 1
            return
        ch = (info >> 1) & 7
        if lx < 1 or ly < 1 or lx * ly * ch * 2 > self.ev_size - 36:
            raise Malformed("a frame event's lengths")
        if ch not in (1, 3):
            raise Refused("channels", "%d channels" % ch)
        if self.size[0] and (lx, ly) != tuple(self.size):
            raise Refused("size", "%d x %d" % (lx, ly))
        st = A.stamp(mid_exposure(ts_se, ts_ee), self.overflow, t_offset_ns)
        if st is None:
            out["bad"] += 1
            return
        self.pix_need = lx * ly * ch * 2
        self.emit = dict(stamp_sec=st[0], stamp_nsec=st[1], ts_startframe=ts_sf, ts_endframe=ts_ef, ts_startexposure=ts_se, ts_endexposure=ts_ee,
                         exposure_us=ts_ee - ts_se, length_x=lx, length_y=ly, position_x=px, position_y=py, channels=ch,
                         color_filter=(info >> 4) & 15, roi=(info >> 8) & 127, valid=info & 1, slot=self.slot, ts_overflow=self.overflow)


def table(rows):
    t = np.zeros(len(rows), AEDAT_FRAME_DTYPE)
    for k, r in enumerate(rows):
        for name in AEDAT_FRAME_DTYPE.names:
            t[name][k] = r[name]
    return t


def decode(data, size=(0, 0), t_offset_ns=0, flags=0):
    """a whole stream through a fresh walker"""
    return FrameWalker(size).feed(data, t_offset_ns, flags)[1]


def small_stream(w=5, h=3):
    """the stream the cut tests share: w x h frames, mono and colour, between polarity, special and IMU6 packets; a packet
    of two events (the second invalid) with padding events behind them (eventCapacity > eventNumber), a frame with bytes
    behind its pixels, a packet with overflow 1"""
    mono = lambda seed, **kw: frame_event(test_pixels(w, h, 1, seed), w, h, 1, **kw)
    rgb = lambda seed, **kw: frame_event(test_pixels(w, h, 3, seed), w, h, 3, **kw)
    p1 = A.packet(A.POLARITY, [A.polarity(5, 7, 1, 100), A.polarity(3, 2, 0, 101)])
    f1 = frame_packet([mono(1, ts=(100, 140, 110, 131))])
    sp = A.packet(A.SPECIAL, [A.special(2, 103)])
    f2 = frame_packet([rgb(2, ts=(200, 240, 210, 230), position=(1, 2), color_filter=3, roi=5), mono(3, ts=(250, 290, 260, 280), valid=0)], capacity=4)
    im = A.packet(A.IMU6, [A.imu6(114, (0.1, -0.2, 0.98), (1.5, -2.5, 3.25))])
    other = A.packet(7, [bytes(range(12))], size=12)
    f3 = frame_packet([mono(4, ts=(5, 45, 15, 36), size=36 + 2 * w * h + 6), rgb(5, ts=(50, 90, 60, 80))], overflow=1)
    return p1 + f1 + sp + f2 + im + other + f3 + A.packet(A.POLARITY, [A.polarity(1, 1, 1, 300)])


def bad_streams(w=5, h=3):
    """name -> (a stream the rule fails, the exception's class, what the message names or None); each stands alone and may
    follow any well-formed prefix that ends between packets"""
    px1, px3 = test_pixels(w, h, 1, 9), test_pixels(w, h, 3, 9)
    ok = frame_event(px1, w, h, 1)
    out = {
        "eventSize below 36": (A.packet(FRAME, [bytes(35)], size=35, ts_offset=12), Malformed, "below 36"),
        "eventSize - 36 odd": (A.packet(FRAME, [ok + b"\0"], size=len(ok) + 1, ts_offset=12), Malformed, "odd"),
        "eventTSOffset not 12": (frame_packet([ok], ts_offset=4), Malformed, "eventTSOffset"),
        "eventSize 0": (A.packet(FRAME, [], size=0, ts_offset=12, number=0, capacity=0), Malformed, "eventSize <= 0"),
        "eventNumber above eventCapacity": (A.packet(FRAME, [ok], number=2, capacity=1, size=len(ok), ts_offset=12), Malformed, "eventNumber > eventCapacity"),
        "a polarity packet of size 12": (A.packet(A.POLARITY, [bytes(12)], size=12), Malformed, "the type's"),
        "lengthX 0": (frame_packet([frame_event(px1, 0, h, 1)]), Malformed, "lengthX"),
        "lengthY negative": (frame_packet([frame_event(px1, w, -1, 1)]), Malformed, "lengthY"),
        "pixels beyond the event": (frame_packet([frame_event(px1, w, h, 1)], size=36 + 2 * w * h - 2), Malformed, "exceeds"),
        "lengths whose product passes 2^62": (frame_packet([frame_event(px1, 2 ** 31 - 1, 2 ** 31 - 1, 7)]), Malformed, "exceeds"),
        "2 channels": (frame_packet([frame_event(test_pixels(w, h, 2, 9), w, h, 2)]), Refused, "2 channels"),
        "0 channels": (frame_packet([frame_event(px1, w, h, 0)]), Refused, "0 channels"),
        "4 channels": (frame_packet([frame_event(test_pixels(w, h, 4, 9), w, h, 4)]), Refused, "4 channels"),
        "another size": (frame_packet([frame_event(test_pixels(w + 1, h, 1, 9), w + 1, h, 1)]), Refused, "%d x %d" % (w + 1, h)),
        "transposed size": (frame_packet([frame_event(test_pixels(h, w, 3, 9), h, w, 3)]), Refused, "%d x %d" % (h, w)),
        "negative mid-exposure stamp": (frame_packet([frame_event(px3, w, h, 3, ts=(0, 0, -9, 2))]), Bad, None),
        "negative overflow": (frame_packet([ok], overflow=-1), Bad, None),
    }
    return out
