"""The sequential reading of the "rosbag images" rule in include/esvio_fe.h, written from that text alone, on top of
tests/bag_ref.py (its writer and its field parser): sensor_msgs/Image messages and bags that hold them, getImageFromMsg's
conversion as plain loops with the gray in plain integer Python, and the image walker as a plain loop over one byte
string.  Not part of the library.

An ImageWalker is the image walker's state as a value: the bytes it has taken.  feed() reads the whole string again from
the start, stops where the bytes end, and returns what the new chunk completes: the messages whose last byte it brings.
A rule is checked as soon as the bytes it reads are there, so a malformed or refused item fails the call that brings its
last byte, and that call leaves the walker as it was."""
import struct

import numpy as np

import bag_ref as B

IMAGE_TYPE, IMAGE_MD5 = b"sensor_msgs/Image", b"060021388200f6f0f447d0fcd9c64743"  # (the MD5 is never checked)
LEFT_IMAGE, RIGHT_IMAGE = "/davis/left/image_raw", "/davis/right/image_raw"
IMAGE_TOPICS = (LEFT_IMAGE, RIGHT_IMAGE)
TYPES = {LEFT_IMAGE: (IMAGE_TYPE, IMAGE_MD5), RIGHT_IMAGE: (IMAGE_TYPE, IMAGE_MD5)}
CLASSES = {b"mono8": 1, b"8UC1": 1, b"bgr8": 2, b"8UC3": 2, b"rgb8": 3}
BPP = {1: 1, 2: 3, 3: 3}
IMAGE_DTYPE = np.dtype({"names": ["cam", "seq", "stamp_sec", "stamp_nsec", "time_sec", "time_nsec", "height", "width", "step", "encoding",
                                  "is_bigendian", "index"],
                        "formats": ["<i4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<i4", "<i4", "<u8"],
                        "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48], "itemsize": 56})
COUNTERS = ("other_messages", "other_records", "chunks", "connections")


class Refused(B.Malformed):
    """an encoding or a size the rule refuses by name"""


# ---- the writer ----------------------------------------------------------------------------------------------------------
def image_message(seq, stamp, height, width, encoding, step, data, frame_id=b"cam", is_bigendian=0, d=None):
    """a sensor_msgs/Image message; d: the data length word, when it is to lie"""
    enc = encoding if isinstance(encoding, bytes) else encoding.encode()
    return (B.ros_header(seq, stamp, frame_id) + struct.pack("<III", height, width, len(enc)) + enc + struct.pack("<BII", is_bigendian, step,
            len(data) if d is None else d) + bytes(data))


def rows(pixels, step, fill=0xEE):
    """a dense [h, w * bpp] uint8 array -> the data of an Image message whose rows lie `step` bytes apart; the padding
    bytes hold `fill`, which no test image holds where it would matter"""
    h, rb = pixels.shape
    out = np.full((h, step), fill, np.uint8)
    out[:, :rb] = pixels
    return out.tobytes()


def write_bag(messages, **kw):
    """bag_ref.write_bag with the image topics' type"""
    kw["types"] = dict(TYPES, **(kw.get("types") or {}))
    return B.write_bag(messages, **kw)


# ---- getImageFromMsg's conversion ----------------------------------------------------------------------------------------
def gray(r, g, b):
    """cv::cvtColor's 8-bit gray as the rule states it (the 15-bit form)"""
    return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15


def gray14(r, g, b):
    """the OpenCV 3 form the rule is NOT"""
    return (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14


def convert(data, height, width, step, encoding):
    """the gray image [height, width] of an Image message's data: plain loops"""
    cls = CLASSES[encoding if isinstance(encoding, bytes) else encoding.encode()] if not isinstance(encoding, int) else encoding
    data = bytes(data)
    out = np.zeros((height, width), np.uint8)
    for r in range(height):
        for c in range(width):
            p = r * step + c * BPP[cls]
            if cls == 1:
                out[r, c] = data[p]
            elif cls == 2:
                out[r, c] = gray(data[p + 2], data[p + 1], data[p])
            else:
                out[r, c] = gray(data[p], data[p + 1], data[p + 2])
    return out


def convert_rows(data, height, width, step, cls):
    """convert() for the larger images of the GPU tests: the same integer formula on whole arrays (test_bag_image_ref.py
    holds the two equal)"""
    a = np.frombuffer(bytes(data), np.uint8)[:step * height].reshape(height, step)[:, :width * BPP[cls]].astype(np.int64)
    if cls == 1:
        return a.astype(np.uint8)
    a = a.reshape(height, width, 3)
    r, g, b = (a[..., 2], a[..., 1], a[..., 0]) if cls == 2 else (a[..., 0], a[..., 1], a[..., 2])
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)


# ---- the rule ------------------------------------------------------------------------------------------------------------
class _End(Exception):
    """the bytes end here"""


def read_stream(s, topics=IMAGE_TOPICS, size=None):
    """the image walk over the byte string s from the fresh state to where its bytes end -> (the completed messages, the
    counters).  A message: a dict of the table's fields, "cam", "data" (the D payload bytes) and "end" (the position
    behind its last byte).  size = (width, height): the only size taken (None: any).  Malformed / Refused."""
    roles = {t.encode(): r for r, t in enumerate(topics) if t is not None}
    table, done, cnt = {}, [], dict.fromkeys(COUNTERS, 0)
    pos, chunk_end = 0, None

    def read(n):
        nonlocal pos
        if len(s) - pos < n:
            raise _End()
        pos += n
        return s[pos - n:pos]

    def skip(n):
        nonlocal pos
        if len(s) - pos < n:
            pos = len(s)
            raise _End()
        pos += n

    def bad(what, role):
        raise B.Malformed("%s on topic %s" % (what, topics[role]))

    try:
        while True:
            if chunk_end is not None:
                if pos == chunk_end:
                    chunk_end = None
                elif chunk_end - pos < 4:
                    raise B.Malformed("a record overruns its chunk")
            hl = B.u32.unpack(read(4))[0]
            if hl > 4096:
                raise B.Malformed("header_len > 4096")
            if chunk_end is not None and hl + 4 > chunk_end - pos:
                raise B.Malformed("a record overruns its chunk")
            f = B.parse_fields(read(hl), "header")
            if b"op" not in f:
                raise B.Malformed("a header without op")
            if len(f[b"op"]) != 1:
                raise B.Malformed("an op field that is not 1 byte long")
            op, role = f[b"op"][0], None
            if op == 3:
                B.need(f, b"index_pos", 8), B.need(f, b"conn_count", 4), B.need(f, b"chunk_count", 4)
            elif op == 5:
                csize = B.u32.unpack(B.need(f, b"size", 4))[0]
                if B.need(f, b"compression", None) != b"none":
                    raise B.Malformed("a compressed chunk: run `rosbag decompress`")
            elif op == 7:
                conn = B.u32.unpack(B.need(f, b"conn", 4))[0]
                topic = B.need(f, b"topic", None)
                if len(topic) > 255:
                    raise B.Malformed("a topic longer than 255 bytes")
                role = roles.get(topic)
            elif op == 2:
                conn = B.u32.unpack(B.need(f, b"conn", 4))[0]
                time = struct.unpack("<II", B.need(f, b"time", 8))
            dl = B.u32.unpack(read(4))[0]
            if op == 5 and csize != dl:
                raise B.Malformed("a chunk whose size differs from its data_len")
            if chunk_end is not None:
                if op not in (2, 7):
                    raise B.Malformed("a record inside a chunk that is neither message data nor a connection")
                if dl > chunk_end - pos:
                    raise B.Malformed("a record overruns its chunk")
            if op == 5:
                cnt["chunks"] += 1
                chunk_end = pos + dl
            elif op == 7:
                left, ok_type = dl, False
                while left:
                    if left < 4:
                        raise B.Malformed("a field overruns its connection data")
                    fl = B.u32.unpack(read(4))[0]
                    left -= 4
                    if fl > left:
                        raise B.Malformed("a field overruns its connection data")
                    keep = min(fl, 264)
                    head = bytes(read(keep))
                    if b"=" not in head:
                        raise B.Malformed("a connection field without '='")
                    k, v = head.split(b"=", 1)
                    if role is not None and k == b"type":
                        ok_type = fl == keep and v == IMAGE_TYPE
                    skip(fl - keep)
                    left -= fl
                cnt["connections"] += 1
                if conn in table and table[conn] != role:
                    raise B.Malformed("a repeated conn id with another topic")
                if role is not None:
                    if not ok_type:
                        bad("a connection whose type is not sensor_msgs/Image", role)
                    if conn not in table:
                        if len(table) == 64:
                            raise B.Malformed("more than 64 connections with a role")
                        table[conn] = role
            elif op == 2:
                role = table.get(conn)
                if role is None:
                    cnt["other_messages"] += 1
                    skip(dl)
                    continue
                if dl < 38:
                    bad("data_len", role)
                seq, s_sec, s_nsec, flen = struct.unpack("<IIII", read(16))
                if flen > dl - 38:
                    bad("data_len", role)
                skip(flen)
                height, width, le = struct.unpack("<III", read(12))
                if le > 32:
                    bad("an encoding longer than 32 bytes", role)
                if le > dl - 38 - flen:
                    bad("data_len", role)
                if height == 0 or width == 0:
                    bad("height or width 0", role)
                tail = read(le + 9)
                enc = bytes(tail[:le])
                big, step, d = struct.unpack("<BII", tail[le:])
                if d != step * height:
                    bad("D is not step * height", role)
                if dl != 37 + flen + le + d:
                    bad("data_len", role)
                if enc not in CLASSES:
                    raise Refused("encoding %r on topic %s" % (enc, topics[role]))
                cls = CLASSES[enc]
                if step < width * BPP[cls]:
                    bad("step below width * bpp", role)
                if size is not None and (width, height) != tuple(size):
                    raise Refused("%d x %d on topic %s" % (width, height, topics[role]))
                data = read(d)
                done.append(dict(cam=role, seq=seq, stamp_sec=s_sec, stamp_nsec=s_nsec, time_sec=time[0], time_nsec=time[1], height=height,
                                 width=width, step=step, encoding=cls, is_bigendian=big, data=bytes(data), end=pos))
            elif op in (3, 4, 6):
                skip(dl)
            else:
                cnt["other_records"] += 1
                skip(dl)
    except _End:
        pass
    return done, cnt


class ImageWalker:
    """the image walker's state: topics = (left, right), size = (width, height) or None"""

    def __init__(self, topics=IMAGE_TOPICS, size=None, history=b"", seen=None):
        self.topics, self.size, self.history = tuple(topics), size, history
        self.seen = seen if seen is not None else (0, dict.fromkeys(COUNTERS, 0))  # messages and counters behind `history`

    def feed(self, data):
        """-> (the walker behind the chunk, what the chunk completes): "images" per camera a list of gray arrays,
        "payloads" the completed messages' data in stream order, "table" an IMAGE_DTYPE array whose index counts per
        call, the counters.  Malformed / Refused: this walker is as it was."""
        s = self.history + bytes(data)
        done, cnt = read_stream(s, self.topics, self.size)
        new = done[self.seen[0]:]
        res = {k: cnt[k] - self.seen[1][k] for k in COUNTERS}
        res["images"], res["payloads"] = [[], []], [m["data"] for m in new]
        table = np.zeros(len(new), IMAGE_DTYPE)
        for k, m in enumerate(new):
            for name in IMAGE_DTYPE.names[:-1]:
                table[k][name] = m[name]
            table[k]["index"] = len(res["images"][m["cam"]])
            res["images"][m["cam"]].append(convert_rows(m["data"], m["height"], m["width"], m["step"], m["encoding"]))
        res["table"] = table
        return ImageWalker(self.topics, self.size, s, (len(done), cnt)), res


def decode(bag, topics=IMAGE_TOPICS, size=None):
    """a whole bag (the magic included) in one call"""
    assert bag[:13] == B.MAGIC
    return ImageWalker(topics, size).feed(bag[13:])[1]


# ---- the streams of the tests ----------------------------------------------------------------------------------------------
def test_image(h, w, cls, seed):
    """a seeded dense [h, w * bpp] image that holds neither 0xEE nor 0xA5 (the fills of padding and guards)"""
    px = np.random.default_rng(seed).integers(0, 256, (h, w * BPP[cls]), dtype=np.uint8)
    px[(px == 0xEE) | (px == 0xA5)] = 7
    return px


def small_bag(w=5, h=3, **kw):
    """a bag of a few KB with everything in it: both cameras' images in all three classes and with padded, odd steps, the
    right camera first once, events of both cameras, IMU, a foreign topic, and the last image alone in its chunk"""
    ev = B.wire_events([1, 2], [3, 4], [10, 10], [100, 200], [1, 0])
    img = lambda k, name, cls, pad: image_message(k, (10, 100 * k), h, w, name, w * BPP[cls] + pad, rows(test_image(h, w, cls, 40 + k), w * BPP[cls] + pad),
                                                  frame_id=(b"", b"cam", b"camera_left")[k % 3], is_bigendian=k % 2)
    msgs = [(B.LEFT, (10, 500), B.event_array(1, (10, 100), ev)),
            (LEFT_IMAGE, (10, 510), img(1, "mono8", 1, 0)),
            (RIGHT_IMAGE, (10, 520), img(1, "rgb8", 3, 5)),
            (B.IMU, (10, 700), B.imu_message(7, (10, 50), (0.1, -0.2, 0.3), (9.5, 0.25, -1.5))),
            ("/odometry", (10, 710), B.ros_header(4, (10, 90), b"odom") + bytes(range(40))),
            (RIGHT_IMAGE, (10, 800), img(2, "8UC3", 2, 1)),
            (B.RIGHT, (10, 810), B.event_array(1, (10, 100), ev, frame_id=b"")),
            (LEFT_IMAGE, (10, 820), img(2, "bgr8", 2, 16)),
            (LEFT_IMAGE, (11, 0), img(3, "8UC1", 1, 3))]
    kw.setdefault("header_total", None)
    kw.setdefault("per_chunk", 4)
    return write_bag(msgs, **kw)


def bad_streams(w=5, h=3):
    """name -> (a stream that breaks one of the image rules, from the fresh state; what its message must name)"""
    conn = B.connection_record(0, LEFT_IMAGE, IMAGE_TYPE, IMAGE_MD5)
    good = rows(test_image(h, w, 3, 1), 3 * w + 2)
    rec = lambda m: B.chunk_record(conn + B.message_record(0, (1, 1), m))
    im = lambda **k: image_message(1, (1, 1), k.pop("h", h), k.pop("w", w), k.pop("enc", "rgb8"), k.pop("step", 3 * w + 2), k.pop("data", good), **k)
    return {
        "another type on an image topic": (B.chunk_record(B.connection_record(0, RIGHT_IMAGE, b"sensor_msgs/CompressedImage", IMAGE_MD5)), RIGHT_IMAGE),
        "no type on an image topic": (B.record([("conn", b"\0" * 4), ("topic", LEFT_IMAGE.encode()), ("op", b"\x07")], B.field("md5sum", IMAGE_MD5)), LEFT_IMAGE),
        "a message of 37 bytes": (rec(b"\0" * 37), LEFT_IMAGE),
        "a frame_id beyond the message": (rec(struct.pack("<IIII", 1, 1, 1, 4000) + b"\0" * 60), LEFT_IMAGE),
        "an encoding of 33 bytes": (rec(im(enc="m" * 33)), LEFT_IMAGE),
        "an encoding beyond the message": (rec(B.ros_header(1, (1, 1), b"") + struct.pack("<III", 1, 1, 30) + b"mono8\0\1\0\0\0\1\0\0\0\7"), LEFT_IMAGE),
        "height 0": (rec(im(h=0, data=b"")), LEFT_IMAGE),
        "width 0": (rec(im(w=0)), LEFT_IMAGE),
        "D one more than step * height": (rec(im(data=good + b"\0")), LEFT_IMAGE),
        "D says step * height, data_len one more": (rec(im(d=len(good)) + b"\0"), LEFT_IMAGE),
        "data_len one short": (rec(im()[:-1]), LEFT_IMAGE),
        "step one below width * bpp": (rec(im(step=3 * w - 1, data=good[:(3 * w - 1) * h])), LEFT_IMAGE),
        "mono16": (rec(im(enc="mono16", step=2 * w, data=good[:2 * w * h])), "mono16"),
        "bayer_rggb8": (rec(im(enc="bayer_rggb8", step=w, data=good[:w * h])), "bayer_rggb8"),
        "an empty encoding": (rec(im(enc="", step=w, data=good[:w * h])), LEFT_IMAGE),
        "Mono8 in capitals": (rec(im(enc="Mono8", step=w, data=good[:w * h])), "Mono8"),
        "another size": (rec(im(w=w + 1, step=3 * w + 3, data=bytes(h * (3 * w + 3)))), "%d x %d" % (w + 1, h)),
        "width and height swapped": (rec(im(w=h, h=w, step=3 * h, data=bytes(3 * h * w))), "%d x %d" % (h, w)),
    }
