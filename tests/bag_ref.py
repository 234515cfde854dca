"""The sequential reading of the rosbag v2.0 rule in include/esvio_fe.h, written from that text alone: a plain loop over
one byte string, records out — and a bag writer for the tests.  Not part of the library.

A Walker is one walker state of the rule (a handle has two): feed() takes a chunk that may end anywhere and returns the
walker behind it and what the chunk completes.  The rule is written once, as a generator that asks for its next bytes
(`_rule`); a walker is the list of chunks it has taken, and feed() runs the rule over them again before the new chunk —
or goes on with the suspended rule the last feed() left, when the walker is fed for the first time —, so a walker is a
value and a failed chunk leaves nothing behind."""
import struct

import numpy as np

from esvio_amd.events import EVENT_DTYPE

MAGIC = b"#ROSBAG V2.0\n"
EVENT_TYPE, EVENT_MD5, IMU_TYPE = b"dvs_msgs/EventArray", b"5e8beee5a6c107e504c2e78903c224b8", b"sensor_msgs/Imu"
IMU_MD5 = b"6a62c6daae103f4ff57a132d6f95cec2"  # (never checked: the writer has to put something)
LEFT, RIGHT, IMU = "/davis/left/events", "/davis/right/events", "/imu/data"
TOPICS = (LEFT, RIGHT, IMU)
WIRE_DTYPE = np.dtype({"names": ["x", "y", "sec", "nsec", "polarity"], "formats": ["<u2", "<u2", "<u4", "<u4", "u1"],
                       "offsets": [0, 2, 4, 8, 12], "itemsize": 13})
IMU_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("acc", "<f8", (3,)), ("gyr", "<f8", (3,))])
MESSAGE_DTYPE = np.dtype([("cam", "<i4"), ("seq", "<u4"), ("stamp_sec", "<u4"), ("stamp_nsec", "<u4"), ("time_sec", "<u4"),
                          ("time_nsec", "<u4"), ("height", "<u4"), ("width", "<u4"), ("first", "<u8"), ("count", "<u8")])
u32 = struct.Struct("<I")


class Malformed(ValueError):
    pass


class Bad(ValueError):
    """a BAD stamp failed the call; .bad is the exact count (the event walk: per camera)"""

    def __init__(self, bad):
        super().__init__("%s BAD" % (bad,))
        self.bad = bad


# ---- the writer --------------------------------------------------------------------------------------------------------
def field(name, value):
    body = name.encode() + b"=" + value
    return u32.pack(len(body)) + body


def record(fields, data):
    """a record: fields a list of (name, value bytes)"""
    h = b"".join(field(k, v) for k, v in fields)
    return u32.pack(len(h)) + h + u32.pack(len(data)) + data


def bag_header_record(index_pos, conn_count, chunk_count, total=4096):
    """op 0x03, padded with spaces so that the whole record is `total` bytes (None: no padding)"""
    fields = [("index_pos", struct.pack("<Q", index_pos)), ("conn_count", u32.pack(conn_count)), ("chunk_count", u32.pack(chunk_count)),
              ("op", b"\x03")]
    bare = record(fields, b"")
    return record(fields, b" " * (max(total - len(bare), 0) if total else 0))


def connection_record(conn, topic, mtype, md5, definition=b"# a message definition\n", callerid=None, latching=None, extra=()):
    data = [("topic", topic.encode()), ("type", mtype), ("md5sum", md5), ("message_definition", definition)]
    if callerid is not None:
        data.append(("callerid", callerid))
    if latching is not None:
        data.append(("latching", latching))
    data += list(extra)
    return record([("conn", u32.pack(conn)), ("topic", topic.encode()), ("op", b"\x07")], b"".join(field(k, v) for k, v in data))


def message_record(conn, time, data):
    return record([("conn", u32.pack(conn)), ("time", struct.pack("<II", *time)), ("op", b"\x02")], data)


def chunk_record(body, compression=b"none", size=None):
    return record([("compression", compression), ("size", u32.pack(len(body) if size is None else size)), ("op", b"\x05")], body)


def index_record(conn, count):
    return record([("ver", u32.pack(1)), ("conn", u32.pack(conn)), ("count", u32.pack(count)), ("op", b"\x04")], b"\x11" * (12 * count))


def chunk_info_record(chunk_pos, count):
    return record([("ver", u32.pack(1)), ("chunk_pos", struct.pack("<Q", chunk_pos)), ("start_time", b"\0" * 8), ("end_time", b"\0" * 8),
                   ("count", u32.pack(count)), ("op", b"\x06")], b"\x22" * (8 * count))


def ros_header(seq, stamp, frame_id):
    return struct.pack("<IIII", seq, stamp[0], stamp[1], len(frame_id)) + frame_id


def wire_events(x, y, sec, nsec, p):
    ev = np.zeros(len(x), WIRE_DTYPE)
    ev["x"], ev["y"], ev["sec"], ev["nsec"], ev["polarity"] = x, y, sec, nsec, p
    return ev.tobytes()


def event_array(seq, stamp, wire, frame_id=b"cam", height=260, width=346, n=None):
    """a dvs_msgs/EventArray message: `wire` the packed 13-byte events"""
    return ros_header(seq, stamp, frame_id) + struct.pack("<III", height, width, len(wire) // 13 if n is None else n) + wire


def imu_message(seq, stamp, gyr, acc, frame_id=b"imu", orientation=(0.0, 0.0, 0.0, 1.0)):
    cov = [0.25 * k for k in range(9)]
    return ros_header(seq, stamp, frame_id) + struct.pack("<37d", *orientation, *cov, *gyr, *cov, *acc, *cov)


TYPES = {LEFT: (EVENT_TYPE, EVENT_MD5), RIGHT: (EVENT_TYPE, EVENT_MD5), IMU: (IMU_TYPE, IMU_MD5)}


def write_bag(messages, per_chunk=4, types=None, conns_in_chunks=True, conns_at_index=True, index_records=True, chunk_info=True,
              header_total=4096, magic=True):
    """messages: a list of (topic, (sec, nsec) record time, message data) in file order -> the bag's bytes.  A topic's
    connection id is its rank of first appearance; its record goes in front of its first message inside the chunk
    (conns_in_chunks) and again behind the last chunk, where index_pos points (conns_at_index).  per_chunk messages per
    chunk; behind every chunk one index record per connection in it (index_records); at the end the chunk infos."""
    types = dict(TYPES, **(types or {}))
    ids, out, chunk_pos, counts = {}, [], [], []
    conn_rec = lambda t: connection_record(ids[t], t, *types.get(t, (b"sensor_msgs/Image", b"060021388200f6f0f447d0fcd9c64743")))
    pos = (len(MAGIC) if magic else 0) + (header_total or len(bag_header_record(0, 0, 0, None)))
    for i in range(0, len(messages), per_chunk):
        body, seen = [], {}
        for topic, time, data in messages[i:i + per_chunk]:
            if topic not in ids:
                ids[topic] = len(ids)
                if conns_in_chunks:
                    body.append(conn_rec(topic))
            seen[topic] = seen.get(topic, 0) + 1
            body.append(message_record(ids[topic], time, data))
        chunk_pos.append(pos)
        counts.append(len(seen))
        part = chunk_record(b"".join(body))
        if index_records:
            part += b"".join(index_record(ids[t], k) for t, k in seen.items())
        out.append(part)
        pos += len(part)
    tail = b"".join(conn_rec(t) for t in ids) if conns_at_index else b""
    if chunk_info:
        tail += b"".join(chunk_info_record(p, k) for p, k in zip(chunk_pos, counts))
    return (MAGIC if magic else b"") + bag_header_record(pos, len(ids), len(chunk_pos), header_total) + b"".join(out) + tail


def small_bag(**kw):
    """a bag of a little over 2 KB with everything in it: a bag header record without padding, two chunks, both cameras,
    IMU, an image-like foreign topic, an empty EventArray, connection records in the chunks and at the index, index and
    chunk-info records.  5 left and 4 right events, 2 samples."""
    L = [wire_events([1, 2, 345], [3, 4, 259], [10, 10, 10], [100, 200, 999_999_999], [1, 0, 7]),
         wire_events([5, 6], [7, 8], [11, 11], [0, 5], [0, 255])]
    R = [wire_events([9], [9], [10], [150], [1]), wire_events([10, 11, 12], [1, 2, 3], [11, 11, 12], [1, 2, 0], [1, 1, 0])]
    msgs = [(LEFT, (10, 500), event_array(1, (10, 100), L[0])),
            ("/davis/left/image_raw", (10, 600), ros_header(4, (10, 90), b"cam") + bytes(range(60))),
            (IMU, (10, 700), imu_message(7, (10, 50), (0.1, -0.2, 0.3), (9.5, 0.25, -1.5))),
            (RIGHT, (10, 800), event_array(1, (10, 100), R[0], frame_id=b"")),
            (LEFT, (11, 0), event_array(2, (10, 950), b"")),
            (RIGHT, (11, 600), event_array(2, (11, 0), R[1], frame_id=b"right_cam")),
            (IMU, (11, 700), imu_message(8, (11, 1), (1.0, 2.0, 3.0), (-4.0, 5.0, -6.0), frame_id=b"")),
            (LEFT, (11, 800), event_array(3, (11, 0), L[1]))]
    kw.setdefault("header_total", None)
    return write_bag(msgs, **kw)


def malformed_streams():
    """name -> a stream that breaks one rule of the text, from the fresh state or between two records"""
    conn = lambda *a, **k: chunk_record(connection_record(*a, **k))
    ev = event_array(1, (1, 2), wire_events([1], [2], [3], [4], [1]))
    lconn = connection_record(0, LEFT, EVENT_TYPE, EVENT_MD5)
    return {
        "header_len > 4096": b"\x01\x10\x00\x00",
        "a header without op": record([("conn", b"\0" * 4)], b""),
        "op of two bytes": record([("op", b"\x02\x00")], b""),
        "a field overruns its header": b"\x08\x00\x00\x00\x09\x00\x00\x00op=\x02" + b"\0" * 4,
        "a message without time": record([("conn", b"\0" * 4), ("op", b"\x02")], b""),
        "a message with a short conn": record([("conn", b"\0" * 3), ("time", b"\0" * 8), ("op", b"\x02")], b""),
        "a connection without topic": record([("conn", b"\0" * 4), ("op", b"\x07")], b""),
        "a topic of 256 bytes": connection_record(0, "/" + "t" * 255, b"x", b"y"),
        "a chunk without size": record([("compression", b"none"), ("op", b"\x05")], b""),
        "a compressed chunk": chunk_record(b"BZh9", compression=b"bz2"),
        "an lz4 chunk": chunk_record(b"", compression=b"lz4"),
        "size differs from data_len": chunk_record(b"", size=1),
        "a chunk inside a chunk": chunk_record(chunk_record(b"")),
        "an index record inside a chunk": chunk_record(index_record(0, 1)),
        "a record that overruns its chunk": chunk_record(lconn[:-1]),
        "three bytes at a chunk's end": chunk_record(lconn + b"\0\0\0"),
        "a bag header without chunk_count": record([("op", b"\x03"), ("index_pos", b"\0" * 8), ("conn_count", b"\0" * 4)], b""),
        "another type on an event topic": conn(0, RIGHT, b"prophesee_event_msgs/EventArray", EVENT_MD5),
        "another md5 on an event topic": conn(0, LEFT, EVENT_TYPE, b"5e8beee5a6c107e504c2e78903c224b9"),
        "no md5 on an event topic": record([("conn", b"\0" * 4), ("topic", LEFT.encode()), ("op", b"\x07")], field("type", EVENT_TYPE)),
        "a type of 300 bytes": conn(0, LEFT, EVENT_TYPE + b"x" * 281, EVENT_MD5),
        "another type on the imu topic": conn(0, IMU, b"sensor_msgs/Image", IMU_MD5),
        "a connection field that overruns": record([("conn", b"\0" * 4), ("topic", LEFT.encode()), ("op", b"\x07")], b"\x20\x00\x00\x00type=x"),
        "a connection field without =": record([("conn", b"\0" * 4), ("topic", b"/t"), ("op", b"\x07")], b"\x04\x00\x00\x00type"),
        "a repeated conn id with another topic": chunk_record(lconn + connection_record(0, RIGHT, EVENT_TYPE, EVENT_MD5)),
        "a repeated conn id without a role": chunk_record(lconn + connection_record(0, "/t", b"x", b"y")),
        "65 connections with a role": b"".join(connection_record(k, IMU, IMU_TYPE, IMU_MD5) for k in range(65)),
        "an event message one byte long": chunk_record(lconn + message_record(0, (1, 1), ev + b"\0")),
        "an event message with n one too large": chunk_record(lconn + message_record(0, (1, 1), ev[:-17] + b"\x02\0\0\0" + ev[-13:])),
        "an event message of 27 bytes": chunk_record(lconn + message_record(0, (1, 1), b"\0" * 27)),
        "a frame_id beyond the message": chunk_record(lconn + message_record(0, (1, 1), ros_header(1, (1, 1), b"")[:12] + b"\x10\0\0\0" + b"\0" * 20)),
        "an imu message one byte short": chunk_record(connection_record(0, IMU, IMU_TYPE, IMU_MD5) +
                                                        message_record(0, (1, 1), imu_message(1, (1, 1), (0, 0, 0), (0, 0, 0))[:-1])),
    }



# ---- the rule ----------------------------------------------------------------------------------------------------------
def parse_fields(h, what):
    """the fields of a header (or of connection data): {name: value}; the last of a repeated field counts"""
    out, pos = {}, 0
    while pos < len(h):
        if len(h) - pos < 4:
            raise Malformed("a field overruns its %s" % what)
        fl = u32.unpack_from(h, pos)[0]
        pos += 4
        if fl > len(h) - pos:
            raise Malformed("a field overruns its %s" % what)
        f = bytes(h[pos:pos + fl])
        pos += fl
        if b"=" not in f:
            raise Malformed("a field without '='")
        k, v = f.split(b"=", 1)
        out[k] = v
    return out


def need(fields, name, size):
    v = fields.get(name)
    if v is None or (size is not None and len(v) != size):
        raise Malformed("missing or wrong-sized field %s" % name.decode())
    return v


def _rule(topics, mode, out):
    """The rule as a generator.  It yields what it needs next — ("read", n): exactly n bytes; ("skip", n): n bytes
    nobody reads; ("events", k): as many whole 13-byte events as there are, at least one and k at the most — and is sent
    the bytes.  `out` is the dictionary it reports into; the driver exchanges it between chunks."""
    roles = {t.encode(): r for r, t in enumerate(topics) if t is not None}  # topic -> 0 left, 1 right, 2 imu
    table, emitted = {}, [0, 0]
    chunk_left = None  # bytes of the open chunk still to come

    def take(req):
        nonlocal chunk_left
        got = yield req
        n = req[1] if req[0] != "events" else len(got)
        if chunk_left is not None:
            chunk_left -= n
        return got

    while True:
        if chunk_left is not None:
            if chunk_left == 0:
                chunk_left = None
            elif chunk_left < 4:
                raise Malformed("a record overruns its chunk")
        hl = u32.unpack((yield from take(("read", 4))))[0]
        if hl > 4096:
            raise Malformed("header_len > 4096")
        if chunk_left is not None and hl + 4 > chunk_left:
            raise Malformed("a record overruns its chunk")
        f = parse_fields((yield from take(("read", hl))), "header")
        if b"op" not in f:
            raise Malformed("a header without op")
        if len(f[b"op"]) != 1:
            raise Malformed("an op field that is not 1 byte long")
        op = f[b"op"][0]
        role = None
        if op == 3:
            need(f, b"index_pos", 8), need(f, b"conn_count", 4), need(f, b"chunk_count", 4)
        elif op == 5:
            size = u32.unpack(need(f, b"size", 4))[0]
            if need(f, b"compression", None) != b"none":
                raise Malformed("a compressed chunk: run `rosbag decompress`")
        elif op == 7:
            conn = u32.unpack(need(f, b"conn", 4))[0]
            topic = need(f, b"topic", None)
            if len(topic) > 255:
                raise Malformed("a topic longer than 255 bytes")
            role = roles.get(topic)
        elif op == 2:
            conn = u32.unpack(need(f, b"conn", 4))[0]
            time = struct.unpack("<II", need(f, b"time", 8))
        dl = u32.unpack((yield from take(("read", 4))))[0]
        if op == 5 and size != dl:
            raise Malformed("a chunk whose size differs from its data_len")
        if chunk_left is not None:
            if op not in (2, 7):
                raise Malformed("a record inside a chunk that is neither message data nor a connection")
            if dl > chunk_left:
                raise Malformed("a record overruns its chunk")
        if op == 5:
            out["chunks"] += 1
            chunk_left = dl
        elif op == 7:
            # the connection data, field by field: a field's first 264 bytes are looked at when they have arrived
            left, ok_type, ok_md5 = dl, False, False
            while left:
                if left < 4:
                    raise Malformed("a field overruns its connection data")
                fl = u32.unpack((yield from take(("read", 4))))[0]
                left -= 4
                if fl > left:
                    raise Malformed("a field overruns its connection data")
                keep = min(fl, 264)
                head = bytes((yield from take(("read", keep))))
                if b"=" not in head:
                    raise Malformed("a connection field without '='")
                k, v = head.split(b"=", 1)
                if role is not None and k == b"type":
                    ok_type = fl == keep and v == (IMU_TYPE if role == 2 else EVENT_TYPE)
                elif role is not None and k == b"md5sum":
                    ok_md5 = fl == keep and v == EVENT_MD5
                yield from take(("skip", fl - keep))
                left -= fl
            out["connections"] += 1
            if conn in table and table[conn] != role:
                raise Malformed("a repeated conn id with another topic")
            if role is not None:
                if not ok_type:
                    raise Malformed("type on topic %s" % topics[role])
                if role != 2 and not ok_md5:
                    raise Malformed("md5sum on topic %s" % topics[role])
                if conn not in table:
                    if len(table) == 64:
                        raise Malformed("more than 64 connections with a role")
                    table[conn] = role
        elif op == 2:
            role = table.get(conn)
            if role is None:
                out["other_messages"] += 1
                yield from take(("skip", dl))
                continue
            if dl < (16 + 296 if role == 2 else 28):
                raise Malformed("data_len on topic %s" % topics[role])
            seq, s_sec, s_nsec, flen = struct.unpack("<IIII", (yield from take(("read", 16))))
            if role == 2:
                if dl != 16 + flen + 296:
                    raise Malformed("data_len on topic %s" % topics[role])
                yield from take(("skip", flen))
                if mode != "side":
                    yield from take(("skip", 296))
                    continue
                body = bytes((yield from take(("read", 296))))
                if s_nsec >= 10 ** 9:
                    out["bad_imu"] += 1
                else:
                    out["imu"].append((s_sec, s_nsec, body[200:224], body[104:128]))  # stamp, acc, gyr
                continue
            if flen > dl - 28:
                raise Malformed("data_len on topic %s" % topics[role])
            yield from take(("skip", flen))
            height, width, n = struct.unpack("<III", (yield from take(("read", 12))))
            if dl != 28 + flen + 13 * n:
                raise Malformed("data_len on topic %s" % topics[role])
            first, todo = emitted[role], n
            while todo:
                got = yield from take(("events", todo))
                k = len(got) // 13
                out["wire"][role].append(bytes(got))
                emitted[role] += k
                todo -= k
            out["messages"].append((role, seq, s_sec, s_nsec, time[0], time[1], height, width, first, n))
        elif op in (3, 4, 6):
            yield from take(("skip", dl))
        else:
            out["other_records"] += 1
            yield from take(("skip", dl))


def fresh_out():
    return {"wire": [[], []], "messages": [], "imu": [], "bad_imu": 0, "other_messages": 0, "other_records": 0, "chunks": 0,
            "connections": 0}


class Walker:
    """one walker state: mode "events" or "side"; topics = (left, right, imu), None for none"""

    def __init__(self, mode="events", topics=TOPICS, history=()):
        self.mode, self.topics, self.history = mode, tuple(topics), tuple(history)

    def _step(self, live, chunk):
        """the rule, suspended at `live`, run over one more chunk -> what that chunk completes"""
        gen, buf, req = live["gen"], live["buf"], live["req"]
        out = live["out"]
        out.clear()
        out.update(fresh_out())
        buf += chunk
        while True:
            if req[0] == "skip":
                n = min(req[1], len(buf))
                del buf[:n]
                if n < req[1]:
                    req = ("skip", req[1] - n)
                    break
                req = gen.send(b"")
            elif req[0] == "read":
                if len(buf) < req[1]:
                    break
                got = bytes(buf[:req[1]])
                del buf[:req[1]]
                req = gen.send(got)
            else:
                k13 = min(len(buf) // 13, req[1])
                if not k13:
                    break
                got = bytes(buf[:13 * k13])
                del buf[:13 * k13]
                req = gen.send(got)
        live["req"] = req
        return out

    def _resume(self):
        """the rule suspended behind this walker's chunks: the one a feed() left here, if nobody has taken it since, else
        the rule run over the chunks again"""
        live, self._live = getattr(self, "_live", None), None
        if live is None:
            out = fresh_out()
            gen = _rule(self.topics, self.mode, out)
            live = {"gen": gen, "buf": bytearray(), "req": next(gen), "out": out}
            for chunk in self.history:
                self._step(live, chunk)
        return live

    def feed(self, data):
        """-> (the walker behind the chunk, what the chunk completes); Malformed or Bad: this walker is as it was.
        The result: "events" per camera an EVENT_DTYPE array, "wire" per camera the gathered bytes, "messages" a
        MESSAGE_DTYPE array, "imu" an IMU_DTYPE array, the counters."""
        data = bytes(data)
        live = self._resume()
        out = self._step(live, data)  # (an exception leaves the rule dead and this walker without it: the next feed runs it again)
        res = dict(out)
        res["wire"] = [b"".join(w) for w in out["wire"]]
        res["events"] = [records(w) for w in res["wire"]]
        res["messages"] = np.array(out["messages"], MESSAGE_DTYPE) if out["messages"] else np.zeros(0, MESSAGE_DTYPE)
        res["cam_messages"] = [int((res["messages"]["cam"] == cam).sum()) for cam in range(2)]
        imu = np.zeros(len(out["imu"]), IMU_DTYPE)
        for k, (sec, nsec, acc, gyr) in enumerate(out["imu"]):
            imu[k]["sec"], imu[k]["nsec"] = sec, nsec
            imu[k]["acc"], imu[k]["gyr"] = np.frombuffer(acc, "<f8"), np.frombuffer(gyr, "<f8")
        res["imu"] = imu
        if self.mode == "events":
            bad = [int((e["nsec"] >= 10 ** 9).sum()) for e in res["events"]]
            if sum(bad):
                raise Bad(bad)
        elif out["bad_imu"]:
            raise Bad(out["bad_imu"])
        after = Walker(self.mode, self.topics, self.history + (data,))
        after._live = live
        return after, res


def records(wire):
    """packed 13-byte wire events -> EVENT_DTYPE records, as the rule writes them"""
    w = np.frombuffer(wire, WIRE_DTYPE)
    ev = np.zeros(len(w), EVENT_DTYPE)
    ev["x"], ev["y"], ev["sec"], ev["nsec"] = w["x"], w["y"], w["sec"], w["nsec"]
    ev["polarity"] = (w["polarity"] != 0).astype(np.uint8)
    return ev


def decode(bag, mode="events", topics=TOPICS):
    """a whole bag (the magic included) in one call"""
    assert bag[:13] == MAGIC
    return Walker(mode, topics).feed(bag[13:])[1]


def header(data):
    """esvio_fe_bag_header's rule: (payload_offset, index_pos, conn_count, chunk_count, version, complete); Malformed"""
    data = bytes(data)
    m = min(len(data), 13)
    if data[:m] != MAGIC[:m]:
        raise Malformed("not a bag")
    if len(data) < 13:
        return (0, 0, 0, 0, 0, 0)
    if len(data) - 13 < 4:
        return (13, 0, 0, 0, 20, 0)
    hl = u32.unpack_from(data, 13)[0]
    if hl > 4096:
        raise Malformed("header_len > 4096")
    if len(data) - 17 < hl + 4:
        return (13, 0, 0, 0, 20, 0)
    f = parse_fields(data[17:17 + hl], "header")
    if f.get(b"op") != b"\x03":
        raise Malformed("the first record is not the bag header")
    return (13, struct.unpack("<Q", need(f, b"index_pos", 8))[0], u32.unpack(need(f, b"conn_count", 4))[0],
            u32.unpack(need(f, b"chunk_count", 4))[0], 20, 1)
