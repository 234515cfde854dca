"""CPU: tests/bag_ref.py, the sequential reading of the rosbag v2.0 rule, against answers derived by hand from the text in
include/esvio_fe.h — a chunk written out byte by byte — and against itself at every two-call cut of small_bag()."""
import numpy as np
import pytest

import bag_ref as B

# one chunk, one connection on topic "/l" with conn id 0, one EventArray message with two events; every byte by hand
CONN = (b"\x21\x00\x00\x00"                              # header_len 33
        b"\x09\x00\x00\x00conn=\x00\x00\x00\x00"         # 13
        b"\x08\x00\x00\x00topic=/l"                      # 12
        b"\x04\x00\x00\x00op=\x07"                       # 8
        b"\x47\x00\x00\x00"                              # data_len 71
        b"\x18\x00\x00\x00type=dvs_msgs/EventArray"      # 4 + 24
        b"\x27\x00\x00\x00md5sum=5e8beee5a6c107e504c2e78903c224b8")  # 4 + 39
EVENT_0 = b"\x02\x01" b"\x04\x03" b"\x0a\x00\x00\x00" b"\xff\xc9\x9a\x3b" b"\x00"  # x 258, y 772, 10 s, 999 999 999 ns, off
EVENT_1 = b"\x59\x01" b"\x03\x01" b"\x0b\x00\x00\x00" b"\x00\x00\x00\x00" b"\x02"  # x 345, y 259, 11 s, 0 ns, wire byte 2: on
MSG = (b"\x26\x00\x00\x00"                               # header_len 38
       b"\x09\x00\x00\x00conn=\x00\x00\x00\x00"          # 13
       b"\x0d\x00\x00\x00time=\x14\x00\x00\x00\x15\x00\x00\x00"  # 17: 20 s, 21 ns
       b"\x04\x00\x00\x00op=\x02"                        # 8
       b"\x37\x00\x00\x00"                               # data_len 55 = 28 + 1 + 26
       b"\x05\x00\x00\x00" b"\x03\x00\x00\x00" b"\x07\x00\x00\x00"  # seq 5, stamp 3 s 7 ns
       b"\x01\x00\x00\x00c"                              # frame_id "c"
       b"\x04\x01\x00\x00" b"\x5a\x01\x00\x00"           # height 260, width 346
       b"\x02\x00\x00\x00" + EVENT_0 + EVENT_1)
CHUNK = (b"\x29\x00\x00\x00"                             # header_len 41
         b"\x10\x00\x00\x00compression=none"             # 20
         b"\x09\x00\x00\x00size=\xd5\x00\x00\x00"        # 13: 213
         b"\x04\x00\x00\x00op=\x05"                      # 8
         b"\xd5\x00\x00\x00" + CONN + MSG)               # data_len 213


def test_the_hand_written_chunk_field_by_field():
    assert (len(CONN), len(MSG), len(CHUNK)) == (112, 101, 4 + 41 + 4 + 213)
    w, o = B.Walker("events", ("/l", None, None)).feed(CHUNK)
    ev = o["events"][0]
    assert len(ev) == 2 and len(o["events"][1]) == 0
    assert [(int(e["x"]), int(e["y"]), int(e["sec"]), int(e["nsec"]), int(e["polarity"])) for e in ev] == \
        [(258, 772, 10, 999_999_999, 0), (345, 259, 11, 0, 1)]
    assert ev.tobytes() == EVENT_0 + b"\0\0\0" + EVENT_1[:12] + b"\x01\0\0\0"  # the padding 0, the polarity (byte != 0)
    assert o["wire"][0] == EVENT_0 + EVENT_1
    m = o["messages"]
    assert len(m) == 1
    assert [int(m[0][k]) for k in m.dtype.names] == [0, 5, 3, 7, 20, 21, 260, 346, 0, 2]
    assert (o["chunks"], o["connections"], o["other_messages"], o["other_records"]) == (1, 1, 0, 0)
    # the writer builds the same bytes
    conn = B.connection_record(0, "/l", B.EVENT_TYPE, B.EVENT_MD5)
    msg = B.message_record(0, (20, 21), B.event_array(5, (3, 7), EVENT_0 + EVENT_1, frame_id=b"c"))
    assert msg == MSG and conn[:4 + 33] == CONN[:4 + 33] and B.chunk_record(CONN + MSG) == CHUNK
    # the same chunk as the right camera's, and with no role: the message is somebody else's
    _, o = B.Walker("events", (None, "/l", None)).feed(CHUNK)
    assert len(o["events"][1]) == 2 and int(o["messages"][0]["cam"]) == 1
    _, o = B.Walker("events", ("/other", None, None)).feed(CHUNK)
    assert (len(o["events"][0]), o["other_messages"], o["connections"], len(o["messages"])) == (0, 1, 1, 0)
    # a second message continues the camera's stream: first = 2
    _, o = w.feed(B.chunk_record(MSG))
    assert [int(o["messages"][0][k]) for k in ("first", "count")] == [2, 2]


def test_a_bad_event_and_each_hand_made_malformation():
    role = ("/l", None, None)
    bad = CHUNK.replace(b"\xff\xc9\x9a\x3b", b"\x00\xca\x9a\x3b")  # nsec 10^9
    with pytest.raises(B.Bad) as e:
        B.Walker("events", role).feed(bad)
    assert e.value.bad == [1, 0]
    cases = {
        "compressed": CHUNK.replace(b"\x10\x00\x00\x00compression=none", b"\x0f\x00\x00\x00compression=bz2").replace(b"\x29\x00\x00\x00", b"\x28\x00\x00\x00", 1),
        "md5": CHUNK.replace(b"5e8b", b"5e8c"),
        "type": CHUNK.replace(b"dvs_msgs/EventArray", b"dvs_msgs/EventArrax"),
        "data_len": CHUNK.replace(b"\x02\x00\x00\x00" + EVENT_0, b"\x03\x00\x00\x00" + EVENT_0),
        "size": CHUNK.replace(b"size=\xd5", b"size=\xd4"),
        "no op": b"\x0d\x00\x00\x00" b"\x09\x00\x00\x00conn=\x00\x00\x00\x00" b"\x00\x00\x00\x00",
        "field overrun": b"\x08\x00\x00\x00" b"\x05\x00\x00\x00op=\x02" b"\x00\x00\x00\x00",
        "header_len": b"\x01\x10\x00\x00",
        "no =": b"\x07\x00\x00\x00" b"\x03\x00\x00\x00op\x02" b"\x00\x00\x00\x00",
        "index record inside a chunk": B.chunk_record(B.index_record(0, 1)),
        "record overruns the chunk": B.chunk_record(CONN + MSG[:-1], size=212),
    }
    for name, data in cases.items():
        with pytest.raises(B.Malformed):
            B.Walker("events", role).feed(data)
        with pytest.raises(B.Malformed):
            B.Walker("side", role).feed(data)
    # without a role nobody looks at the connection's type or the message's lengths
    for name in ("md5", "type", "data_len"):
        _, o = B.Walker("events", (None, None, None)).feed(cases[name])
        assert o["other_messages"] == 1


def test_small_bag_whole_and_the_header():
    s = B.small_bag()
    assert 1500 < len(s) < 4096
    o = B.decode(s)
    assert [len(e) for e in o["events"]] == [5, 4]
    assert o["events"][0]["polarity"].tolist() == [1, 0, 1, 0, 1] and o["events"][0]["nsec"].tolist() == [100, 200, 999_999_999, 0, 5]
    assert [tuple(int(v) for v in m) for m in o["messages"]] == [
        (0, 1, 10, 100, 10, 500, 260, 346, 0, 3), (1, 1, 10, 100, 10, 800, 260, 346, 0, 1), (0, 2, 10, 950, 11, 0, 260, 346, 3, 0),
        (1, 2, 11, 0, 11, 600, 260, 346, 1, 3), (0, 3, 11, 0, 11, 800, 260, 346, 3, 2)]
    # 2 chunks; 4 connections in the chunks and 4 again at the index; the image message; no record of another op
    assert (o["chunks"], o["connections"], o["other_messages"], o["other_records"]) == (2, 8, 1, 0)
    side = B.decode(s, "side")
    assert side["imu"]["sec"].tolist() == [10, 11] and side["imu"]["nsec"].tolist() == [50, 1]
    assert side["imu"]["gyr"].tolist() == [[0.1, -0.2, 0.3], [1.0, 2.0, 3.0]] and side["imu"]["acc"].tolist() == [[9.5, 0.25, -1.5], [-4.0, 5.0, -6.0]]
    assert (side["chunks"], side["connections"], side["other_messages"]) == (2, 8, 1)
    h = B.header(s)
    assert h[:1] + h[2:] == (13, 4, 2, 20, 1) and s[h[1]:h[1] + 4] == B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5)[:4]
    padded = B.small_bag(header_total=4096)
    assert B.decode(padded)["wire"] == o["wire"] and B.header(padded)[1] - h[1] == len(padded) - len(s)


def test_every_two_call_cut_of_small_bag_gives_the_whole():
    s = B.small_bag()[13:]
    for mode in ("events", "side"):
        whole = B.Walker(mode).feed(s)[1]
        for cut in range(len(s) + 1):
            w, a = B.Walker(mode).feed(s[:cut])
            w, b = w.feed(s[cut:])
            assert a["wire"][0] + b["wire"][0] == whole["wire"][0] and a["wire"][1] + b["wire"][1] == whole["wire"][1], cut
            assert np.concatenate([a["messages"], b["messages"]]).tobytes() == whole["messages"].tobytes(), cut
            assert np.concatenate([a["imu"], b["imu"]]).tobytes() == whole["imu"].tobytes(), cut
            for k in ("chunks", "connections", "other_messages", "other_records"):
                assert a[k] + b[k] == whole[k], (cut, k)
            # a message is listed by the call that brings its last byte
            assert len(a["messages"]) == sum(1 for m in whole["messages"] if _message_end(s, m) <= cut), cut


def _message_end(s, m):
    """where the last byte of message m's record lies in s: found by its time field, which is unique in small_bag"""
    import struct
    at = s.index(b"time=" + struct.pack("<II", int(m["time_sec"]), int(m["time_nsec"])))
    at = s.index(b"op=\x02", at) + 4
    return at + 4 + struct.unpack_from("<I", s, at)[0]
