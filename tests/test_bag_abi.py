"""CPU: the boundary of the rosbag entry points that needs no device — the library exports them, the structs are laid out
by the C compiler as their ctypes mirrors say, a null handle is refused — the whole of esvio_fe_bag_header, which is host
only, and the host walk alone (esvio_fe_bag_walk_tap) against tests/bag_ref.py at every cut."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bag_ref as B
from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "esvio_fe_bag_topics": (FE.BagTopics, ["left", "right", "imu"]),
    "esvio_fe_bag_header_info": (FE.BagHeaderInfo, ["payload_offset", "index_pos", "conn_count", "chunk_count", "version", "complete"]),
    "esvio_fe_bag_message": (FE.BagMessage, ["cam", "seq", "stamp_sec", "stamp_nsec", "time_sec", "time_nsec", "height", "width", "first", "count"]),
    "esvio_fe_bag_cam_info": (FE.BagCamInfo, ["events", "bad", "messages", "first_sec", "first_nsec", "last_sec", "last_nsec"]),
    "esvio_fe_bag_info": (FE.BagInfo, ["cam", "other_messages", "other_records", "chunks", "connections"]),
    "esvio_fe_bag_side_info": (FE.BagSideInfo, ["imu", "bad", "other_messages", "other_records", "chunks", "connections"]),
}
ENTRY_POINTS = ("esvio_fe_bag_header", "esvio_fe_bag_set_topics", "esvio_fe_decode_bag", "esvio_fe_bag_side", "esvio_fe_feed_push_bag")


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    info, side, feed = FE.BagInfo(), FE.BagSideInfo(), (FE.FeedInfo * 2)()
    assert L.esvio_fe_bag_set_topics(None, C.byref(FE.BagTopics(b"/l", b"/r", None))) == -1
    assert L.esvio_fe_decode_bag(None, None, 0, 0, None, None, FE.HOST, None, 0, C.byref(info)) == -1
    assert L.esvio_fe_bag_side(None, None, 0, 0, None, 0, C.byref(side)) == -1
    assert L.esvio_fe_feed_push_bag(None, None, 0, 0, C.byref(feed)) == -1
    assert FE.BAG_MESSAGE_DTYPE == B.MESSAGE_DTYPE and FE.BAG_MESSAGE_DTYPE.itemsize == C.sizeof(FE.BagMessage) == 48
    assert [FE.BAG_MESSAGE_DTYPE.fields[n][1] for n in FE.BAG_MESSAGE_DTYPE.names] == [getattr(FE.BagMessage, n).offset for n in FE.BAG_MESSAGE_DTYPE.names]
    assert FE.IMU_DTYPE == B.IMU_DTYPE


def test_the_new_kernel_is_appended_to_the_ingest_range():
    L = FE.load_library()
    stage, ingest = L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(ingest)]
    assert "k_bag_emit" in names[stage:ingest] and "k_bag_emit" not in names[:stage]
    assert names[stage:ingest].index("k_bag_emit") > names[stage:ingest].index("k_aedat_emit")  # behind K_AEDAT_EMIT
    assert names[stage - 2:stage] == ["k_trig_reduce", "k_trig_emit"]  # the stage table ends where it ended
    assert L.esvio_fe_kernel_name(ingest).decode() == ""
    assert L.esvio_fe_bag_tile_events() > 0 and L.esvio_fe_bag_tile_events() % 64 == 0


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {"]
    want = []
    for name, (mirror, members) in STRUCTS.items():
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        assert [m for m, _ in mirror._fields_] == members
        want += [C.sizeof(mirror)] + [getattr(mirror, m).offset for m in members]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want
    assert (C.sizeof(FE.BagHeaderInfo), C.sizeof(FE.BagCamInfo), C.sizeof(FE.BagInfo), C.sizeof(FE.BagSideInfo)) == (32, 40, 112, 48)


# ---- esvio_fe_bag_header -------------------------------------------------------------------------------------------------
def hdr(data):
    i = FE.bag_header(data)
    return (int(i.payload_offset), int(i.index_pos), i.conn_count, i.chunk_count, i.version, i.complete)


def test_the_header_of_a_padded_and_an_unpadded_bag():
    for total in (None, 4096):
        s = B.small_bag(header_total=total)
        assert hdr(s) == B.header(s) and hdr(s)[2:] == (4, 2, 20, 1)
        if total:
            assert hdr(s[:13 + 4096]) == B.header(s) and s[13 + 4096 + 4 + 41 - 4:][:4] == b"op=\x05"  # the record is 4096 bytes
    L = FE.load_library()
    info = FE.BagHeaderInfo()
    assert L.esvio_fe_bag_header(None, 4, C.byref(info)) == -1 and L.esvio_fe_bag_header(b"#R", 2, None) == -1
    assert L.esvio_fe_bag_header(None, 0, C.byref(info)) == 0 and (info.complete, info.version) == (0, 0)
    good = B.MAGIC + B.bag_header_record(77, 3, 2, None)
    assert hdr(good) == (13, 77, 3, 2, 20, 1)
    for bad in (b"#ROSBAG V1.2\n" + good[13:], b"x", B.MAGIC + b"\x01\x10\x00\x00", B.MAGIC + B.chunk_record(b""),
                B.MAGIC + B.record([("op", b"\x03"), ("index_pos", b"\0" * 8), ("conn_count", b"\0" * 4)], b""),
                B.MAGIC + B.record([("op", b"\x03"), ("index_pos", b"\0" * 4), ("conn_count", b"\0" * 4), ("chunk_count", b"\0" * 4)], b"")):
        with pytest.raises(B.Malformed):
            B.header(bad)
        with pytest.raises(FE.FrontendError):
            FE.bag_header(bad)


def test_a_header_cut_at_every_byte():
    s = B.small_bag()
    end = 13 + 4 + int(np.frombuffer(s[13:17], "<u4")[0]) + 4
    for n in range(end + 40):
        got = hdr(s[:n])
        assert got == B.header(s[:n]), n
        assert got[5] == (1 if n >= end else 0) and got[0] == (13 if n >= 13 else 0), n


# ---- the host walk alone -------------------------------------------------------------------------------------------------
COUNTS = ("chunks", "connections", "other_messages", "other_records")


def tap_all(chunks, side=False, topics=B.TOPICS):
    st, wire, msgs, imu, tot = None, [b"", b""], [], [], dict.fromkeys(COUNTS, 0)
    for ch in chunks:
        st, pay, m, i, c = FE.bag_walk_tap(st, ch, topics, side)
        assert (len(pay[0]), len(pay[1]), len(m), len(i)) == (13 * c[0], 13 * c[1], c[4], c[5]) and c[2] + c[3] == c[4]
        wire = [wire[0] + pay[0], wire[1] + pay[1]]
        msgs.append(m)
        imu.append(i)
        for k, v in zip(("other_messages", "other_records", "chunks", "connections"), c[7:11]):
            tot[k] += v
    return st, wire, np.concatenate(msgs), np.concatenate(imu), tot


def test_the_walk_equals_the_loop_at_every_cut_and_at_random_multi_cuts():
    s = B.small_bag()[13:]
    for side in (False, True):
        want = B.Walker("side" if side else "events").feed(s)[1]

        def same(parts, tag):
            st, wire, msgs, imu, tot = tap_all(parts, side)
            assert wire == ([b"", b""] if side else want["wire"]), tag
            assert msgs.tobytes() == (b"" if side else want["messages"].tobytes()), tag
            assert imu.tobytes() == want["imu"].tobytes(), tag
            assert tot == {k: want[k] for k in COUNTS}, tag

        for cut in range(len(s) + 1):
            same([s[:cut], s[cut:]], cut)
        rng = np.random.default_rng(7)
        for _ in range(200):
            cuts = sorted(rng.integers(0, len(s) + 1, int(rng.integers(2, 9))).tolist())
            same([s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])], cuts)
    # counting alone: no room for anything
    st, pay, m, i, c = FE.bag_walk_tap(None, s, B.TOPICS, events_cap=0, msgs_cap=0, imu_cap=0)
    assert c[:5] == (5, 4, 3, 2, 5) and pay == (b"", b"")
    # each call's own share equals the loop's, call by call, and the message table's `first` carries over
    w, st = B.Walker("events"), None
    for lo in range(0, len(s), 97):
        w, o = w.feed(s[lo:lo + 97])
        st, pay, m, i, c = FE.bag_walk_tap(st, s[lo:lo + 97], B.TOPICS)
        assert list(pay) == o["wire"] and m.tobytes() == o["messages"].tobytes(), lo


def test_every_malformed_cause_is_refused_with_the_state_unchanged_in_the_call_the_loop_names():
    s = B.small_bag()[13:]
    L = FE.load_library()
    assert 64 * 8 < L.esvio_fe_bag_walk_state_bytes() < 8192
    for side in (False, True):
        lead_st, _, _, _, _ = FE.bag_walk_tap(None, s, B.TOPICS, side)  # behind a whole bag: between records, 4 connections known
        lead_w = B.Walker("side" if side else "events").feed(s)[0]
        for name, data in B.malformed_streams().items():
            if name.startswith("a repeated conn id") or name.startswith("65 conn"):
                starts = ((None, B.Walker("side" if side else "events")),)  # (conn 0 is the left topic's behind small_bag too)
            else:
                starts = ((None, B.Walker("side" if side else "events")), (lead_st, lead_w))
            for st, w in starts:
                # the loop names the first call that fails when the stream comes in 5-byte pieces
                fails_at = None
                for lo in range(0, len(data), 5):
                    try:
                        w, _ = w.feed(data[lo:lo + 5])
                    except B.Malformed:
                        fails_at = lo
                        break
                assert fails_at is not None, name
                for lo in range(0, len(data), 5):
                    if lo < fails_at:
                        st = FE.bag_walk_tap(st, data[lo:lo + 5], B.TOPICS, side)[0]
                        continue
                    with pytest.raises(FE.FrontendError) as e:
                        FE.bag_walk_tap(st, data[lo:lo + 5], B.TOPICS, side)
                    assert (lo, len(str(e.value)) > 30) == (fails_at, True), (name, str(e.value))
                    break
    with pytest.raises(FE.FrontendError, match="rosbag decompress"):
        FE.bag_walk_tap(None, B.malformed_streams()["a compressed chunk"])
    with pytest.raises(FE.FrontendError, match=B.RIGHT):
        FE.bag_walk_tap(None, B.malformed_streams()["another type on an event topic"], B.TOPICS)
    # the state bytes of a failed call are untouched
    state = np.frombuffer(lead_st, np.uint8).copy()
    before, counts, buf = state.copy(), np.zeros(12, np.uint64), np.frombuffer(b"\x01\x10\x00\x00", np.uint8)
    rc = L.esvio_fe_bag_walk_tap(FE._p(state), len(state), C.byref(FE.BagTopics()), 0, FE._p(buf), 4, None, None, None, 0, None, 0, FE._p(counts), None, 0)
    assert rc == -1 and (state == before).all()
    assert L.esvio_fe_bag_walk_tap(None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, None, 0) == -1
    # topics: two roles on one topic, an empty one, one of 256 bytes
    for bad in ((b"/a", b"/a", None), (b"", None, None), (None, None, b"/" + b"t" * 255)):
        assert L.esvio_fe_bag_walk_tap(FE._p(state), len(state), C.byref(FE.BagTopics(*bad)), 0, None, 0, None, None, None, 0, None, 0, FE._p(counts), None, 0) == -1
