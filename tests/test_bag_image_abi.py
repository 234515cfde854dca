"""CPU: the boundary of the rosbag image entry points that needs no device — the library exports them, the structs are
laid out by the C compiler as their ctypes mirrors say, a null handle is refused before anything else — and the host walk
in its image mode alone (esvio_fe_bag_image_walk_tap) against tests/bag_image_ref.py: at every cut, at cuts inside every
kind of structure, at every malformed cause and both refusals.  (The clash of an image topic with an event topic needs
both topic calls, so it is checked where they are: in the stand-alone walk program and on the device.)"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bag_image_ref as I
import bag_ref as B
from esvio_amd import frontend as FE
from esvio_amd.node import StereoImageTrackerNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (5, 3)
STRUCTS = {
    "esvio_fe_bag_image": (FE.BagImage, ["cam", "seq", "stamp_sec", "stamp_nsec", "time_sec", "time_nsec", "height", "width", "step", "encoding",
                                         "is_bigendian", "index"]),
    "esvio_fe_bag_image_cam_info": (FE.BagImageCamInfo, ["images", "first_sec", "first_nsec", "last_sec", "last_nsec"]),
    "esvio_fe_bag_image_info": (FE.BagImageInfo, ["cam", "other_messages", "other_records", "chunks", "connections"]),
    "esvio_fe_bag_topics": (FE.BagTopics, ["left", "right", "imu"]),  # (keeps its three fields)
}
ENTRY_POINTS = ("esvio_fe_bag_set_image_topics", "esvio_fe_decode_bag_images", "esvio_fe_convert_image", "esvio_fe_track_image_space")


def test_entry_points_are_exported_and_refuse_a_null_handle_before_the_device():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS, name
    assert "esvio_fe_bag_image_walk_tap" in FE.TEST_SYMBOLS
    info, tr, px = FE.BagImageInfo(), (C.c_uint8 * 512)(), np.zeros(16, np.uint8)
    assert L.esvio_fe_bag_set_image_topics(None, b"/l", b"/r") == -1
    assert L.esvio_fe_decode_bag_images(None, None, 0, 0, None, None, FE.HOST, None, 0, C.byref(info)) == -1
    assert L.esvio_fe_convert_image(None, FE._p(px), FE.HOST, 1, 1, 1, 1, FE._p(px), FE.HOST) == -1
    assert L.esvio_fe_track_image_space(None, 0.0, FE._p(px), None, FE.DEVICE, 1, C.byref(tr)) == -1
    assert FE.BAG_IMAGE_DTYPE == I.IMAGE_DTYPE and FE.BAG_IMAGE_DTYPE.itemsize == C.sizeof(FE.BagImage) == 56
    assert [FE.BAG_IMAGE_DTYPE.fields[n][1] for n in FE.BAG_IMAGE_DTYPE.names] == [getattr(FE.BagImage, n).offset for n in FE.BAG_IMAGE_DTYPE.names]
    assert (FE.ENC_MONO, FE.ENC_BGR, FE.ENC_RGB) == (1, 2, 3)


def test_the_new_kernel_is_appended_to_the_ingest_range():
    L = FE.load_library()
    stage, ingest = L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(ingest)]
    assert names[stage:ingest].index("k_image_emit") > names[stage:ingest].index("k_bag_emit") and "k_image_emit" not in names[:stage]
    assert names[stage - 2:stage] == ["k_trig_reduce", "k_trig_emit"]  # the stage table ends where it ended
    assert L.esvio_fe_image_tile_pixels() > 0 and L.esvio_fe_image_tile_pixels() % 256 == 0
    assert 64 * 8 < L.esvio_fe_bag_walk_state_bytes() < 8192  # the state that is copied per call stays small


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
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert (C.sizeof(FE.BagImageCamInfo), C.sizeof(FE.BagImageInfo), C.sizeof(FE.BagTopics)) == (24, 80, 24)


# ---- the host walk alone -------------------------------------------------------------------------------------------------
def payloads(pix, table):
    """the gathered bytes cut into the messages' payloads: each begins at a 16-byte boundary"""
    out, at = [], 0
    for m in table:
        n = int(m["step"]) * int(m["height"])
        out.append(pix[at:at + n])
        at += (n + 15) & ~15
    assert at == len(pix)
    return out


def tap_all(parts, topics=I.IMAGE_TOPICS, size=SIZE):
    st, pay, rows, tot = None, [], [], dict.fromkeys(I.COUNTERS, 0)
    for part in parts:
        st, pix, table, c = FE.bag_image_walk_tap(st, part, topics, size)
        assert (len(table), c[1] + c[2], len(pix), len(st[1])) == (c[0], c[0], c[3], c[8])
        pay += payloads(pix, table)
        rows.append(table)
        for k, v in zip(I.COUNTERS, c[4:8]):
            tot[k] += v
    return st, pay, rows, tot


def same_as_the_loop(s, parts, tag, size=SIZE):
    w, want_pay, want_rows = I.ImageWalker(size=size), [], []
    for part in parts:
        w, o = w.feed(part)
        want_pay += o["payloads"]
        want_rows.append(o["table"])
    st, pay, rows, tot = tap_all(parts, size=size)
    assert pay == want_pay, tag
    assert [r.tobytes() for r in rows] == [r.tobytes() for r in want_rows], tag  # call by call: the index counts per call
    whole = I.read_stream(s, size=size)[1]
    assert tot == whole, tag
    return st


def test_the_walk_equals_the_loop_at_every_byte_cut_in_two_calls():
    s = I.small_bag()[13:]
    st = same_as_the_loop(s, [s], "one call")
    assert st[1] == b""
    longest = 0
    for cut in range(len(s) + 1):
        st = same_as_the_loop(s, [s[:cut], s[cut:]], cut)
        assert st[1] == b""
        longest = max(longest, len(FE.bag_image_walk_tap(None, s[:cut], I.IMAGE_TOPICS, SIZE)[0][1]))
    assert longest == 3 * 31 - 1  # the bgr8 image of step 31: all of its payload but the last byte waited once
    # counting alone: no room for anything
    st, pix, table, c = FE.bag_image_walk_tap(None, s, I.IMAGE_TOPICS, SIZE, pix_cap=0, imgs_cap=0)
    assert c[:4] == (5, 3, 2, 16 + 64 + 48 + 96 + 32) and pix == b"" and len(table) == 0


def spans(bag, topics=I.IMAGE_TOPICS):
    """kind -> the (lo, hi) byte ranges of a bag (magic included) that are of that kind"""
    out = {k: [] for k in ("length word", "record header", "message header", "encoding string", "payload", "connection data")}
    conns = {}

    def walk(lo, hi):
        pos = lo
        while pos < hi:
            hl = struct.unpack_from("<I", bag, pos)[0]
            f = B.parse_fields(bag[pos + 4:pos + 4 + hl], "header")
            dl = struct.unpack_from("<I", bag, pos + 4 + hl)[0]
            d0, op = pos + 8 + hl, f[b"op"][0]
            out["length word"] += [(pos + 1, pos + 4), (d0 - 3, d0)]
            if op != 4:
                out["record header"].append((pos + 5, d0 - 4))
            if op == 7:
                conns[f[b"conn"]] = f[b"topic"].decode()
                out["connection data"].append((d0 + 1, d0 + dl))
            elif op == 2 and conns.get(f[b"conn"]) in topics:
                fl = struct.unpack_from("<I", bag, d0 + 12)[0]
                le = struct.unpack_from("<I", bag, d0 + 16 + fl + 8)[0]
                enc = d0 + 16 + fl + 12
                out["message header"].append((d0 + 1, enc))
                out["encoding string"].append((enc + 1, enc + le))
                out["length word"].append((enc + le + 6, enc + le + 9))  # (inside D)
                out["payload"].append((enc + le + 10, d0 + dl))
            if op == 5:
                walk(d0, d0 + dl)
            pos = d0 + dl

    walk(13, len(bag))
    return out


def test_the_walk_equals_the_loop_at_64_seeded_multi_cuts_each_inside_another_structure():
    bag = I.small_bag()
    places = spans(bag)
    assert all(len(v) > 0 for v in places.values()), {k: len(v) for k, v in places.items()}
    s, kinds, rng = bag[13:], sorted(places), np.random.default_rng(11)
    for it in range(64):
        chosen = rng.choice(len(kinds), int(rng.integers(2, 6)), replace=False)
        cuts = []
        for c in chosen:
            lo, hi = places[kinds[c]][int(rng.integers(0, len(places[kinds[c]])))]
            cuts.append(int(rng.integers(lo, hi)) - 13)
        cuts = sorted(cuts)
        same_as_the_loop(s, [s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])], ([kinds[c] for c in chosen], cuts))


def test_every_new_malformed_cause_and_both_refusals_fail_the_call_that_brings_the_items_last_byte_with_the_state_as_it_was():
    s = I.small_bag()[13:]
    s = s[:I.read_stream(s, size=SIZE)[0][-1]["end"]]  # up to the last image's last byte, which ends its chunk
    for name, (data, names) in I.bad_streams().items():
        for lead in (b"", s[:len(s) - 20]):  # from the fresh state, and behind a bag whose last image waits but for 20 bytes
            st, w = None, I.ImageWalker(size=SIZE)
            if lead:
                st, w = FE.bag_image_walk_tap(None, lead, I.IMAGE_TOPICS, SIZE)[0], w.feed(lead)[0]
                assert len(st[1]) == 3 * 8 - 20
            data_ = s[len(s) - 20:] + data if lead else data  # (conn 0 is nobody's to the image walk so far)
            fails_at = None
            for lo in range(0, len(data_), 5):  # the loop names the first call that fails when the stream comes in 5-byte pieces
                try:
                    w, _ = w.feed(data_[lo:lo + 5])
                except B.Malformed:
                    fails_at = lo
                    break
            assert fails_at is not None, name
            for lo in range(0, len(data_), 5):
                if lo < fails_at:
                    st = FE.bag_image_walk_tap(st, data_[lo:lo + 5], I.IMAGE_TOPICS, SIZE)[0]
                    continue
                with pytest.raises(FE.FrontendError) as e:
                    FE.bag_image_walk_tap(st, data_[lo:lo + 5], I.IMAGE_TOPICS, SIZE)
                assert lo == fails_at and names in str(e.value), (name, lo, fails_at, str(e.value))
                break
    # a failed call touches neither the state bytes nor the waiting bytes; the corrected continuation gives the loop's result
    st = FE.bag_image_walk_tap(None, s[:len(s) - 20], I.IMAGE_TOPICS, SIZE)[0]
    L = FE.load_library()
    state, carry = np.frombuffer(st[0], np.uint8).copy(), np.frombuffer(st[1] + b"\x5a" * 64, np.uint8).copy()
    before, counts, why = (state.copy(), carry.copy()), np.zeros(12, np.uint64), C.create_string_buffer(256)
    bad = np.frombuffer(s[len(s) - 20:] + b"\x01\x10\x00\x00", np.uint8)
    rc = L.esvio_fe_bag_image_walk_tap(FE._p(state), len(state), I.LEFT_IMAGE.encode(), I.RIGHT_IMAGE.encode(), 5, 3, FE._p(bad), len(bad), FE._p(carry),
                                       len(carry), None, 0, None, 0, FE._p(counts), why, 256)
    assert rc == -1 and b"header_len" in why.value and (state == before[0]).all() and (carry == before[1]).all()
    _, pix, table, c = FE.bag_image_walk_tap(st, s[len(s) - 20:], I.IMAGE_TOPICS, SIZE)
    assert payloads(pix, table) == [I.decode(I.small_bag(), size=SIZE)["payloads"][-1]] and c[0] == 1
    # any size is taken when none is asked for; the other size is refused by name
    assert FE.bag_image_walk_tap(None, s, I.IMAGE_TOPICS)[3][0] == 5
    with pytest.raises(FE.FrontendError, match="5 x 3"):
        FE.bag_image_walk_tap(None, s, I.IMAGE_TOPICS, (3, 5))


def test_the_caps_one_too_small():
    s = I.small_bag()[13:]
    need = FE.bag_image_walk_tap(None, s, I.IMAGE_TOPICS, SIZE)[3][3]
    st, pix, table, c = FE.bag_image_walk_tap(None, s, I.IMAGE_TOPICS, SIZE, pix_cap=need - 1)
    assert c[3] == need and pix == b"" and len(table) == 5  # the bytes needed come back, no payload is stored
    L = FE.load_library()
    state, counts = np.zeros(L.esvio_fe_bag_walk_state_bytes(), np.uint8), np.zeros(12, np.uint64)
    buf, room, rows = np.frombuffer(s, np.uint8), np.full(need, 0xA5, np.uint8), np.zeros(5, FE.BAG_IMAGE_DTYPE)
    rows.view(np.uint8)[:] = 0xA5
    carry = np.zeros(len(s), np.uint8)
    args = lambda pc, ic: (FE._p(state), len(state), I.LEFT_IMAGE.encode(), I.RIGHT_IMAGE.encode(), 5, 3, FE._p(buf), len(buf), FE._p(carry), len(carry),
                           FE._p(room), pc, FE._p(rows), ic, FE._p(counts), None, 0)
    assert L.esvio_fe_bag_image_walk_tap(*args(need - 1, 4)) == 0
    assert (room == 0xA5).all() and (rows[4:].view(np.uint8) == 0xA5).all() and counts[0] == 5
    assert rows[:4].tobytes() == I.decode(I.small_bag(), size=SIZE)["table"][:4].tobytes()


def test_the_topic_rules_and_the_argument_errors_of_the_tap():
    L = FE.load_library()
    state, counts = np.zeros(L.esvio_fe_bag_walk_state_bytes(), np.uint8), np.zeros(12, np.uint64)
    call = lambda left, right, **k: L.esvio_fe_bag_image_walk_tap(FE._p(state), k.get("n", len(state)), left, right, 0, 0, None, 0, None, 0, None, 0, None, 0,
                                                                  FE._p(counts), None, 0)
    assert call(b"/a", b"/b") == 0 and call(None, None) == 0 and call(None, b"/b") == 0 and call(b"/" + b"t" * 254, None) == 0
    for bad in ((b"/a", b"/a"), (b"", None), (None, b""), (b"/" + b"t" * 255, None)):
        assert call(*bad) == -1, bad
    assert call(b"/a", b"/b", n=len(state) - 1) == -1
    assert L.esvio_fe_bag_image_walk_tap(None, 0, None, None, 0, 0, None, 0, None, 0, None, 0, None, 0, None, None, 0) == -1
    # a topic without a role is nobody's: with the left topic alone the right camera's images are other messages
    s = I.small_bag()[13:]
    _, _, table, c = FE.bag_image_walk_tap(None, s, (I.LEFT_IMAGE, None), SIZE)
    assert table["cam"].tolist() == [0, 0, 0] and c[4] == 6
    _, _, table, c = FE.bag_image_walk_tap(None, s, (I.RIGHT_IMAGE, I.LEFT_IMAGE), SIZE)  # the roles swapped
    assert table["cam"].tolist() == [1, 0, 0, 1, 1]
    # the event topics' walk passes the images over as it did: they are other messages to it
    assert FE.bag_walk_tap(None, s, B.TOPICS)[4][7] == 5 + 1


# ---- the node's pairing, off line ------------------------------------------------------------------------------------------
def test_pair_images_applies_the_nodes_rule_to_a_table():
    def table(entries):
        t = np.zeros(len(entries), FE.BAG_IMAGE_DTYPE)
        for k, (cam, sec, nsec) in enumerate(entries):
            t[k]["cam"], t[k]["stamp_sec"], t[k]["stamp_nsec"], t[k]["seq"] = cam, sec, nsec, k
        return t
    pair = lambda e: [(int(l["seq"]), int(r["seq"]), t) for l, r, t in StereoImageTrackerNode.pair_images(table(e))]
    assert pair([(0, 10, 0), (1, 10, 0)]) == [(0, 1, 10.0)]
    assert pair([(1, 10, 500), (0, 10, 0)]) == [(1, 0, 10.0)]  # within 1 s: a pair, msg_timestamp the left stamp
    assert pair([(0, 10, 0), (1, 11, 0)]) == []  # a left image 1 s older: dropped (time_left <= time_right - 1)
    assert pair([(0, 10, 1), (1, 11, 0)]) == [(0, 1, 10.000000001)]
    assert pair([(0, 11, 0), (1, 10, 0)]) == [(0, 1, 11.0)]  # 1 s newer exactly: still a pair (time_left > time_right + 1 is false)
    assert pair([(0, 11, 1), (1, 10, 0), (1, 11, 0)]) == [(0, 2, 11.000000001)]  # more than 1 s newer: the right one is dropped
    assert pair([(0, 5, 0), (0, 10, 0), (1, 10, 0), (1, 20, 0), (0, 20, 0)]) == [(1, 2, 10.0), (4, 3, 20.0)]
    assert pair([(0, 10, 0)]) == [] and pair([]) == []
