"""CPU: the boundary of the AEDAT frame entry points that needs no device — the library exports them, the structs are laid
out by the C compiler as their ctypes mirrors say, a null handle is refused before anything else — and the host walk in
its frame mode alone (esvio_fe_aedat_frame_walk_tap) against tests/aedat_frame_ref.py: at every cut, byte by byte, behind
failed calls, and beside the other two walkers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aedat_frame_ref as F
import aedat_ref as A
from esvio_amd import frontend as FE
from esvio_amd.node import StereoImageTrackerNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (5, 3)
STRUCTS = {
    "esvio_fe_aedat_frame": (FE.AedatFrame, ["stamp_sec", "stamp_nsec", "ts_startframe", "ts_endframe", "ts_startexposure", "ts_endexposure",
                                             "exposure_us", "length_x", "length_y", "position_x", "position_y", "channels", "color_filter", "roi",
                                             "valid", "slot", "ts_overflow", "index"]),
    "esvio_fe_aedat_frame_info": (FE.AedatFrameInfo, ["frames", "invalid", "bad", "frame_packets", "other_packets", "first_sec", "first_nsec",
                                                      "last_sec", "last_nsec"]),
}
COUNTS = ("invalid", "bad", "frame_packets", "other_packets")


def test_entry_points_are_exported_and_refuse_a_null_handle_before_the_device():
    L = FE.load_library()
    for name in ("esvio_fe_decode_aedat_frames", "esvio_fe_convert_frame16"):
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS, name
    for name in ("esvio_fe_aedat_frame_walk_tap", "esvio_fe_aedat_frame_kernel_stats", "esvio_fe_frame16_tile_pixels"):
        assert hasattr(L, name) and name in FE.TEST_SYMBOLS, name
    info, px = FE.AedatFrameInfo(), np.zeros(16, np.uint16)
    assert L.esvio_fe_decode_aedat_frames(None, 0, None, 0, 0, 0, None, 0, FE.HOST, None, 0, C.byref(info)) == -1
    assert L.esvio_fe_convert_frame16(None, FE._p(px), FE.HOST, 1, 1, 1, FE._p(px), FE.HOST) == -1
    assert L.esvio_fe_aedat_frame_kernel_stats(None, None, None, None) == -1
    assert FE.AEDAT_FRAME_DTYPE.itemsize == C.sizeof(FE.AedatFrame) == 80 and C.sizeof(FE.AedatFrameInfo) == 56
    assert [FE.AEDAT_FRAME_DTYPE.fields[n][1] for n in FE.AEDAT_FRAME_DTYPE.names] == [getattr(FE.AedatFrame, n).offset for n in FE.AEDAT_FRAME_DTYPE.names]
    assert L.esvio_fe_frame16_tile_pixels() > 0 and L.esvio_fe_frame16_tile_pixels() % 256 == 0


def test_the_new_kernel_has_a_timer_slot_outside_every_pinned_table():
    L = FE.load_library()
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(L.esvio_fe_ingest_kernel_count() + 16)]
    assert "k_frame16_emit" not in names and names[L.esvio_fe_ingest_kernel_count() - 1] == "k_image_emit"
    assert "k_frame16_emit" not in [L.esvio_fe_kf_kernel_name(k).decode() for k in range(8)] + [L.esvio_fe_bow_kernel_name(k).decode() for k in range(8)]
    assert 64 < L.esvio_fe_aedat_walk_state_bytes() < 256  # the state that is copied per call stays small: the pixels wait beside it


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', '#include "esvio_fe_test.h"', "int main(void) {"]
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


def test_the_header_says_what_is_cited_what_is_recalled_and_what_the_slot_0_rows_are():
    hdr = " ".join(open(os.path.join(ROOT, "include", "esvio_fe.h")).read().split())
    at = hdr.index("AEDAT 3.1 frames: the DAVIS frame packets")
    text = hdr[at:hdr.index("rosbag v2.0 recordings:", at)].replace(" * ", " ")
    for cite in ("driver.cpp:778-823", ":788-804", ":807-814", ":817-818", ":823", "stereo_image_tracker_node.cpp:296-301", ":781",
                 "RESTATED FROM RECALL AND UNPINNED", "THIS TEXT IS THE SPECIFICATION",
                 "THE ROWS WITH slot == 0 UNDER ESVIO_FE_AEDAT_KEEP_INVALID ARE EXACTLY THE DRIVER'S FRAMES", "computeNewExposure"):
        assert cite in text, cite


# ---- the host walk alone -------------------------------------------------------------------------------------------------
def pixel_blocks(pix, table):
    """the gathered bytes cut into the frames' pixel bytes: each begins at a 16-byte boundary"""
    out, at = [], 0
    for m in table:
        n = int(m["length_x"]) * int(m["length_y"]) * int(m["channels"]) * 2
        out.append(pix[at:at + n])
        at += (n + 15) & ~15
    assert at == len(pix)
    return out


def same_as_the_reading(parts, tag, size=SIZE, t_offset_ns=0, flags=0, start=None):
    """the tap and the reading side by side, call by call -> (tap state, reading state)"""
    st, w = start if start else (None, F.FrameWalker(size))
    for part in parts:
        w, o = w.feed(part, t_offset_ns, flags)
        st, pix, table, c = FE.aedat_frame_walk_tap(st, part, size, t_offset_ns, flags)
        assert (len(table), len(pix)) == (c[0], c[1]), tag
        assert pixel_blocks(pix, table) == o["pixels"], tag
        assert table.tobytes() == o["table"].tobytes(), tag  # (the index counts per call)
        assert c[2:6] == tuple(o[k] for k in COUNTS), tag
        assert len(st[1]) == c[6] == (w.ev_off - 36 if w.emit is not None else 0), tag
    return st, w


def test_the_walk_equals_the_reading_on_the_small_stream_cut_in_two_at_every_byte():
    s = F.small_stream()
    whole = F.decode(s, size=SIZE)
    assert len(whole["rows"]) == 4 and {r["channels"] for r in whole["rows"]} == {1, 3} and whole["invalid"] == 1
    st, _ = same_as_the_reading([s], "one call")
    assert st[1] == b""
    longest = 0
    for cut in range(len(s) + 1):
        st, _ = same_as_the_reading([s[:cut], s[cut:]], cut)
        assert st[1] == b""
        longest = max(longest, len(FE.aedat_frame_walk_tap(None, s[:cut], SIZE)[0][1]))
    assert longest == 5 * 3 * 3 * 2 - 1  # a colour frame: all of its pixel bytes but the last waited once
    for flags in (0, F.KEEP_INVALID):
        same_as_the_reading([s[:200], s[200:]], ("flags", flags), flags=flags, t_offset_ns=123456789)
    # counting alone: no room for anything
    _, pix, table, c = FE.aedat_frame_walk_tap(None, s, SIZE, pix_cap=0, frames_cap=0)
    assert c[:2] == (4, 32 + 96 + 32 + 96) and pix == b"" and len(table) == 0


def test_the_walk_equals_the_reading_byte_by_byte():
    s = F.small_stream()
    st, w = same_as_the_reading([s[k:k + 1] for k in range(len(s))], "byte by byte", flags=F.KEEP_INVALID)
    assert st[1] == b"" and w.payload_left == 0


def test_a_failed_call_behind_every_seventh_cut_leaves_state_and_carry_as_they_were():
    s = F.small_stream()
    bad = sorted(F.bad_streams().items())
    L = FE.load_library()
    for k, cut in enumerate(range(0, len(s) + 1, 7)):
        name, (data, kind, names) = bad[k % len(bad)]
        start = same_as_the_reading([s[:cut]], (cut, "lead"))
        with pytest.raises(kind):
            start[1].feed(s[cut:] + data)
        # through the raw entry point: neither the state bytes nor the waiting bytes are touched
        state, carry = np.frombuffer(start[0][0], np.uint8).copy(), np.frombuffer(start[0][1] + b"\x5a" * 64, np.uint8).copy()
        before, counts, why = (state.copy(), carry.copy()), np.zeros(8, np.uint64), C.create_string_buffer(256)
        chunk = np.frombuffer(s[cut:] + data, np.uint8)
        carry_room = np.concatenate([carry, np.zeros(len(chunk), np.uint8)])
        rc = L.esvio_fe_aedat_frame_walk_tap(FE._p(state), len(state), 5, 3, FE._p(chunk), len(chunk), 0, 0, FE._p(carry_room), len(carry_room), None, 0,
                                             None, 0, FE._p(counts), why, 256)
        assert rc == -1 and (state == before[0]).all() and (carry_room[:len(carry)] == before[1]).all(), (name, cut)
        if names:
            assert names.encode() in why.value, (name, cut, why.value)
        else:
            assert b"BAD" in why.value and counts[3] == 1, (name, cut, why.value)
        same_as_the_reading([s[cut:]], (cut, "after the failure"), start=start)


def test_every_malformed_and_refused_case_fails_in_the_call_that_brings_the_heads_last_byte():
    lead = F.small_stream()
    for name, (data, kind, names) in sorted(F.bad_streams().items()):
        st, w = same_as_the_reading([lead], "lead")
        fails_at = None
        for lo in range(0, len(data), 5):  # the reading names the first call that fails when the stream comes in 5-byte pieces
            try:
                w, _ = w.feed(data[lo:lo + 5])
            except (F.Malformed, F.Bad):
                fails_at = lo
                break
        assert fails_at is not None, name
        for lo in range(0, len(data), 5):
            if lo < fails_at:
                st = FE.aedat_frame_walk_tap(st, data[lo:lo + 5], SIZE)[0]
                continue
            with pytest.raises(FE.FrontendError) as e:
                FE.aedat_frame_walk_tap(st, data[lo:lo + 5], SIZE)
            assert lo == fails_at and (names or "BAD") in str(e.value), (name, lo, fails_at, str(e.value))
            break
    # any size is taken when none is asked for; the other size is refused by name
    assert FE.aedat_frame_walk_tap(None, lead)[3][0] == 4
    with pytest.raises(FE.FrontendError, match="5 x 3"):
        FE.aedat_frame_walk_tap(None, lead, (3, 5))


def test_the_three_walkers_over_the_same_bytes_do_not_disturb_each_other():
    s = F.small_stream()
    whole_f, whole_e = F.decode(s, size=SIZE), A.decode(s)
    assert whole_e["other_packets"] == 3 + 1  # the existing event walk still counts the frame packets as other packets
    cuts = [0, 29, 100, 101, 300, len(s)]
    ev_state, fr_state, records, rows, pixels, other = None, None, [], [], [], 0
    for lo, hi in zip(cuts, cuts[1:]):
        fr_state, pix, table, c = FE.aedat_frame_walk_tap(fr_state, s[lo:hi], SIZE)
        pixels += pixel_blocks(pix, table)
        rows += [r.tobytes()[:-8] for r in table]
        ev_state, runs, pay, counts = FE.aedat_walk_tap(ev_state, s[lo:hi])
        records.append(pay)
        other += counts[3]
    assert pixels == whole_f["pixels"] and rows == [r.tobytes()[:-8] for r in whole_f["table"]]
    assert b"".join(records) == b"".join(r for r, _ in whole_e["records"]) and other == 4
    assert len(A.decode(s, mode="side")["imu"]) == 1


def test_the_caps_one_too_small_and_the_argument_errors_of_the_tap():
    s = F.small_stream()
    need = FE.aedat_frame_walk_tap(None, s, SIZE)[3][1]
    st, pix, table, c = FE.aedat_frame_walk_tap(None, s, SIZE, pix_cap=need - 1)
    assert c[1] == need and pix == b"" and len(table) == 4  # the bytes needed come back, no pixel is stored
    L = FE.load_library()
    state, counts = np.zeros(L.esvio_fe_aedat_walk_state_bytes(), np.uint8), np.zeros(8, np.uint64)
    buf, room, rows = np.frombuffer(s, np.uint8), np.full(need, 0xA5, np.uint8), np.zeros(4, FE.AEDAT_FRAME_DTYPE)
    rows.view(np.uint8)[:] = 0xA5
    carry = np.zeros(len(s), np.uint8)
    args = lambda pc, ic, n=len(state): (FE._p(state), n, 5, 3, FE._p(buf), len(buf), 0, 0, FE._p(carry), len(carry), FE._p(room), pc, FE._p(rows), ic,
                                         FE._p(counts), None, 0)
    assert L.esvio_fe_aedat_frame_walk_tap(*args(need - 1, 3)) == 0
    assert (room == 0xA5).all() and (rows[3:].view(np.uint8) == 0xA5).all() and counts[0] == 4
    assert rows[:3].tobytes() == F.decode(s, size=SIZE)["table"][:3].tobytes()
    assert L.esvio_fe_aedat_frame_walk_tap(*args(need, 4, len(state) - 1)) == -1
    assert L.esvio_fe_aedat_frame_walk_tap(None, 0, 0, 0, None, 0, 0, 0, None, 0, None, 0, None, 0, None, None, 0) == -1


def test_merged_frame_tables_pair_as_the_node_pairs():
    def table(stamps):
        t = np.zeros(len(stamps), FE.AEDAT_FRAME_DTYPE)
        for k, (sec, nsec) in enumerate(stamps):
            t[k]["stamp_sec"], t[k]["stamp_nsec"], t[k]["index"] = sec, nsec, k
        return t
    merged = StereoImageTrackerNode.merge_frame_tables(table([(5, 0), (10, 0), (20, 0)]), table([(10, 500), (20, 0)]))
    assert merged.dtype.names[0] == "cam" and merged["cam"].tolist() == [0, 0, 0, 1, 1] and merged["index"].tolist() == [0, 1, 2, 0, 1]
    pairs = StereoImageTrackerNode.pair_images(merged)
    assert [(int(l["index"]), int(r["index"]), t) for l, r, t in pairs] == [(1, 0, 10.0), (2, 1, 20.0)]
    assert len(StereoImageTrackerNode.merge_frame_tables(table([]), table([(1, 1)]))) == 1
