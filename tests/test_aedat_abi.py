"""CPU: the boundary of the AEDAT 3.1 entry points that needs no device — the library exports them, the structs are laid
out by the C compiler as their ctypes mirrors say, a null handle is refused — the whole of esvio_fe_aedat_header, which is
host only, and the host walk alone (esvio_fe_aedat_walk_tap) against tests/aedat_ref.py at every cut."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import aedat_ref as A
from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "esvio_fe_aedat_info": (FE.AedatInfo, ["events", "invalid", "bad", "polarity_packets", "other_packets", "first_t_us", "last_t_us"]),
    "esvio_fe_imu_sample": (FE.ImuSample, ["sec", "nsec", "acc", "gyr"]),
    "esvio_fe_aedat_side_info": (FE.AedatSideInfo, ["imu", "triggers", "resets", "other_specials", "invalid", "bad", "special_packets",
                                                    "imu_packets", "other_packets"]),
    "esvio_fe_aedat_header_info": (FE.AedatHeaderInfo, ["payload_offset", "version", "complete"]),
}
ENTRY_POINTS = ("esvio_fe_aedat_header", "esvio_fe_decode_aedat", "esvio_fe_aedat_side", "esvio_fe_track_aedat", "esvio_fe_feed_push_aedat")


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    info, side, feed, binfo, pair = FE.AedatInfo(), FE.AedatSideInfo(), FE.FeedInfo(), FE.BatchInfo(), (FE.AedatInfo * 2)()
    assert L.esvio_fe_decode_aedat(None, 0, None, 0, 0, 0, None, 0, FE.HOST, C.byref(info)) == -1
    assert L.esvio_fe_aedat_side(None, 0, None, 0, 0, 0, None, 0, None, 0, C.byref(side)) == -1
    assert L.esvio_fe_track_aedat(None, None, 0, None, 0, 0, 0, 1, None, None, None, C.byref(binfo), C.byref(pair)) == -1
    assert L.esvio_fe_feed_push_aedat(None, 0, None, 0, 0, 0, C.byref(feed)) == -1
    assert FE.IMU_DTYPE.itemsize == C.sizeof(FE.ImuSample) == 56 and FE.IMU_DTYPE == A.IMU_DTYPE
    assert [FE.IMU_DTYPE.fields[n][1] for n in ("sec", "nsec", "acc", "gyr")] == [0, 4, 8, 32]
    assert FE.AEDAT_KEEP_INVALID == A.KEEP_INVALID == 1


def test_the_new_kernels_are_a_range_of_their_own_behind_the_stage_table():
    L = FE.load_library()
    stage, ingest = L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()
    assert ingest >= stage
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(ingest)]
    for n in ("k_aedat_count", "k_aedat_scan", "k_aedat_emit"):
        assert n in names[stage:ingest] and n not in names[:stage]
    assert names[stage - 2:stage] == ["k_trig_reduce", "k_trig_emit"]  # the stage table ends where it ended
    assert L.esvio_fe_kernel_name(ingest).decode() == ""
    assert L.esvio_fe_aedat_tile_events() > 0 and L.esvio_fe_aedat_tile_events() % 64 == 0


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {"]
    want = []
    for name, (mirror, members) in STRUCTS.items():
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        assert [m for m, _ in mirror._fields_] == members
        want += [C.sizeof(mirror)] + [getattr(mirror, m).offset for m in members]
    lines += ['  printf("%u\\n", ESVIO_FE_AEDAT_KEEP_INVALID);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want + [FE.AEDAT_KEEP_INVALID]
    assert C.sizeof(FE.AedatInfo) == 56 and C.sizeof(FE.AedatSideInfo) == 72 and C.sizeof(FE.AedatHeaderInfo) == 16


# ---- esvio_fe_aedat_header ----------------------------------------------------------------------------------------------
def hdr(data):
    i = FE.aedat_header(data)
    return (int(i.payload_offset), i.version, i.complete)


def test_the_header_on_both_line_endings():
    for nl in (b"\n", b"\r\n"):
        h = nl.join([b"#!AER-DAT3.1", b"#Format: RAW", b"#Source 1: DAVIS346", b"#Start-Time: 2019-01-01 10:00:00 (TZ+0100)", b"#!END-HEADER", b""])
        for first in (0x00, 0x01):  # a payload that begins with a special or a polarity packet's type byte
            assert hdr(h + bytes([first, 0x00, 0x01, 0x00])) == (len(h), 31, 1)
        assert hdr(h) == (len(h), 31, 1)  # (the end line is the end even when nothing follows)
        assert hdr(h + b"#not a header line\n") == (len(h), 31, 1)  # behind the end line nothing is header
    assert hdr(b"#!AER-DAT2.0\n#!END-HEADER\n") == (26, 20, 1)
    assert hdr(b"#!AER-DAT12.3\r\n\x01") == (15, 123, 1)
    for text in (b"#!AER-DAT\n", b"#!AER-DAT3\n", b"#!AER-DAT3.x\n", b"#!AER-DAT3.11\n", b"# AER-DAT3.1\n", b"#comment\n#!AER-DAT3.1\n"):
        assert hdr(text + b"\x01") == (len(text), 0, 1), text


def test_a_missing_end_line_no_header_and_empty_input():
    h = b"#!AER-DAT3.1\n#Format: RAW\n"
    assert hdr(h + b"\x01\x00") == (len(h), 31, 1)  # the first line of another kind ends it
    assert hdr(h) == (len(h), 31, 0)                # directly behind a whole line that is not the end line: not known yet
    assert hdr(b"\x01\x00\x01\x00") == (0, 0, 1) and hdr(b"\n#!AER-DAT3.1\n") == (0, 0, 1)
    assert hdr(b"") == (0, 0, 0)
    L = FE.load_library()
    info = FE.AedatHeaderInfo()
    assert L.esvio_fe_aedat_header(None, 4, C.byref(info)) == -1 and L.esvio_fe_aedat_header(b"#!", 2, None) == -1
    assert L.esvio_fe_aedat_header(None, 0, C.byref(info)) == 0 and info.complete == 0


def test_a_header_cut_at_every_byte():
    h = b"#!AER-DAT3.1\r\n#Format: RAW\r\n#!END-HEADER\r\n"
    whole = h + A.small_stream()[:40]
    first, second = len(b"#!AER-DAT3.1\r\n"), len(b"#!AER-DAT3.1\r\n#Format: RAW\r\n")
    for n in range(len(whole) + 1):
        off, version, complete = hdr(whole[:n])
        assert complete == (1 if n >= len(h) else 0), n
        assert off == (len(h) if n >= len(h) else second if n >= second else first if n >= first else 0), n
        assert version == (31 if n >= first else 0), n


# ---- the host walk alone ------------------------------------------------------------------------------------------------
def tap_all(chunks):
    """the chunks through the tap, one state carried: (records with their overflow, packet counts)"""
    st, recs, pp, op = None, [], 0, 0
    for ch in chunks:
        st, runs, pay, counts = FE.aedat_walk_tap(st, ch)
        assert counts[0] * 8 == len(pay) and counts[1] == len(runs)
        assert (counts[0] == 0) == (len(runs) == 0) and (len(runs) == 0 or runs[0][0] == 0)
        assert all(runs[k][0] < runs[k + 1][0] and runs[k][1] != runs[k + 1][1] for k in range(len(runs) - 1))
        for i in range(counts[0]):
            ovf = [int(o) for f, o in runs if f <= i][-1]
            recs.append((pay[8 * i:8 * i + 8], ovf))
        pp, op = pp + counts[2], op + counts[3]
    return st, recs, pp, op


def test_the_walk_equals_the_loop_at_every_cut_and_at_random_multi_cuts():
    s = A.small_stream()
    want = A.decode(s)
    fresh = bytes(FE.load_library().esvio_fe_aedat_walk_state_bytes())
    for cut in range(len(s) + 1):
        st, recs, pp, op = tap_all([s[:cut], s[cut:]])
        assert recs == want["records"] and (pp, op) == (3, 1), cut
        # between packets: only the remembered header bytes and type of the last packet differ from the fresh state
        assert len(st) == len(fresh)
    rng = np.random.default_rng(7)
    for _ in range(200):
        cuts = sorted(rng.integers(0, len(s) + 1, int(rng.integers(2, 9))).tolist())
        parts = [s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])]
        st, recs, pp, op = tap_all(parts)
        assert recs == want["records"] and (pp, op) == (3, 1), cuts
    # counting alone: no room for anything
    st, runs, pay, counts = FE.aedat_walk_tap(None, s, runs_cap=0, events_cap=0)
    assert counts == (12, 2, 3, 1)


def test_every_malformed_header_is_refused_with_the_state_unchanged():
    ok = A.polarity(1, 1, 1, 7)
    H = lambda etype, size=8, capacity=1, number=1, ts_offset=4: A.HEADER.pack(etype, 1, size, ts_offset, 0, capacity, number, 0)
    bad = [H(1, size=0), H(7, size=-8), H(1, capacity=-1, number=0), H(1, number=-1), H(1, number=2), H(1, size=12),
           H(0, ts_offset=0), H(3, size=8), H(3, size=36, ts_offset=8), H(1, capacity=0x7FFFFFFF, number=-0x80000000),
           H(2, size=0x7FFFFFFF, capacity=0x7FFFFFFF, number=-1)]
    s = A.small_stream()
    st0, _, _, _ = FE.aedat_walk_tap(None, s[:100])  # inside the second polarity packet's header, which ends at byte 124
    st1, _, _, _ = FE.aedat_walk_tap(st0, s[100:124])
    L = FE.load_library()
    for h in bad:
        with pytest.raises(A.Malformed):
            A.decode(h + ok)
        for st in (None, st1):
            buf = np.frombuffer(h + ok, np.uint8)
            state = np.frombuffer(st if st is not None else bytes(L.esvio_fe_aedat_walk_state_bytes()), np.uint8).copy()
            before, counts = state.copy(), np.zeros(4, np.uint64)
            # behind whatever the open packet still expects comes the malformed header
            lead = np.frombuffer(s[124:164] if st is not None else b"", np.uint8)
            chunk = np.concatenate([lead, buf])
            rc = L.esvio_fe_aedat_walk_tap(FE._p(state), len(state), FE._p(chunk), len(chunk), None, 0, None, 0, FE._p(counts))
            assert rc == -1 and (state == before).all(), h
    assert L.esvio_fe_aedat_walk_tap(None, 0, None, 0, None, 0, None, 0, None) == -1
