"""CPU: the boundary of the EVT2.1, trigger, explicit-window and file-header entry points that needs no device — the
library exports them, the structs are laid out by the C compiler as their ctypes mirrors say, a null handle is refused —
and the whole of esvio_fe_raw_header, which is host only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "esvio_fe_trigger": (FE.Trigger, ["sec", "nsec", "id", "value", "_pad"]),
    "esvio_fe_trigger_info": (FE.TriggerInfo, ["triggers", "untimed", "bad", "wraps", "first_t_us", "last_t_us"]),
    "esvio_fe_raw_header_info": (FE.RawHeaderInfo, ["payload_offset", "format", "width", "height", "complete"]),
}
ENTRY_POINTS = ("esvio_fe_decode_triggers", "esvio_fe_slice_events_at", "esvio_fe_raw_header")


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    tinfo, sinfo, cuts, trig = FE.TriggerInfo(), FE.SliceInfo(), (C.c_uint64 * 4)(), (FE.Trigger * 4)()
    assert L.esvio_fe_decode_triggers(None, 0, FE.RAW_EVT3, None, 0, FE.HOST, 0, C.byref(trig), 4, C.byref(tinfo)) == -1
    assert L.esvio_fe_slice_events_at(None, 0, None, 0, FE.HOST, None, 0, C.byref(cuts), 4, C.byref(sinfo)) == -1
    info = FE.RawInfo()
    assert L.esvio_fe_decode_raw(None, 0, FE.RAW_EVT21, None, 0, FE.HOST, 0, None, 0, FE.HOST, C.byref(info)) == -1
    assert FE.RAW_EVT21 == 21 and FE.raw_bound(FE.RAW_EVT21, 4096) == 16384 and FE.RAW_WORD_BYTES[FE.RAW_EVT21] == 8
    assert FE.TRIGGER_DTYPE.itemsize == C.sizeof(FE.Trigger) == 16
    assert [FE.TRIGGER_DTYPE.fields[n][1] for n in ("sec", "nsec", "id", "value", "_pad")] == [0, 4, 8, 9, 10]
    # the two stage kernels of the trigger chain are listed behind every earlier stage's, the track table is as it was
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(L.esvio_fe_stage_kernel_count())]
    assert names[-2:] == ["k_trig_reduce", "k_trig_emit"] and names[-3] == "k_hot_pick"
    assert "k_trig_reduce" not in names[:L.esvio_fe_kernel_count()]


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {"]
    want = []
    for name, (mirror, members) in STRUCTS.items():
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        assert [m for m, _ in mirror._fields_] == members
        want += [C.sizeof(mirror)] + [getattr(mirror, m).offset for m in members]
    lines += ['  printf("%d\\n", ESVIO_FE_RAW_EVT21);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want + [FE.RAW_EVT21]
    assert C.sizeof(FE.Trigger) == 16 and C.sizeof(FE.TriggerInfo) == 48 and C.sizeof(FE.RawHeaderInfo) == 24


# ---- esvio_fe_raw_header ------------------------------------------------------------------------------------------------
def hdr(data):
    i = FE.raw_header(data)
    return (int(i.payload_offset), i.format, i.width, i.height, i.complete)


PAYLOAD = bytes([0x01, 0x80, 0x25, 0x25, 0x0a, 0x00])  # (holds '%' and '\n' bytes: they are payload)


def test_both_spellings_of_the_format_and_the_geometry():
    old = b"% date 2021-03-02 11:20:01\n% evt 3.0\n% geometry 1280x720\n% serial_number 00001\n"
    assert hdr(old + PAYLOAD) == (len(old), FE.RAW_EVT3, 1280, 720, 1)
    for text, fmt in ((b"2.0", FE.RAW_EVT2), (b"2.1", FE.RAW_EVT21), (b"3.0", FE.RAW_EVT3), (b"4.0", 0)):
        h = b"% evt " + text + b"\n"
        assert hdr(h + PAYLOAD) == (len(h), fmt, 0, 0, 1)
    new = b"% camera_integrator_name Prophesee\n% format EVT21;height=720;width=1280\n% generation 4.2\n% end\n"
    assert hdr(new + PAYLOAD) == (len(new), FE.RAW_EVT21, 1280, 720, 1)
    for text, fmt in ((b"EVT2", FE.RAW_EVT2), (b"EVT21", FE.RAW_EVT21), (b"EVT3", FE.RAW_EVT3), (b"EVT4", 0), (b"EVT", 0)):
        h = b"% format " + text + b"\n% end\n"
        assert hdr(h + PAYLOAD) == (len(h), fmt, 0, 0, 1), text
    # `% format` wins over `% evt` wherever the two stand; a format line without geometry leaves `% geometry`'s
    for h in (b"% evt 3.0\n% format EVT2\n% geometry 640x480\n", b"% format EVT2\n% geometry 640x480\n% evt 3.0\n"):
        assert hdr(h + PAYLOAD) == (len(h), FE.RAW_EVT2, 640, 480, 1)
    # blanks behind '%', a carriage return in front of the newline, keys that only begin like a known one
    h = b"%evt 2.1\r\n%   geometry 346x260\r\n% evtx 3.0\n% formatter EVT3\n% geometry_note 1x1\n"
    assert hdr(h + PAYLOAD) == (len(h), FE.RAW_EVT21, 346, 260, 1)
    # values that are no numbers are not taken
    h = b"% geometry 12x\n% geometry x7\n% geometry -3x4\n% format EVT3;width=abc;height=\n"
    assert hdr(h + PAYLOAD) == (len(h), FE.RAW_EVT3, 0, 0, 1)


def test_end_line_and_payload_that_begins_with_a_percent_sign():
    h = b"% evt 2.1\n% end\n"
    tail = b"%\x00\x11\x22\n% evt 3.0\n"  # payload: behind `% end` nothing is header, whatever it looks like
    assert hdr(h + tail) == (len(h), FE.RAW_EVT21, 0, 0, 1)
    assert hdr(h) == (len(h), FE.RAW_EVT21, 0, 0, 1)  # (`% end` is the end even when nothing follows)
    # without `% end` such bytes would be read as a header line: that is what the line is for
    assert hdr(b"% evt 2.1\n" + tail + PAYLOAD) == (len(b"% evt 2.1\n" + tail), FE.RAW_EVT3, 0, 0, 1)


def test_no_header_at_all_and_empty_input():
    assert hdr(PAYLOAD) == (0, 0, 0, 0, 1)
    assert hdr(b"\n% evt 3.0\n") == (0, 0, 0, 0, 1)
    assert hdr(b"") == (0, 0, 0, 0, 0)
    L = FE.load_library()
    info = FE.RawHeaderInfo()
    assert L.esvio_fe_raw_header(None, 4, C.byref(info)) == -1 and L.esvio_fe_raw_header(b"% e", 3, None) == -1
    assert L.esvio_fe_raw_header(None, 0, C.byref(info)) == 0 and info.complete == 0


def test_a_header_cut_anywhere_is_incomplete_until_its_end_is_inside():
    h = b"% evt 3.0\n% geometry 1280x720\n% end\n"
    whole = h + PAYLOAD
    first, second = len(b"% evt 3.0\n"), len(b"% evt 3.0\n% geometry 1280x720\n")
    for n in range(len(whole) + 1):
        off, fmt, w, ht, complete = hdr(whole[:n])
        assert complete == (1 if n >= len(h) else 0), n
        # only whole lines were read; payload_offset is where the next line starts or started
        assert off == (len(h) if n >= len(h) else second if n >= second else first if n >= first else 0), n
        assert fmt == (FE.RAW_EVT3 if n >= first else 0) and (w, ht) == ((1280, 720) if n >= second else (0, 0)), n
    # without `% end` the header's end is the first byte of another kind: directly behind a whole line it is not known yet
    h = b"% evt 2.0\n% geometry 640x480\n"
    assert hdr(h) == (len(h), FE.RAW_EVT2, 640, 480, 0)
    assert hdr(h + PAYLOAD[:1]) == (len(h), FE.RAW_EVT2, 640, 480, 1)
    # the bytes need not be a bytes object: a numpy view of a file's first block
    blk = np.frombuffer(h + PAYLOAD, np.uint8)
    assert hdr(blk) == (len(h), FE.RAW_EVT2, 640, 480, 1)
    with pytest.raises(TypeError):
        FE.raw_header(None)
