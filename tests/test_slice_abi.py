"""CPU: the boundary of the stream-slicing and feed entry points that needs no device — the library exports them, the
structs are laid out by the C compiler as their ctypes mirrors say, a null handle is refused, the tile the GPU tests place
their edges by is a whole number of four-record lanes."""
import ctypes as C
import os
import subprocess

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "esvio_fe_slice_params": (FE.SliceParams, ["frequency", "origin", "has_origin", "reserved"]),
    "esvio_fe_slice_info": (FE.SliceInfo, ["closed", "first_window", "count", "open_events", "first_sec", "first_nsec", "last_sec",
                                           "last_nsec"]),
    "esvio_fe_feed_info": (FE.FeedInfo, ["appended", "rejected", "bad", "closed", "queued"]),
    "esvio_fe_feed_window": (FE.FeedWindow, ["ready", "reserved", "index", "end_sec", "end_nsec", "count"]),
    "esvio_fe_event": (FE.EventRecord, ["x", "y", "sec", "nsec", "polarity", "_pad"]),
}
ENTRY_POINTS = ("esvio_fe_slice_events", "esvio_fe_slice_flush", "esvio_fe_slice_reset", "esvio_fe_feed_open", "esvio_fe_feed_push_events",
                "esvio_fe_feed_push_fields", "esvio_fe_feed_push_raw", "esvio_fe_feed_peek", "esvio_fe_feed_track", "esvio_fe_feed_close")


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    assert "esvio_fe_slice_tile_events" in FE.TEST_SYMBOLS
    prm, info, cuts = FE.SliceParams(30.0), FE.SliceInfo(), (C.c_uint64 * 4)()
    assert L.esvio_fe_slice_events(None, 0, None, 0, FE.HOST, C.byref(prm), C.byref(cuts), 4, C.byref(info)) == -1
    assert L.esvio_fe_slice_flush(None, 0, C.byref(info)) == -1
    assert L.esvio_fe_slice_reset(None) == -1
    finfo, win, tr, binfo = FE.FeedInfo(), FE.FeedWindow(), FE.Tracks(), FE.BatchInfo()
    assert L.esvio_fe_feed_open(None, C.byref(prm), None) == -1
    assert L.esvio_fe_feed_push_events(None, 0, None, 0, FE.HOST, C.byref(finfo)) == -1
    assert L.esvio_fe_feed_push_fields(None, 0, None, 0, FE.HOST, C.byref(finfo)) == -1
    assert L.esvio_fe_feed_push_raw(None, 0, FE.RAW_EVT3, None, 0, FE.HOST, 0, C.byref(finfo)) == -1
    assert L.esvio_fe_feed_peek(None, C.byref(win)) == -1
    assert L.esvio_fe_feed_track(None, 1, None, C.byref(tr), C.byref(binfo)) == -1
    assert L.esvio_fe_feed_close(None) == -1
    tile = L.esvio_fe_slice_tile_events()
    assert tile > 0 and tile % 256 == 0
    assert prm.frequency == 30.0 and prm.has_origin == 0
    prm = FE.SliceParams(1000.0, (10, 500))
    assert (prm.origin.sec, prm.origin.nsec, prm.has_origin, prm.reserved) == (10, 500, 1, 0)


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {"]
    want = []
    for name, (mirror, members) in STRUCTS.items():
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        assert [m for m, _ in mirror._fields_] == members
        want += [C.sizeof(mirror)] + [getattr(mirror, m).offset for m in members]
    lines += ['  printf("%d\\n", ESVIO_FE_SLICE_MAX_WINDOWS);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want + [FE.SLICE_MAX_WINDOWS]
