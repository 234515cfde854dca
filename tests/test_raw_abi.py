"""CPU: the boundary of the raw-stream entry points that needs no device — the library exports them, esvio_fe_raw_info is
laid out by the C compiler as its ctypes mirror says, a null handle is refused, the tile the GPU tests place their
edges by is a whole number of words."""
import ctypes as C
import os
import subprocess

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["events", "untimed", "other", "bad", "wraps", "first_t_us", "last_t_us"]


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ("esvio_fe_decode_raw", "esvio_fe_decode_reset", "esvio_fe_track_raw"):
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    info = FE.RawInfo()
    assert L.esvio_fe_decode_raw(None, 0, FE.RAW_EVT3, None, 0, FE.HOST, 0, None, 0, FE.HOST, C.byref(info)) == -1
    assert L.esvio_fe_decode_reset(None) == -1
    tr, binfo, raw = FE.Tracks(), FE.BatchInfo(), (FE.RawInfo * 2)()
    assert L.esvio_fe_track_raw(None, FE.RAW_EVT2, None, 0, None, 0, FE.HOST, 0, 1, None, None, C.byref(tr), C.byref(binfo),
                                C.byref(raw)) == -1
    assert FE.RAW_EVT2 == 2 and FE.RAW_EVT3 == 3
    tile = L.esvio_fe_raw_tile_bytes()
    assert tile > 0 and tile % 16 == 0


def test_raw_info_layout_equals_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {",
             '  printf("%zu", sizeof(esvio_fe_raw_info));']
    lines += ['  printf(" %%zu", offsetof(esvio_fe_raw_info, %s));' % m for m in MEMBERS]
    lines += ['  printf(" %d %d\\n", ESVIO_FE_RAW_EVT2, ESVIO_FE_RAW_EVT3);', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert [m for m, _ in FE.RawInfo._fields_] == MEMBERS
    assert got == [C.sizeof(FE.RawInfo)] + [getattr(FE.RawInfo, m).offset for m in MEMBERS] + [FE.RAW_EVT2, FE.RAW_EVT3]
