"""CPU: the boundary of the address-stage and hot-pixel entry points that needs no device — the library exports them,
the binding lists them, a null handle is refused, the three structs are laid out by the C compiler as their ctypes
mirrors say."""
import ctypes as C
import os
import subprocess

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("esvio_fe_set_address_filter", "esvio_fe_set_pixel_mask", "esvio_fe_get_pixel_mask", "esvio_fe_hot_learn",
         "esvio_fe_hot_select", "esvio_fe_hot_reset")
STRUCTS = [("esvio_fe_address_filter", FE.AddressFilter), ("esvio_fe_hot_params", FE.HotParams), ("esvio_fe_hot_info", FE.HotInfo)]


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    a, prm, info, n, bad = FE.AddressFilter(), FE.HotParams(), FE.HotInfo(), C.c_size_t(0), C.c_uint64(0)
    assert L.esvio_fe_set_address_filter(None, 0, C.byref(a)) == -1
    assert L.esvio_fe_set_pixel_mask(None, 0, None, 0) == -1
    assert L.esvio_fe_get_pixel_mask(None, 0, None, 0, C.byref(n)) == -1
    assert L.esvio_fe_hot_learn(None, 0, None, None, 0, FE.HOST, C.byref(bad)) == -1
    assert L.esvio_fe_hot_select(None, 0, C.byref(prm), None, None, 0, C.byref(info)) == -1
    assert L.esvio_fe_hot_reset(None) == -1


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {"]
    want = []
    for cname, mirror in STRUCTS:
        lines.append('  printf("%%zu ", sizeof(%s));' % cname)
        want.append(C.sizeof(mirror))
        for m, _ in mirror._fields_:
            lines.append('  printf("%%zu ", offsetof(%s, %s));' % (cname, m))
            want.append(getattr(mirror, m).offset)
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert got == want
    assert C.sizeof(FE.AddressFilter) == 24 and C.sizeof(FE.HotParams) == 24 and C.sizeof(FE.HotInfo) == 32
