"""CPU: the boundary of the keyframe entry points (esvio_fe_kf_*) that needs no device: the library exports them and the
lists name them, a null handle is refused before anything else, the output struct is laid out by the C compiler as its
ctypes mirror says, the kernel tables that tests and recorded launch traces pin return what they returned, and the
stage's own table lists its three kernels."""
import ctypes as C
import os
import subprocess

import numpy as np

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("esvio_fe_kf_set_pattern", "esvio_fe_kf_blur", "esvio_fe_kf_fast", "esvio_fe_kf_brief", "esvio_fe_kf_match",
                "esvio_fe_kf_describe")
TAPS = ("esvio_fe_kf_kernel_count", "esvio_fe_kf_kernel_name", "esvio_fe_kf_kernel_stats", "esvio_fe_kf_blur_tile")
KF_OUT = ["window_desc", "kp_xy", "kp_score", "kp_norm", "kp_desc", "kp_capacity", "n_kp", "n_detected", "desc_space"]
# the tables as they stood before the stage existed: the track kernels, the stages', the ingest range's last names
TRACK_KERNELS, STAGE_KERNELS, INGEST_KERNELS = 29, 48, 53
INGEST_NAMES = ["k_aedat_count", "k_aedat_scan", "k_aedat_emit", "k_bag_emit", "k_image_emit"]


def test_entry_points_are_exported_and_listed():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS, name
    for name in TAPS:
        assert hasattr(L, name) and name in FE.TEST_SYMBOLS, name
    hdr = open(os.path.join(ROOT, "include", "esvio_fe.h")).read()
    tst = open(os.path.join(ROOT, "include", "esvio_fe_test.h")).read()
    assert all("int %s(" % n in hdr for n in ENTRY_POINTS) and all("%s(" % n in tst for n in TAPS)
    assert "#define ESVIO_FE_KF_BEST_INIT 128" in hdr and "#define ESVIO_FE_KF_MATCH_DIST 80" in hdr
    assert (FE.KF_BEST_INIT, FE.KF_MATCH_DIST) == (128, 80)


def test_a_null_handle_is_refused_before_the_device():
    L = FE.load_library()
    px, w = np.zeros(64, np.uint8), np.zeros(8, np.uint32)
    pat = np.zeros(256, np.int32)
    n, out = C.c_int32(7), FE.KfOut()
    p = FE._p
    assert L.esvio_fe_kf_set_pattern(None, p(pat), p(pat), p(pat), p(pat), 256) == -1
    assert L.esvio_fe_kf_blur(None, p(px), FE.HOST, p(px), FE.HOST) == -1
    assert L.esvio_fe_kf_fast(None, p(px), FE.HOST, 20, None, None, 0, C.byref(n), None) == -1
    assert L.esvio_fe_kf_brief(None, p(px), FE.HOST, None, 0, None, FE.HOST) == -1
    assert L.esvio_fe_kf_match(None, p(w), 1, p(w), 1, FE.HOST, p(w), p(w), p(px)) == -1
    assert L.esvio_fe_kf_describe(None, 0, p(px), FE.HOST, None, 0, 20, C.byref(out)) == -1
    assert L.esvio_fe_kf_kernel_stats(None, 0, None, None, None) == -1
    assert L.esvio_fe_kf_blur_tile(None, None) == -1


def test_the_output_struct_is_laid_out_as_the_c_compiler_lays_it_out(tmp_path):
    assert [m for m, _ in FE.KfOut._fields_] == KF_OUT
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', "int main(void) {",
             '  printf("%zu ", sizeof(esvio_fe_kf_out));']
    lines += ['  printf("%%zu ", offsetof(esvio_fe_kf_out, %s));' % m for m in KF_OUT]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [C.sizeof(FE.KfOut)] + [getattr(FE.KfOut, m).offset for m in KF_OUT]
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert C.sizeof(FE.KfOut) == 56


def test_the_existing_kernel_tables_are_as_they_were():
    L = FE.load_library()
    assert (L.esvio_fe_kernel_count(), L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()) == (TRACK_KERNELS, STAGE_KERNELS, INGEST_KERNELS)
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(INGEST_KERNELS)]
    assert names[0] == "k_tile_hist" and names[TRACK_KERNELS - 1] == "k_events_from_fields" and names[TRACK_KERNELS] == "k_baf_heads"
    assert names[STAGE_KERNELS - 1] == "k_trig_emit" and names[STAGE_KERNELS:] == INGEST_NAMES
    assert len(set(names)) == INGEST_KERNELS and not any(n.startswith("k_kf_") for n in names)
    for k in (INGEST_KERNELS, INGEST_KERNELS + 1, INGEST_KERNELS + 2, INGEST_KERNELS + 5, -1):
        assert L.esvio_fe_kernel_name(k) == b""


def test_the_stage_has_a_table_of_its_own():
    L = FE.load_library()
    assert L.esvio_fe_kf_kernel_count() == 3
    assert [L.esvio_fe_kf_kernel_name(k) for k in range(-1, 4)] == [b"", b"k_kf_blur", b"k_kf_brief", b"k_kf_match", b""]
    tw, th = C.c_int32(0), C.c_int32(0)
    assert L.esvio_fe_kf_blur_tile(C.byref(tw), C.byref(th)) == 0
    assert tw.value >= 4 and tw.value % 4 == 0 and th.value >= 1
