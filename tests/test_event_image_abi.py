"""CPU: the boundary of the event images that needs no device — the library exports the four entry points, the header
declares them with the signatures the issue sets (a C compiler checks that), a null handle is refused before anything
else, and the Python mirrors exist."""
import ctypes as C
import os
import subprocess

import numpy as np

from esvio_amd import frontend as FE
from esvio_amd.node import StereoEventTrackerNode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("esvio_fe_set_event_images", "esvio_fe_clear_event_images", "esvio_fe_get_event_image", "esvio_fe_get_event_canvas")
SIGNATURES = """
#include "esvio_fe.h"
int (*p_set)(esvio_fe_handle, int) = esvio_fe_set_event_images;
int (*p_clear)(esvio_fe_handle) = esvio_fe_clear_event_images;
int (*p_image)(esvio_fe_handle, int, uint8_t*, int) = esvio_fe_get_event_image;
int (*p_canvas)(esvio_fe_handle, uint8_t*, int) = esvio_fe_get_event_canvas;
"""


def test_entry_points_are_exported_and_refuse_a_null_handle_before_the_device():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS, name
    assert "esvio_fe_event_image_kernel_stats" in FE.TEST_SYMBOLS
    px = np.zeros(16, np.uint8)
    assert L.esvio_fe_set_event_images(None, 1) == -1
    assert L.esvio_fe_clear_event_images(None) == -1
    assert L.esvio_fe_get_event_image(None, 0, FE._p(px), FE.HOST) == -1
    assert L.esvio_fe_get_event_canvas(None, FE._p(px), FE.HOST) == -1
    assert L.esvio_fe_event_image_kernel_stats(None, 0, None, None, None) == -1
    assert (px == 0).all()


def test_the_header_declares_them_with_these_signatures(tmp_path):
    src = tmp_path / "sig.c"
    src.write_text(SIGNATURES)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "sig.o")])
    hdr = open(os.path.join(ROOT, "include", "esvio_fe.h")).read()
    for name in ENTRY_POINTS:
        assert hdr.count("int %s(esvio_fe_handle h" % name) == 1, name
    # the rule is the header's: the citations it rests on are there
    for cite in ("feature_tracker.cpp:352-353", "event_detector.cc:145-146", ":1107", "event_detector.cc:128-129", "(255, 0, 0)", "(0, 0, 255)"):
        assert cite in hdr, cite
    # the timer slots of the two kernels are outside the stage and ingest tables: both end where they ended
    L = FE.load_library()
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(L.esvio_fe_ingest_kernel_count() + 2)]
    assert names[-3:] == ["k_image_emit", "", ""] and not [n for n in names if "evimg" in n]


def test_the_frontend_mirrors_exist():
    for name in ("set_event_images", "event_image", "event_canvas", "clear_event_images"):
        assert callable(getattr(FE.FeatureTracker, name)), name
    for name in ("cur_event_mat_left", "cur_event_mat_right"):
        assert isinstance(getattr(FE.EventDetector, name), property), name
    import inspect
    assert inspect.signature(StereoEventTrackerNode.__init__).parameters["show_track"].default is False
    L = FE.load_library()
    assert L.esvio_fe_get_event_image.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert L.esvio_fe_get_event_canvas.argtypes == [C.c_void_p, C.c_void_p, C.c_int]
