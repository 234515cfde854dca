"""The layout of the blocks the LK kernels read and write in place — the result block (d_res, h_pin) and the two
speculative / chained blocks of h_spec — lives in esvio_amd/csrc/fe_layout.h alone.  tests/layout_check.cpp is built
against that header only (no HIP, no library source) and checks, for max_cnt values around the 64-byte status
padding and the 256-byte block padding: every region inside its block, no two regions overlapping (the two copies
of set 1 apart, the mask area behind the padded layout), float2 regions 8-byte and counters / flags 4-byte aligned,
block sizes equal to what esvio_fe_create allocates.  And no other source file does that arithmetic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "esvio_amd", "csrc")
MAX_CNTS = (0, 1, 63, 64, 65, 120, 1000, 1017)


def test_result_and_speculative_block_layouts(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "layout_check")
    p = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "layout_check.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe] + [str(m) for m in MAX_CNTS], capture_output=True, text=True, timeout=30)
    assert p.returncode == 0 and p.stdout.strip() == "layout ok: %d sizes" % len(MAX_CNTS), p.stdout[-3000:] + p.stderr[-1000:]


def test_layout_header_stands_alone_and_owns_the_offsets():
    hdr = open(os.path.join(CSRC, "fe_layout.h")).read()
    assert set(re.findall(r"#include\s+([<\"][^>\"]+[>\"])", hdr)) == {"<cstddef>", "<cstdint>"}
    api = open(os.path.join(CSRC, "fe_api.cpp")).read()
    # what create allocates, and what create and reset clear
    assert "h_pin.alloc(c, pin_bytes(" in api and "d_res.alloc(c, res_layout(" in api
    assert api.count("kSpecBlocks * spec_layout(") == 2
    for name in sorted(os.listdir(CSRC)):
        if name == "fe_layout.h" or not name.endswith((".cpp", ".h")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for expr in (r"\* 16 \+ 2 \*", r"\bstM\b", r"\bspec_bytes\b"):
            assert not re.search(expr, text), "%s computes an offset of its own: %s" % (name, expr)


def test_partition_scratch_layouts_live_in_fe_kernels_h():
    """the word offsets into the tiled partition's scratch (d_tile) and the radix sort's (hist) are computed by
    tile_scratch / sort_scratch in fe_kernels.h — pinned there by static_asserts — and by no source file"""
    hdr = open(os.path.join(CSRC, "fe_kernels.h")).read()
    for pinned in ("kTileOffTileOff == 2048", "kTileOffOrder == 4128", "kTileOffMeta == 6176", "kTileOffRanges == 6208",
                   "kTileOffP == 8256", "kSortHeadWords == 1088"):
        assert pinned in hdr, pinned
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".cpp"):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for expr in (r"kTileMaxBins", r"kTileOff", r"kRadixMaxPasses\s*<<", r"kSortTickets", r"->(hist|d_tile)(\.p)?\s*\+"):
            assert not re.search(expr, text), "%s computes a scratch offset of its own: %s" % (name, expr)
