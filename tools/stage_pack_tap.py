#!/usr/bin/env python3
"""The staging packer alone, one thread, no device: esvio_fe_host_stage_pack per 64 KiB chunk over 120 different 2.67 MB
event arrays (nothing cached), each chunk into its own place of a destination buffer, as the staging threads call it.
Prints ns per chunk: packable chunks, then refused chunks (the second half of every array one second earlier: the chunk
holding the step is refused) together with the raw copy that follows a refusal.
    python tools/stage_pack_tap.py            (ESVIO_FE_LIB=<other build> for an A/B, one process each, in turns)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import EVENT_DTYPE  # noqa: E402

L = FE.load_library(build_if_missing=False)
L.esvio_fe_host_stage_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
L.esvio_fe_host_stage_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
N_ARR, EV, CH = 120, 166912, 4096  # 2.67 MB of 16-byte records, 64 KiB chunks
rng = np.random.default_rng(5)
arrs = []
for a in range(N_ARR):
    ev = np.zeros(EV, EVENT_DTYPE)
    ev["x"], ev["y"] = rng.integers(0, 640, EV), rng.integers(0, 480, EV)
    ev["sec"], ev["nsec"] = 1700000000 + a, np.sort(rng.integers(0, 33_000_000, EV))
    ev["polarity"] = rng.integers(0, 2, EV)
    arrs.append(ev)
dst = np.zeros(EV * 16 + 64, np.uint8)
d0 = dst.ctypes.data + (-dst.ctypes.data) % 16
base = C.c_uint32(0)
lib = os.environ.get("ESVIO_FE_LIB", "in-tree")


def run(label, expect_refusals):
    ts, refused = [], 0
    for ev in arrs:
        p = ev.ctypes.data
        for o in range(0, EV * 16, CH * 16):
            n = min(CH * 16, EV * 16 - o)
            t0 = time.perf_counter_ns()
            rc = L.esvio_fe_host_stage_pack(d0 + o, p + o, n, C.byref(base))
            if rc == 0:
                L.esvio_fe_host_stage_copy(d0 + o, p + o, n)
            t1 = time.perf_counter_ns()
            if n == CH * 16 and (rc == 0) == expect_refusals:
                ts.append(t1 - t0)
            refused += rc == 0
    print("%s %s: %d chunks, mean %.0f ns, median %.0f ns, p90 %.0f ns per 64 KiB chunk (%d refused in the pass)" % (
        lib, label, len(ts), statistics.mean(ts), statistics.median(ts), sorted(ts)[len(ts) * 9 // 10], refused), flush=True)


run("packable", False)
for ev in arrs:
    ev["sec"][EV // 2:] -= 1
run("refused+raw", True)
