"""esvio_fe_decode_text micro-benchmark.  The bench's scene stream, left batch, at C1 (346x260, 1 Mev/s) and at C3's
batch size (640x480, 5 Mev/s), written as text by the cited writers' lines (tests/text_ref.py): {TXYP, SEC_DECIMAL}, the
davis extractor's events.txt, and {XYPT, INT_US}, the dvs extractor's and writer.cpp's.  Per input: each launch of the
chain from the LIBRARY'S OWN TIMERS (esvio_fe_text_kernel_stats: HIP events around the launch); k_text_emit's bytes — the
text read, the records written — as a share of the device copy rate MEASURED IN THE SAME RUN (a device-to-device
hipMemcpy of 256 MiB, read + written bytes over its time); the whole call's wall time from pageable, page-locked and
device memory into device memory.  Beside it the bridge the call replaces: tools/text_seq_decode.cpp on one core, then
esvio_fe_mem_upload of its records.  Per figure: the median of BLOCKS blocks of REPS calls after a warm-up block, and the
blocks' min - max.  One process, one pass, no retries; run it under a time limit:

    python -c "from esvio_amd import build as B; B.build_text_seq()"
    timeout -k 10 600 python tools/text_microbench.py > profiles/text_microbench.txt
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import text_ref as T  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

BLOCKS, REPS = 5, 20
SHAPES = (("C1", 346, 260, 1e6), ("C3", 640, 480, 5e6))
FORMATS = (("TXYP, SEC_DECIMAL", T.TXYP, T.SEC_DECIMAL, T.write_davis), ("XYPT, INT_US", T.XYPT, T.INT_US, T.write_dvs))
SEQ = os.path.join(ROOT, "tools", "_bin", "text_seq_decode")
COPY_BYTES = 256 << 20


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def copy_rate(hip):
    """read + written bytes per second of a device-to-device copy of COPY_BYTES, the best of 5 after a warm-up"""
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(a), C.c_size_t(COPY_BYTES)) == 0 and hip.hipMalloc(C.byref(b), C.c_size_t(COPY_BYTES)) == 0
    assert hip.hipMemset(a, 1, C.c_size_t(COPY_BYTES)) == 0 and hip.hipDeviceSynchronize() == 0
    best = None
    for k in range(6):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(b, a, C.c_size_t(COPY_BYTES), 3) == 0 and hip.hipDeviceSynchronize() == 0
        dt = time.perf_counter() - t0
        if k and (best is None or dt < best):
            best = dt
    hip.hipFree(a)
    hip.hipFree(b)
    return 2 * COPY_BYTES / best / 1e9


def main():
    L = FE.load_library()
    hip = C.CDLL("libamdhip64.so")
    ft = FE.FeatureTracker(FE.make_config(346, 260))
    h = ft._hd.h
    rate = copy_rate(hip)
    print("device copy rate measured in this run: %.0f GB/s (read + written, device-to-device hipMemcpy of %d MiB, best of 5)" % (rate, COPY_BYTES >> 20))
    names = [L.esvio_fe_text_kernel_name(k).decode() for k in range(L.esvio_fe_text_kernel_count())]
    for tag, W, H, ev_rate in SHAPES:
        left = SceneStream(W=W, H=H, rate=ev_rate, seed=7).next_batch()[0]
        tup = list(zip(left["x"].tolist(), left["y"].tolist(), left["sec"].tolist(), left["nsec"].tolist(), (left["polarity"] != 0).astype(int).tolist()))
        for name, order, tkind, write in FORMATS:
            data = write(tup)
            n, nb = len(tup), len(data)
            buf = np.frombuffer(data, np.uint8)
            print("%s, {%s}: %d events, %d bytes of text (%.1f bytes per event), %d bytes of records" % (tag, name, n, nb, nb / n, 16 * n))
            fmt = FE.TextFormat(order, tkind, T.END, 0)
            cap = FE.text_bound(nb)
            ddst, dsrc, psrc = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * cap, C.byref(ddst)) == 0 and L.esvio_fe_mem_alloc(FE.DEVICE, nb, C.byref(dsrc)) == 0
            assert L.esvio_fe_mem_alloc(FE.HOST, nb, C.byref(psrc)) == 0
            assert L.esvio_fe_mem_upload(dsrc, FE._p(buf), nb) == 0
            C.memmove(psrc, FE._p(buf), nb)
            info = FE.TextInfo()
            sources = (("pageable", FE._p(buf), FE.HOST), ("page-locked", psrc, FE.HOST), ("device", dsrc, FE.DEVICE))

            def call(src, space):
                assert L.esvio_fe_decode_text(h, 0, C.byref(fmt), src, nb, space, 0, ddst, cap, FE.DEVICE, C.byref(info)) == 0

            for _, src, space in sources:  # warm-up, and the answer checked once per source
                for _ in range(REPS):
                    call(src, space)
                assert info.events == n and info.lines == n and info.carried == 0
                back = np.zeros(16 * n, np.uint8)
                assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(16 * n), 2) == 0
                assert back.tobytes() == T.records_array(tup).tobytes()
            per = {k: [] for k in names}
            for _ in range(BLOCKS):  # the launches, by the library's timers, from device memory
                ft.set_profiling(True)
                ft.reset_kernel_stats()
                for _ in range(REPS):
                    call(dsrc, FE.DEVICE)
                for k, kn in enumerate(names):
                    ms, launches = C.c_double(0), C.c_uint64(0)
                    ft._hd.check(L.esvio_fe_text_kernel_stats(h, k, C.byref(ms), C.byref(launches), None))
                    assert launches.value == REPS  # one launch of each per call
                    per[kn].append(ms.value / REPS * 1e3)
                ft.set_profiling(False)
            for kn in names:
                m = med(per[kn])
                extra = ""
                if kn == "k_text_emit":
                    gbs = (nb + 16 * n) / (m[0] * 1e-6) / 1e9
                    extra = "; %.0f GB/s of text read and records written = %.1f %% of the copy rate" % (gbs, 100 * gbs / rate)
                if kn == "k_text_count":
                    gbs = nb / (m[0] * 1e-6) / 1e9
                    extra = "; %.0f GB/s of text read = %.1f %% of the copy rate" % (gbs, 100 * gbs / rate)
                print("    %-13s %7.1f us (%.1f - %.1f%s)" % (kn, m[0], m[1], m[2], extra))
            calls = {}
            for sname, src, space in sources:  # the call's wall time without the timers' events
                laps = []
                for _ in range(BLOCKS):
                    t0 = time.perf_counter()
                    for _ in range(REPS):
                        call(src, space)
                    laps.append((time.perf_counter() - t0) / REPS * 1e6)
                calls[sname] = med(laps)
                c = calls[sname]
                print("    call from %-11s memory %8.1f us (%.1f - %.1f) = %6.1f Mev/s, %5.2f GB/s of text" % (sname, c[0], c[1], c[2], n / c[0], nb / c[0] / 1e3))
            if os.path.exists(SEQ):  # the bridge: one core reads the lines, then the records are uploaded
                with tempfile.NamedTemporaryFile(suffix=".txt") as f:
                    f.write(data)
                    f.flush()
                    line = subprocess.check_output([SEQ, f.name, str(order), str(tkind), str(BLOCKS)]).decode().split()
                seq = dict(zip(line[::2], line[1::2]))
                assert int(seq["events"]) == n
                rec = T.records_array(tup)
                up = []
                for _ in range(BLOCKS + 1):
                    t1 = time.perf_counter()
                    assert L.esvio_fe_mem_upload(ddst, FE._p(rec), rec.nbytes) == 0
                    up.append((time.perf_counter() - t1) * 1e6)
                u = med(up[1:])
                total = float(seq["us_median"]) + u[0]
                print("    the bridge: the lines on one core %.0f us (%s - %s) + esvio_fe_mem_upload of the records %.0f us (%.0f - %.0f) = %.0f us"
                      % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], total))
                print("    the bridge / the call from pageable memory: %.1f" % (total / calls["pageable"][0]))
            L.esvio_fe_mem_free(FE.DEVICE, ddst)
            L.esvio_fe_mem_free(FE.DEVICE, dsrc)
            L.esvio_fe_mem_free(FE.HOST, psrc)
    ft.close()


if __name__ == "__main__":
    main()
