"""esvio_fe_decode_aedat_frames micro-benchmark.  DAVIS346 frames, 346x260, with one channel and with three, one frame per
call and eight per call, as libcaer / AEDAT 3.1 packets: a frame packet of one event behind a polarity packet of 4096
events and an IMU6 packet (tests/aedat_frame_ref.py's writer).  Per shape: the host walks alone
(esvio_fe_aedat_frame_walk_tap, which runs the counting walk and then the gathering one as the call does; without room
for the pixels both passes only count, so the counting walk is half of that call and the gathering walk is the full call
less that half); the copy of the gathered bytes from pinned memory (esvio_fe_mem_upload, with its wait); k_frame16_emit
from the LIBRARY'S OWN TIMER (esvio_fe_aedat_frame_kernel_stats: HIP events around the launch), its bytes — read and
written — as a share of the device copy rate MEASURED IN THE SAME RUN (a device-to-device hipMemcpy of 256 MiB, read +
written bytes over its time); the whole call's wall time from pageable memory into device memory.  Beside it the bridge
the call replaces: tools/aedat_frame_seq.cpp on one core — the driver's loop, one push_back(value >> 8) per value — then
esvio_fe_mem_upload of its gray images.  Per figure: the median of BLOCKS blocks of REPS after a warm-up block, and the
blocks' min - max.  One process, one pass, no retries; run it under a time limit:

    python -c "from esvio_amd import build as B; B.build_frame_seq()"
    timeout -k 10 600 python tools/aedat_frame_microbench.py > profiles/aedat_frame_microbench.txt
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

import aedat_frame_ref as F  # noqa: E402
import aedat_ref as A  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402

BLOCKS, REPS = 5, 20
W, H = 346, 260
SHAPES = ((1, 1), (1, 8), (3, 1), (3, 8))  # (channels, frames per call)
SEQ = os.path.join(ROOT, "tools", "_bin", "aedat_frame_seq")
COPY_BYTES = 256 << 20


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def chunk(channels, n, rng):
    parts = []
    for k in range(n):
        rec = np.zeros((4096, 2), "<u4")
        rec[:, 0] = 1 | rng.integers(0, 2, 4096) << 1 | rng.integers(0, H, 4096) << 2 | rng.integers(0, W, 4096) << 17
        rec[:, 1] = 33000 * k + np.sort(rng.integers(0, 33000, 4096))
        parts += [A.packet(A.POLARITY, [rec.tobytes()], number=4096, capacity=4096), A.packet(A.IMU6, [A.imu6(33000 * k, (0, 0, 1), (0, 0, 0))]),
                  F.frame_packet([F.frame_event(F.test_pixels(W, H, channels, 10 * channels + k), W, H, channels,
                                                ts=(33000 * k, 33000 * k + 9000, 33000 * k + 1000, 33000 * k + 8000))])]
    return b"".join(parts)


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
    ft = FE.FeatureTracker(FE.make_config(W, H))
    rate = copy_rate(hip)
    print("device copy rate measured in this run: %.0f GB/s (read + written, device-to-device hipMemcpy of %d MiB, best of 5)" % (rate, COPY_BYTES >> 20))
    rng = np.random.default_rng(5)
    wh = W * H
    for channels, n in SHAPES:
        data = chunk(channels, n, rng)
        buf = np.frombuffer(data, np.uint8)
        want = F.decode(data, size=(W, H))["images"]
        pix_bytes = n * ((wh * channels * 2 + 15) & ~15)
        print("346x260, %d channel%s, %d frame%s per call: %d bytes of packets (%d of them gathered pixel bytes, %d bytes of gray out)"
              % (channels, "" if channels == 1 else "s", n, "" if n == 1 else "s", len(data), pix_bytes, n * wh))
        # the host walks alone, as the call runs them
        stt, cnt = np.zeros(L.esvio_fe_aedat_walk_state_bytes(), np.uint8), np.zeros(8, np.uint64)
        pix, rows, carry = np.zeros(pix_bytes, np.uint8), np.zeros(n, FE.AEDAT_FRAME_DTYPE), np.zeros(16, np.uint8)
        walk_us = []
        for _ in range(BLOCKS + 1):
            lap = []
            for out in ((None, 0, None, 0), (FE._p(pix), pix_bytes, FE._p(rows), n)):
                t0 = time.perf_counter()
                for _ in range(REPS):
                    stt[:] = 0
                    assert L.esvio_fe_aedat_frame_walk_tap(FE._p(stt), len(stt), W, H, FE._p(buf), len(buf), 0, 0, FE._p(carry), len(carry), *out,
                                                           FE._p(cnt), None, 0) == 0
                lap.append((time.perf_counter() - t0) / REPS * 1e6)
            assert int(cnt[0]) == n and int(cnt[1]) == pix_bytes
            walk_us.append(lap)
        both, full = med([w[0] for w in walk_us[1:]]), med([w[1] for w in walk_us[1:]])
        print("    host: two counting passes %.1f us (%.1f - %.1f), so the counting walk ~%.1f us; counting + gathering walk %.1f us (%.1f - %.1f), so the gathering walk ~%.1f us"
              % (both + (both[0] / 2,) + full + (full[0] - both[0] / 2,)))
        # the copy of the gathered bytes: pinned -> device, waited for
        pin, dpk = C.c_void_p(), C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.HOST, pix_bytes, C.byref(pin)) == 0 and L.esvio_fe_mem_alloc(FE.DEVICE, pix_bytes, C.byref(dpk)) == 0
        C.memset(pin, 0x5a, pix_bytes)
        cp = []
        for _ in range(BLOCKS + 1):
            t0 = time.perf_counter()
            for _ in range(REPS):
                assert L.esvio_fe_mem_upload(dpk, pin, pix_bytes) == 0
            cp.append((time.perf_counter() - t0) / REPS * 1e6)
        cp = med(cp[1:])
        L.esvio_fe_mem_free(FE.HOST, pin)
        L.esvio_fe_mem_free(FE.DEVICE, dpk)
        print("    copy of %d gathered bytes, pinned -> device, with its wait: %.1f us (%.1f - %.1f) = %.1f GB/s" % (pix_bytes, cp[0], cp[1], cp[2], pix_bytes / cp[0] / 1e3))
        ddst = C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.DEVICE, n * wh, C.byref(ddst)) == 0
        info = FE.AedatFrameInfo()
        ft.decode_reset()

        def call():
            assert L.esvio_fe_decode_aedat_frames(ft._hd.h, 0, FE._p(buf), len(buf), 0, 0, ddst, n, FE.DEVICE, FE._p(rows), n, C.byref(info)) == 0

        for _ in range(REPS):
            call()
        assert info.frames == n
        back = np.zeros(n * wh, np.uint8)
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(n * wh), 2) == 0
        assert back.tobytes() == b"".join(g.tobytes() for g in want)
        emit_us = []
        for _ in range(BLOCKS):
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            for _ in range(REPS):
                call()
            ms, launches = C.c_double(0), C.c_uint64(0)
            ft._hd.check(L.esvio_fe_aedat_frame_kernel_stats(ft._hd.h, C.byref(ms), C.byref(launches), None))
            ft.set_profiling(False)
            assert launches.value == REPS  # one launch per call
            emit_us.append(ms.value / REPS * 1e3)
        plain = []  # the call's wall time without the timers' events
        for _ in range(BLOCKS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            plain.append((time.perf_counter() - t0) / REPS * 1e6)
        e, c = med(emit_us), med(plain)
        gbs = n * wh * (2 * channels + 1) / (e[0] * 1e-6) / 1e9  # the values' bytes in, a byte per pixel out
        print("    k_frame16_emit %7.1f us (%.1f - %.1f; %5.0f GB/s = %4.1f %% of the copy rate) | call %8.1f us (%.1f - %.1f) = %6.1f frames/s"
              % (e[0], e[1], e[2], gbs, 100 * gbs / rate, c[0], c[1], c[2], n * 1e6 / c[0]))
        if os.path.exists(SEQ):  # the bridge: one core walks and converts, then the gray images are uploaded
            with tempfile.NamedTemporaryFile(suffix=".aedatbytes") as f:
                f.write(data)
                f.flush()
                line = subprocess.check_output([SEQ, f.name, "6"]).decode().split()
            seq = dict(zip(line[::2], line[1::2]))
            assert int(seq["frames"]) == n
            up = []
            for _ in range(BLOCKS + 1):
                t1 = time.perf_counter()
                for k, g in enumerate(want):
                    assert L.esvio_fe_mem_upload(C.c_void_p(ddst.value + k * wh), C.c_void_p(g.ctypes.data), g.nbytes) == 0
                up.append((time.perf_counter() - t1) * 1e6)
            u = med(up[1:])
            total = float(seq["us_median"]) + u[0]
            print("    the bridge: walk and per-value loop on one core %.0f us (%s - %s) + esvio_fe_mem_upload of the gray images %.0f us (%.0f - %.0f) = %.0f us"
                  % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], total))
            print("    the bridge / the call: %.2f" % (total / c[0]))
        L.esvio_fe_mem_free(FE.DEVICE, ddst)
    ft.close()


if __name__ == "__main__":
    main()
