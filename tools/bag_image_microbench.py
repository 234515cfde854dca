"""esvio_fe_decode_bag_images micro-benchmark.  One stereo frame pair per call at two shapes: 346x260 mono8 (DAVIS) and
1440x1080 rgb8 (DSEC), as a rosbag — a left and a right sensor_msgs/Image message in one chunk, rows padded by 4 bytes
(tests/bag_image_ref.py's writer).  Per shape: the host walks alone (esvio_fe_bag_image_walk_tap, which runs the counting
walk and then the gathering one as the call does; without room for the payloads both passes only count, so the counting
walk is half of that call and the gathering walk is the full call less that half); the copy of the gathered bytes from
pinned memory (esvio_fe_mem_upload, with its wait); k_image_emit from the LIBRARY'S OWN TIMERS
(esvio_fe_get_kernel_stats: HIP events around the launch), its bytes — read and written
— as a share of the measured copy rate; the whole call's wall time from pageable memory into device memory.  Beside it
the bridge the call replaces: tools/bag_image_seq_decode.cpp on one core, then esvio_fe_mem_upload of its gray images.
Per figure: the median of BLOCKS blocks of REPS after a warm-up block, and the blocks' min - max.  One process, one pass,
no retries; run it under a time limit:

    g++ -O2 -std=c++17 -Iesvio_amd/csrc tools/bag_image_seq_decode.cpp -o tools/_bin/bag_image_seq_decode
    timeout -k 10 600 python tools/bag_image_microbench.py > profiles/bag_image_microbench.txt
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

import bag_image_ref as I  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (KERNELS.md)
BLOCKS, REPS = 5, 20
SHAPES = (("DAVIS", 346, 260, 1, "mono8"), ("DSEC", 1440, 1080, 3, "rgb8"))
SEQ = os.path.join(ROOT, "tools", "_bin", "bag_image_seq_decode")


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def pair_bag(W, H, cls, name):
    step = W * I.BPP[cls] + 4
    msgs = [(topic, (7, 1000), I.image_message(1, (7, 1000), H, W, name, step, I.rows(I.test_image(H, W, cls, seed), step)))
            for topic, seed in ((I.LEFT_IMAGE, 1), (I.RIGHT_IMAGE, 2))]
    return I.write_bag(msgs, per_chunk=2)[13:]


def emit_stats(ft):
    L = ft._hd.L
    for k in range(L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()):
        if L.esvio_fe_kernel_name(k).decode() == "k_image_emit":
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            ft._hd.check(L.esvio_fe_get_kernel_stats(ft._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
            return ms.value, n.value
    raise KeyError("k_image_emit")


def main():
    L = FE.load_library()
    hip = C.CDLL("libamdhip64.so")
    for tag, W, H, cls, name in SHAPES:
        data = pair_bag(W, H, cls, name)
        buf = np.frombuffer(data, np.uint8)
        want = I.decode(I.B.MAGIC + data, size=(W, H))["images"]
        wh, bpp = W * H, I.BPP[cls]
        pix_bytes = 2 * (((W * bpp + 4) * H + 15) & ~15)
        print("%s %dx%d %s: a stereo pair, %d bytes of bag (%d of them pixel payload, %d bytes of gray out)" % (tag, W, H, name, len(data), pix_bytes, 2 * wh))
        # the host walks alone, as the call runs them
        stt, cnt = np.zeros(L.esvio_fe_bag_walk_state_bytes(), np.uint8), np.zeros(12, np.uint64)
        pix, rows, carry = np.zeros(pix_bytes, np.uint8), np.zeros(2, FE.BAG_IMAGE_DTYPE), np.zeros(16, np.uint8)
        walk_us = []
        for _ in range(BLOCKS + 1):
            lap = []
            for out in ((None, 0, None, 0), (FE._p(pix), pix_bytes, FE._p(rows), 2)):
                t0 = time.perf_counter()
                for _ in range(REPS):
                    stt[:] = 0
                    assert L.esvio_fe_bag_image_walk_tap(FE._p(stt), len(stt), I.LEFT_IMAGE.encode(), I.RIGHT_IMAGE.encode(), W, H, FE._p(buf), len(buf),
                                                         FE._p(carry), len(carry), *out, FE._p(cnt), None, 0) == 0
                lap.append((time.perf_counter() - t0) / REPS * 1e6)
            assert int(cnt[0]) == 2 and int(cnt[3]) == pix_bytes
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
        ddst = [C.c_void_p(), C.c_void_p()]
        for cam in range(2):
            assert L.esvio_fe_mem_alloc(FE.DEVICE, wh, C.byref(ddst[cam])) == 0
        dptr, caps = (C.c_void_p * 2)(ddst[0].value, ddst[1].value), (C.c_size_t * 2)(1, 1)
        msgs, info = np.zeros(2, FE.BAG_IMAGE_DTYPE), FE.BagImageInfo()
        ft = FE.FeatureTracker(FE.make_config(W, H))
        ft.bag_set_image_topics(*I.IMAGE_TOPICS)

        def call():
            assert L.esvio_fe_decode_bag_images(ft._hd.h, FE._p(buf), len(buf), 0, C.byref(dptr), C.byref(caps), FE.DEVICE, FE._p(msgs), 2, C.byref(info)) == 0

        for _ in range(REPS):
            call()
        assert (info.cam[0].images, info.cam[1].images) == (1, 1)
        for cam in range(2):
            back = np.zeros(wh, np.uint8)
            assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst[cam], C.c_size_t(wh), 2) == 0
            assert back.tobytes() == want[cam][0].tobytes()
        emit_us = []
        for _ in range(BLOCKS):
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            for _ in range(REPS):
                call()
            ms, launches = emit_stats(ft)
            ft.set_profiling(False)
            assert launches == REPS  # one launch per call
            emit_us.append(ms / max(launches, 1) * 1e3)
        plain = []  # the call's wall time without the timers' events
        for _ in range(BLOCKS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            plain.append((time.perf_counter() - t0) / REPS * 1e6)
        e, c = med(emit_us), med(plain)
        gbs = 2 * wh * (bpp + 1) / (e[0] * 1e-6) / 1e9  # the pixels' bytes in, a byte per pixel out
        print("    k_image_emit %7.1f us (%.1f - %.1f; %5.0f GB/s = %4.1f %% of the copy rate) | call %8.1f us (%.1f - %.1f) = %6.1f frame pairs/s"
              % (e[0], e[1], e[2], gbs, 100 * gbs / HBM_GBS, c[0], c[1], c[2], 1e6 / c[0]))
        ft.close()
        if os.path.exists(SEQ):  # the bridge: one core walks and converts, then the gray images are uploaded
            with tempfile.NamedTemporaryFile(suffix=".bagbytes") as f:
                f.write(data)
                f.flush()
                line = subprocess.check_output([SEQ, f.name, I.LEFT_IMAGE, I.RIGHT_IMAGE, "6"]).decode().split()
            seq = dict(zip(line[::2], line[1::2]))
            assert [int(seq["left"]), int(seq["right"])] == [1, 1]
            up = []
            for _ in range(BLOCKS + 1):
                t1 = time.perf_counter()
                for cam in range(2):
                    g = want[cam][0]
                    assert L.esvio_fe_mem_upload(ddst[cam], C.c_void_p(g.ctypes.data), g.nbytes) == 0
                up.append((time.perf_counter() - t1) * 1e6)
            u = med(up[1:])
            total = float(seq["us_median"]) + u[0]
            print("    the bridge: walk and per-pixel conversion on one core %.0f us (%s - %s) + esvio_fe_mem_upload of both gray images %.0f us (%.0f - %.0f) = %.0f us"
                  % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], total))
            print("    the bridge / the call: %.2f" % (total / c[0]))
        for cam in range(2):
            L.esvio_fe_mem_free(FE.DEVICE, ddst[cam])


if __name__ == "__main__":
    main()
