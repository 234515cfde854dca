"""esvio_fe_decode_bag micro-benchmark.  The bench's scene stream at C1 (346x260, 1 Mev/s) and at C3's batch size
(640x480, 5 Mev/s): one 30 Hz frame of both cameras as a rosbag — a left and a right dvs_msgs/EventArray message,
sensor_msgs/Imu at 1 kHz and one image-like message of W x H bytes on a foreign topic, three messages per chunk
(tests/bag_ref.py's writer).  Per batch: the host walks alone (esvio_fe_bag_walk_tap: the counting walk, then the
gathering one — what the call runs before any device work); the copy of the gathered bytes from pinned memory
(esvio_fe_mem_upload, with its wait); k_bag_emit from the LIBRARY'S OWN TIMERS (esvio_fe_get_kernel_stats: HIP events
around the launch), its bytes as a share of the measured copy rate; the whole call's wall time from pageable memory into device memory.  Beside it the bridge the call replaces:
tools/bag_seq_decode.cpp on one core, then esvio_fe_mem_upload of its records.  Per figure: the median of BLOCKS blocks
of REPS after a warm-up block, and the blocks' min - max.  One process, one pass, no retries; run it under a time limit:

    g++ -O2 -std=c++17 -Iesvio_amd/csrc tools/bag_seq_decode.cpp -o tools/_bin/bag_seq_decode
    timeout -k 10 600 python tools/bag_microbench.py [--json out.json]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bag_ref as B  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (KERNELS.md)
BLOCKS, REPS = 5, 20
SHAPES = (("C1", 346, 260, 1e6), ("C3", 640, 480, 5e6))
SEQ = os.path.join(ROOT, "tools", "_bin", "bag_seq_decode")


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def frame_bag(left, right, W, H):
    rng = np.random.default_rng(1)
    t0 = int(left["sec"][0]) * 10 ** 9 + int(left["nsec"][0])
    t1 = int(left["sec"][-1]) * 10 ** 9 + int(left["nsec"][-1])
    stamp = (t1 // 10 ** 9, t1 % 10 ** 9)
    msgs = []
    for topic, ev in ((B.LEFT, left), (B.RIGHT, right)):
        msgs.append((topic, stamp, B.event_array(1, stamp, B.wire_events(ev["x"], ev["y"], ev["sec"], ev["nsec"], ev["polarity"]), height=H, width=W)))
    imu = [(B.IMU, (t // 10 ** 9, t % 10 ** 9), B.imu_message(k, (t // 10 ** 9, t % 10 ** 9), rng.normal(0, 1, 3), rng.normal(0, 9, 3)))
           for k, t in enumerate(range(t0, t1, 10 ** 6))]
    image = ("/davis/left/image_raw", stamp, B.ros_header(1, stamp, b"cam") + bytes(W * H))
    return B.write_bag(imu[:len(imu) // 2] + [image, msgs[0]] + imu[len(imu) // 2:] + [msgs[1]], per_chunk=3)[13:]


def emit_stats(ft):
    L = ft._hd.L
    for k in range(L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()):
        if L.esvio_fe_kernel_name(k).decode() == "k_bag_emit":
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            ft._hd.check(L.esvio_fe_get_kernel_stats(ft._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
            return ms.value, n.value
    raise KeyError("k_bag_emit")


def main():
    L = FE.load_library()
    hip = C.CDLL("libamdhip64.so")
    rows = []
    for tag, W, H, rate in SHAPES:
        st = SceneStream(W=W, H=H, rate=rate, seed=3)
        left, right, _ = st.next_batch()
        n = [len(left), len(right)]
        data = frame_bag(left, right, W, H)
        buf = np.frombuffer(data, np.uint8)
        print("%s %dx%d: %d + %d events, %d bytes of bag (%d of them wire events)" % (tag, W, H, n[0], n[1], len(data), 13 * sum(n)))
        # the host walks alone, as the call runs them
        topics = FE._bag_topics(*B.TOPICS)
        stt, cnt = np.zeros(L.esvio_fe_bag_walk_state_bytes(), np.uint8), np.zeros(12, np.uint64)
        pay = [np.zeros(13 * n[0], np.uint8), np.zeros(13 * n[1], np.uint8)]
        ptrs, caps = (C.c_void_p * 2)(pay[0].ctypes.data, pay[1].ctypes.data), (C.c_size_t * 2)(*n)
        walk_us = []
        for _ in range(BLOCKS + 1):
            lap = []
            for out in ((None, None), (C.byref(ptrs), C.byref(caps))):
                t0 = time.perf_counter()
                for _ in range(REPS):
                    stt[:] = 0
                    assert L.esvio_fe_bag_walk_tap(FE._p(stt), len(stt), C.byref(topics), 0, FE._p(buf), len(buf), *out, None, 0, None, 0, FE._p(cnt), None, 0) == 0
                lap.append((time.perf_counter() - t0) / REPS * 1e6)
            assert [int(cnt[0]), int(cnt[1])] == n
            walk_us.append(lap)
        cw, gw = med([w[0] for w in walk_us[1:]]), med([w[1] for w in walk_us[1:]])
        print("    host: counting walk %.1f us (%.1f - %.1f) + gathering walk %.1f us (%.1f - %.1f)" % (cw + gw))
        # the copy of the gathered bytes: pinned -> device, waited for
        nbytes = 13 * sum(n) + 16
        pin, dpk = C.c_void_p(), C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.HOST, nbytes, C.byref(pin)) == 0 and L.esvio_fe_mem_alloc(FE.DEVICE, nbytes, C.byref(dpk)) == 0
        C.memset(pin, 0x5a, nbytes)
        cp = []
        for _ in range(BLOCKS + 1):
            t0 = time.perf_counter()
            for _ in range(REPS):
                assert L.esvio_fe_mem_upload(dpk, pin, nbytes) == 0
            cp.append((time.perf_counter() - t0) / REPS * 1e6)
        cp = med(cp[1:])
        L.esvio_fe_mem_free(FE.HOST, pin)
        L.esvio_fe_mem_free(FE.DEVICE, dpk)
        print("    copy of %d gathered bytes, pinned -> device, with its wait: %.1f us (%.1f - %.1f) = %.1f GB/s" % (nbytes, cp[0], cp[1], cp[2], nbytes / cp[0] / 1e3))
        want = [B.records(pay[0].tobytes()), B.records(pay[1].tobytes())]
        assert want[0].tobytes() == left.tobytes() and want[1].tobytes() == right.tobytes()
        ddst = [C.c_void_p(), C.c_void_p()]
        for cam in range(2):
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n[cam], C.byref(ddst[cam])) == 0
        dptr = (C.c_void_p * 2)(ddst[0].value, ddst[1].value)
        msgs, info = np.zeros(8, FE.BAG_MESSAGE_DTYPE), FE.BagInfo()
        row = dict(batch=tag, n=n, bag_bytes=len(data), count_walk_us=cw, gather_walk_us=gw, copy_us=cp)
        ft = FE.FeatureTracker(FE.make_config(W, H))
        ft.bag_set_topics(*B.TOPICS)

        def call():
            ft.decode_reset()
            assert L.esvio_fe_decode_bag(ft._hd.h, FE._p(buf), len(buf), 0, C.byref(dptr), C.byref(caps), FE.DEVICE, FE._p(msgs), 8, C.byref(info)) == 0

        for _ in range(REPS):
            call()
        assert [info.cam[0].events, info.cam[1].events] == n and info.cam[0].bad == 0
        for cam in range(2):
            back = np.zeros(n[cam], want[cam].dtype)
            assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst[cam], C.c_size_t(16 * n[cam]), 2) == 0
            assert back.tobytes() == want[cam].tobytes()
        emit_us, call_us = [], []
        for _ in range(BLOCKS):
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            call_us.append((time.perf_counter() - t0) / REPS * 1e6)
            ms, launches = emit_stats(ft)
            ft.set_profiling(False)
            emit_us.append(ms / max(launches, 1) * 1e3)
        # the call's wall time without the timers' events
        plain = []
        for _ in range(BLOCKS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            plain.append((time.perf_counter() - t0) / REPS * 1e6)
        e, c = med(emit_us), med(plain)
        gbs = 29 * sum(n) / (e[0] * 1e-6) / 1e9  # 13 bytes in, 16 out
        print("    k_bag_emit %6.1f us (%.1f - %.1f; %5.0f GB/s = %4.1f %% of the copy rate) | call %7.1f us (%.1f - %.1f) = %6.1f Mev/s"
              % (e[0], e[1], e[2], gbs, 100 * gbs / HBM_GBS, c[0], c[1], c[2], sum(n) / c[0]))
        row["k_bag_emit"] = dict(emit_us=e, emit_gbs=gbs, emit_copy_frac=gbs / HBM_GBS, call_us=c, call_us_profiled=med(call_us), mev_s_call=sum(n) / c[0])
        ft.close()
        if os.path.exists(SEQ):  # the bridge: one core walks and deserializes, then the records are uploaded
            with tempfile.NamedTemporaryFile(suffix=".bagbytes") as f:
                f.write(data)
                f.flush()
                line = subprocess.check_output([SEQ, f.name, B.LEFT, B.RIGHT, "6"]).decode().split()
            seq = dict(zip(line[::2], line[1::2]))
            assert [int(seq["left"]), int(seq["right"])] == n and int(seq["bad"]) == 0
            up = []
            for _ in range(BLOCKS + 1):
                t1 = time.perf_counter()
                for cam in range(2):
                    assert L.esvio_fe_mem_upload(ddst[cam], C.c_void_p(want[cam].ctypes.data), want[cam].nbytes) == 0
                up.append((time.perf_counter() - t1) * 1e6)
            u = med(up[1:])
            total = float(seq["us_median"]) + u[0]
            row["bridge"] = dict(decode_us=float(seq["us_median"]), decode_us_min=float(seq["us_min"]), decode_us_max=float(seq["us_max"]), upload_us=u,
                                 total_us=total, mev_s=sum(n) / total)
            print("    the bridge: walk and deserialization on one core %.0f us (%s - %s) + esvio_fe_mem_upload of both cameras' records %.0f us (%.0f - %.0f) = %.0f us = %.1f Mev/s"
                  % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], total, sum(n) / total))
            print("    the bridge / the call: %.2f" % (total / row["k_bag_emit"]["call_us"][0]))
            row["k_bag_emit"]["bridge_over_call"] = total / row["k_bag_emit"]["call_us"][0]
        for cam in range(2):
            L.esvio_fe_mem_free(FE.DEVICE, ddst[cam])
        rows.append(row)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
