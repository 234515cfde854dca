"""esvio_fe_decode_aedat micro-benchmark.  The bench's scene stream, left batch, at C1 (346x260, 1 Mev/s) and at C3's
batch size (640x480, 5 Mev/s), written as libcaer polarity packets of 4096 events with an IMU6 packet per millisecond
(tests/aedat_ref.py's writer).  Per batch: the host walk + gather alone (esvio_fe_aedat_walk_tap: the counting walk, then
the gathering one — what the call runs before any device work); each launch of the chain from the LIBRARY'S OWN TIMERS
(esvio_fe_get_kernel_stats: HIP events around each launch); the whole call's wall time from pageable memory into device
memory, dropping invalid events (three launches) and keeping them (one); the emit's record stores as a share of the
measured copy rate; the run look-up on the batch as it is (one run) and with eventTSOverflow alternating between 3-event
packets (a run per 3 records: the stress case of the table search).  Beside
it the bridge the call replaces: tools/aedat_seq_decode.cpp on one core, then esvio_fe_mem_upload of its records.  Per
figure: the median of BLOCKS blocks after a warm-up block, and the blocks' min - max.  One process, one pass, no retries;
run it under a time limit:

    g++ -O2 -std=c++17 tools/aedat_seq_decode.cpp -o tools/_bin/aedat_seq_decode
    timeout -k 10 600 python tools/aedat_microbench.py [--json out.json]
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

import aedat_ref as A  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import make_events  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (8 TB/s spec)
BLOCKS, REPS = 5, 20
SHAPES = (("C1", 346, 260, 1e6), ("C3", 640, 480, 5e6))
SEQ = os.path.join(ROOT, "tools", "_bin", "aedat_seq_decode")
KERNELS = ("k_aedat_count", "k_aedat_scan", "k_aedat_emit")


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def records(x, y, p, ts):
    r = np.zeros((len(x), 2), "<u4")
    r[:, 0] = 1 | p << 1 | y << 2 | x << 17
    r[:, 1] = ts
    return r.tobytes()


def as_packets(x, y, p, ts, per=4096, imu=True, overflow=lambda k: 0):
    rec, parts = records(x, y, p, ts), []
    rng = np.random.default_rng(1)
    for k, i in enumerate(range(0, len(ts), per)):
        j = min(i + per, len(ts))
        parts.append(A.packet(A.POLARITY, [rec[8 * i:8 * j]], overflow(k), number=j - i))
        if imu:
            for ms in range(int(ts[i]) // 1000, int(ts[j - 1]) // 1000 + 1):
                parts.append(A.packet(A.IMU6, [A.imu6(ms * 1000, rng.normal(0, 1, 3), rng.normal(0, 50, 3))]))
    return b"".join(parts)


def ingest_stats(ft):
    L, out = ft._hd.L, {}
    for k in range(L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count()):
        ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        ft._hd.check(L.esvio_fe_get_kernel_stats(ft._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
        out[L.esvio_fe_kernel_name(k).decode()] = dict(ms=ms.value, launches=n.value)
    return out


def call_bench(L, ft, data, off, flags, ddst, n, want=None):
    buf, info = np.frombuffer(data, np.uint8), FE.AedatInfo()

    def call():
        ft.decode_reset()
        assert L.esvio_fe_decode_aedat(ft._hd.h, 0, FE._p(buf), len(buf), off, flags, ddst, n, FE.DEVICE, C.byref(info)) == 0

    for _ in range(REPS):
        call()
    assert info.events == n and info.bad == 0
    if want is not None:
        back = np.zeros(n, want.dtype)
        assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(16 * n), 2) == 0
        assert back.tobytes() == want.tobytes()
    ks, call_us = {k: [] for k in KERNELS}, []
    for _ in range(BLOCKS):
        ft.set_profiling(True)
        ft.reset_kernel_stats()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        call_us.append((time.perf_counter() - t0) / REPS * 1e6)
        st = ingest_stats(ft)
        ft.set_profiling(False)
        for k in ks:
            ks[k].append(st[k]["ms"] / max(st[k]["launches"], 1) * 1e3 if st[k]["launches"] else 0.0)
    return med(call_us), {k: med(v) for k, v in ks.items()}


def main():
    L = FE.load_library()
    rows = []
    for tag, W, H, rate in SHAPES:
        st = SceneStream(W=W, H=H, rate=rate, seed=3)
        base = st.t_us - 1000
        left, _, _ = st.next_batch()
        x, y, p = (left[k].astype(np.int64) for k in ("x", "y", "polarity"))
        t = left["sec"].astype(np.int64) * 10 ** 6 + left["nsec"].astype(np.int64) // 1000
        rec, n = make_events(x, y, t, p), len(t)
        data = as_packets(x, y, p, t - base)
        runs3 = as_packets(x, y, p, t - base, per=3, imu=False, overflow=lambda k: k & 1)
        print("%s %dx%d: %d events, %d bytes of packets (%.2f B/event)" % (tag, W, H, n, len(data), len(data) / n))
        # the host walk alone: the counting walk and the gathering walk, as the call runs them
        walk_us = []
        buf = np.frombuffer(data, np.uint8)
        stt, runs, pay, cnt = (np.zeros(L.esvio_fe_aedat_walk_state_bytes(), np.uint8), np.zeros((16, 2), np.uint32), np.zeros(8 * n, np.uint8),
                               np.zeros(4, np.uint64))
        for _ in range(BLOCKS + 1):
            lap = []
            for out in ((None, 0, None, 0), (FE._p(runs), 16, FE._p(pay), n)):
                t0 = time.perf_counter()
                for _ in range(REPS):
                    stt[:] = 0
                    assert L.esvio_fe_aedat_walk_tap(FE._p(stt), len(stt), FE._p(buf), len(buf), *out, FE._p(cnt)) == 0
                lap.append((time.perf_counter() - t0) / REPS * 1e6)
            assert int(cnt[0]) == n and pay.tobytes() == records(x, y, p, t - base)
            walk_us.append(lap)
        cw, gw = med([w[0] for w in walk_us[1:]]), med([w[1] for w in walk_us[1:]])
        print("    host: counting walk %.1f us (%.1f - %.1f) + gathering walk %.1f us (%.1f - %.1f)" % (cw + gw))
        ddst = C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(ddst)) == 0
        row = dict(batch=tag, n=n, packet_bytes=len(data), count_walk_us=cw, gather_walk_us=gw)
        ft = FE.FeatureTracker(FE.make_config(W, H))
        for name, src, flags in (("drop invalid", data, 0), ("keep invalid", data, FE.AEDAT_KEEP_INVALID), ("a run per 3 records", runs3, 0)):
            want = rec if name != "a run per 3 records" else None
            c, k = call_bench(L, ft, src, base * 1000 if want is not None else 0, flags, ddst, n, want)
            emit_gbs = 16 * n / (k["k_aedat_emit"][0] * 1e-6) / 1e9
            print("    %-20s count %6.1f us | scan %5.1f us | emit %6.1f us (%.1f - %.1f; the stores %5.0f GB/s = %4.1f %% of the copy rate)"
                  " | call %7.1f us (%.1f - %.1f) = %6.1f Mev/s"
                  % (name, k["k_aedat_count"][0], k["k_aedat_scan"][0], k["k_aedat_emit"][0], k["k_aedat_emit"][1],
                     k["k_aedat_emit"][2], emit_gbs, 100 * emit_gbs / HBM_GBS, c[0], c[1], c[2], n / c[0]))
            row[name] = dict(kernels_us=k, call_us=c, emit_store_gbs=emit_gbs, emit_copy_frac=emit_gbs / HBM_GBS, mev_s_call=n / c[0])
        ft.close()
        if os.path.exists(SEQ):  # the bridge: one core walks and decodes, then the records are uploaded
            with tempfile.NamedTemporaryFile(suffix=".aedat") as f:
                f.write(data)
                f.flush()
                line = subprocess.check_output([SEQ, f.name, str(base * 1000), "6"]).decode().split()
            seq = dict(zip(line[::2], line[1::2]))
            assert int(seq["events"]) == n and int(seq["bad"]) == 0
            up = []
            for _ in range(BLOCKS + 1):
                t1 = time.perf_counter()
                assert L.esvio_fe_mem_upload(ddst, C.c_void_p(rec.ctypes.data), rec.nbytes) == 0
                up.append((time.perf_counter() - t1) * 1e6)
            u = med(up[1:])
            total = float(seq["us_median"]) + u[0]
            print("    the bridge: sequential decoder on one core %.0f us (%s - %s) + esvio_fe_mem_upload of the records %.0f us (%.0f - %.0f) = %.0f us = %.1f Mev/s"
                  % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], total, n / total))
            row["bridge"] = dict(decode_us=float(seq["us_median"]), decode_us_min=float(seq["us_min"]), decode_us_max=float(seq["us_max"]), upload_us=u,
                                 total_us=total, mev_s=n / total)
        L.esvio_fe_mem_free(FE.DEVICE, ddst)
        rows.append(row)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
