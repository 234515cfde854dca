"""esvio_fe_decode_raw / esvio_fe_track_raw micro-benchmark.  The bench's scene stream at C3's batch (640x480, 5 Mev/s:
~167 k events per camera) and C5's (1280x720, 100 Mev/s: ~3.3 M), encoded as EVT3 in read-out order with vector words,
as EVT3 without vector words and as EVT2 (the encoders of tests/evt_ref.py; vectorised forms for the two without
vectors, checked against them).  Per encoding: the realised bytes per event; per launch of the decode chain the time
from the LIBRARY'S OWN TIMERS (esvio_fe_get_kernel_stats: HIP events around each launch — not a rocprofv3 summary), the
bytes read and written and the share of the HBM rate k_raw_emit's record stores amount to; the whole call's wall time
from device memory, page-locked memory read in place, page-locked memory copied first (ESVIO_FE_RAW_PINNED_COPY=1) and
pageable memory, into device memory; for page-locked words also the first 4 .. 512 KiB of C3's stream both ways (where
reading in place stops paying).  Beside it the sequential decoder the call replaces (tools/raw_seq_decode.cpp on
one core, + esvio_fe_mem_upload of its records), and esvio_fe_track_raw from pageable words against esvio_fe_track_event
from pageable records on the same events: plain calls, two handles of one configuration, A/B in one process, ROUNDS
alternations.  Per figure: the median of BLOCKS blocks after a warm-up block, and the blocks' min - max.  Also EVT2.1
(the greedy encoder of tests/evt21_ref.py, and n / 32 words with full masks: 32 records per word), and per encoding
esvio_fe_decode_triggers on the same words in device memory with a frame's two edges appended.  One process,
one pass, no retries; run it under a time limit:

    g++ -O2 -std=c++17 tools/raw_seq_decode.cpp -o tools/_bin/raw_seq_decode
    timeout -k 10 900 python tools/raw_microbench.py [--json out.json] [--only C3] [--formats evt21,evt2] [--device-only]
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

import evt21_ref as E21  # noqa: E402
import evt_ref as R  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import event_times, make_events  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (8 TB/s spec)
BLOCKS, REPS, ROUNDS = 5, 20, 6
SHAPES = (("C3", 640, 480, 5e6, 6), ("C5", 1280, 720, 100e6, 2))  # tag, W, H, rate, frames of the track A/B
SEQ = os.path.join(ROOT, "tools", "_bin", "raw_seq_decode")


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def fields_of(ev):
    t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
    return ev["x"].astype(np.int64), ev["y"].astype(np.int64), ev["polarity"].astype(np.int64), t


def changed(a):
    c = np.ones(len(a), bool)
    c[1:] = a[1:] != a[:-1]
    return c


def encode_evt2_np(x, y, p, t):
    """evt_ref.encode_evt2 without the loop"""
    h = changed(t >> 6)
    pos = np.cumsum(h + 1) - 1  # where each event's CD word goes
    out = np.zeros(int(pos[-1]) + 1, np.int64)
    out[pos] = (p << 28) | ((t & 0x3F) << 22) | (x << 11) | y
    out[pos[h] - 1] = 0x80000000 | (t[h] >> 6)
    return out.astype("<u4")


def encode_evt3_novect_np(x, y, p, t):
    """evt_ref.encode_evt3(vect=False) without the loop: TIME_HIGH, TIME_LOW, ADDR_Y where they change, then ADDR_X"""
    a, b, c = changed(t >> 12), changed(t & 0xFFF), changed(y)
    pos = np.cumsum(a.astype(np.int64) + b + c + 1) - 1
    out = np.zeros(int(pos[-1]) + 1, np.int64)
    out[pos] = 0x2000 | (p << 11) | x
    out[pos[c] - 1] = y[c]
    out[pos[b] - 1 - c[b]] = 0x6000 | (t[b] & 0xFFF)
    out[pos[a] - 1 - c[a] - b[a]] = 0x8000 | (t[a] >> 12)
    return out.astype("<u2")


def encode_evt21_np(x, y, p, t):
    """evt21_ref.encode_evt21 with the loop only inside runs of equal (t, y, p) and increasing x (rare in the scene stream)"""
    n = len(t)
    brk = changed(t) | changed(y) | changed(p)
    brk[1:] |= x[1:] <= x[:-1]
    starts = np.flatnonzero(brk)
    ends = np.append(starts[1:], n)
    word_start = brk.copy()
    for s in np.flatnonzero(ends - starts > 1):
        i = int(starts[s])
        for j in range(i + 1, int(ends[s])):
            if x[j] - x[i] >= 32:
                word_start[j] = True
                i = j
    ws = np.flatnonzero(word_start)
    wid = np.cumsum(word_start) - 1
    mask = np.zeros(len(ws), np.uint64)
    np.bitwise_or.at(mask, wid, np.uint64(1) << (x - x[ws][wid]).astype(np.uint64))
    u = [a[ws].astype(np.uint64) for a in (p, t & 0x3F, x, y)]
    ev = (u[0] << np.uint64(60)) | (u[1] << np.uint64(54)) | (u[2] << np.uint64(43)) | (u[3] << np.uint64(32)) | mask
    h = changed(t[ws] >> 6)
    pos = np.cumsum(h + 1) - 1
    out = np.zeros(int(pos[-1]) + 1, np.uint64)
    out[pos] = ev
    out[pos[h] - 1] = (np.uint64(8) << np.uint64(60)) | ((t[ws][h] >> 6).astype(np.uint64) << np.uint64(32))
    return out.astype("<u8")


FORMATS = None  # --formats evt21,evt2: only these encodings are built and measured (the EVT3 loop encoder takes minutes at C5)
DEVICE_ONLY = False  # --device-only: the per-launch figures from device memory and the trigger call; no host sources, no track A/B


def encodings(ev, base):
    x, y, p, t = fields_of(ev)
    o = R.readout_order(x, y, p, t)
    xr, yr, pr, tr = x[o], y[o], p[o], t[o] - base
    k = min(len(x), 20000)
    assert np.array_equal(encode_evt2_np(xr[:k], yr[:k], pr[:k], tr[:k]), R.encode_evt2(xr[:k], yr[:k], pr[:k], tr[:k]))
    assert np.array_equal(encode_evt3_novect_np(xr[:k], yr[:k], pr[:k], tr[:k]), R.encode_evt3(xr[:k], yr[:k], pr[:k], tr[:k], vect=False))
    assert np.array_equal(encode_evt21_np(xr[:k], yr[:k], pr[:k], tr[:k]), E21.encode_evt21(xr[:k], yr[:k], pr[:k], tr[:k]))
    rec = make_events(xr, yr, tr + base, pr)
    makers = (("EVT3, read-out order, vectors", "evt3", R.EVT3, lambda: R.encode_evt3(xr, yr, pr, tr)),
              ("EVT3, no vectors", "evt3nv", R.EVT3, lambda: encode_evt3_novect_np(xr, yr, pr, tr)),
              ("EVT2", "evt2", R.EVT2, lambda: encode_evt2_np(xr, yr, pr, tr)),
              ("EVT2.1", "evt21", FE.RAW_EVT21, lambda: encode_evt21_np(xr, yr, pr, tr)))
    return rec, tuple((name, fmt, make()) for name, key, fmt, make in makers if FORMATS is None or key in FORMATS)


def dense_evt21(n, W, base):
    """n // 32 EVT2.1 words with full masks behind one TIME_HIGH — 32 records per word, the format's densest — and the
    records they stand for: what the emit launch does when its stores, not its walk, are the work"""
    k = np.arange(n // 32, dtype=np.int64)
    per_row = W // 32
    bx, y = (k % per_row) * 32, (k // per_row) % 2048
    words = np.empty(len(k) + 1, np.uint64)
    words[0] = (np.uint64(8) << np.uint64(60)) | (np.uint64(20) << np.uint64(32))
    words[1:] = (np.uint64(1) << np.uint64(60)) | (np.uint64(5) << np.uint64(54)) | (bx.astype(np.uint64) << np.uint64(43)) | \
        (y.astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    x = (bx[:, None] + np.arange(32)[None, :]).reshape(-1)
    rec = make_events(x, np.repeat(y, 32), np.full(len(x), 20 * 64 + 5 + base, np.int64), np.ones(len(x), np.int64))
    return rec, words.astype("<u8")


def trigger_bench(L, ft, tag, name, fmt, words, base, arena, rows):
    """esvio_fe_decode_triggers on the same words in device memory, with a frame's two edges appended: the call's wall
    time and its launches (the scan is k_raw_scan)"""
    wd = words.dtype
    edge = {R.EVT3: [0xA001, 0xA000], R.EVT2: [0xA0000001, 0xA0000000], FE.RAW_EVT21: [(0xA << 60) | (1 << 32), 0xA << 60]}[fmt]
    w = np.concatenate([words, np.array(edge, np.uint64).astype(wd)])
    nb = w.nbytes
    _, _, dsrc, _ = arena
    assert L.esvio_fe_mem_upload(dsrc, C.c_void_p(w.ctypes.data), nb) == 0
    out, info = (FE.Trigger * 8)(), FE.TriggerInfo()

    def call():
        ft.decode_reset()
        assert L.esvio_fe_decode_triggers(ft._hd.h, 0, fmt, dsrc, nb, FE.DEVICE, base, C.byref(out), 8, C.byref(info)) == 0
    for _ in range(REPS):
        call()
    assert info.triggers == 2 and (out[0].value, out[1].value) == (1, 0)
    ks, call_us = {k: [] for k in ("k_trig_reduce", "k_raw_scan", "k_trig_emit")}, []
    for _ in range(BLOCKS):
        ft.set_profiling(True)
        ft.reset_kernel_stats()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        call_us.append((time.perf_counter() - t0) / REPS * 1e6)
        st = ft.kernel_stats(stages=True)
        ft.set_profiling(False)
        for k in ks:
            assert st[k]["launches"] == REPS
            ks[k].append(st[k]["ms"] / REPS * 1e3)
    c = med(call_us)
    k = {name_: med(v) for name_, v in ks.items()}
    print("    %-18s trig reduce %7.1f us | scan %6.1f us | trig emit %7.1f us | call %8.1f us (%.1f - %.1f), 2 triggers"
          % ("triggers, device", k["k_trig_reduce"][0], k["k_raw_scan"][0], k["k_trig_emit"][0], c[0], c[1], c[2]))
    rows.append(dict(batch=tag, encoding=name, source="device", stage="triggers", word_bytes=nb, kernels_us=k, call_us=c))


def stage_bench(L, ft, ft_copy, tag, rec, name, fmt, words, base, arena, rows):
    n, nb = len(rec), words.nbytes
    pin, pinned, dsrc, ddst = arena
    pinned[:nb] = words.view(np.uint8)
    assert L.esvio_fe_mem_upload(dsrc, C.c_void_p(words.ctypes.data), nb) == 0
    print("%s %-30s %9d events, %9d words: %.2f B/event" % (tag, name, n, len(words), nb / n))
    info = FE.RawInfo()
    for src, tr, ptr, space in (("device", ft, dsrc, FE.DEVICE), ("pinned, in place", ft, pin, FE.HOST),
                                ("pinned, copy first", ft_copy, pin, FE.HOST), ("pageable", ft, C.c_void_p(words.ctypes.data), FE.HOST)):
        if DEVICE_ONLY and src != "device":
            continue

        def call():
            tr.decode_reset()
            assert L.esvio_fe_decode_raw(tr._hd.h, 0, fmt, ptr, nb, space, base, ddst, n, FE.DEVICE, C.byref(info)) == 0

        reps = REPS if n < 1_000_000 or src == "device" else 5
        for _ in range(reps):
            call()
        assert info.events == n and info.untimed == 0 and info.bad == 0
        if src == "device":  # the records, once: byte for byte what make_events builds
            back = np.zeros(n, rec.dtype)
            assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(16 * n), 2) == 0
            assert back.tobytes() == rec.tobytes()
        ks, call_us = {k: [] for k in ("k_raw_reduce", "k_raw_scan", "k_raw_emit")}, []
        for _ in range(BLOCKS):
            tr.set_profiling(True)
            tr.reset_kernel_stats()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            call_us.append((time.perf_counter() - t0) / reps * 1e6)
            st = tr.kernel_stats(stages=True)
            tr.set_profiling(False)
            for k in ks:
                assert st[k]["launches"] == reps
                ks[k].append(st[k]["ms"] / reps * 1e3)
        c = med(call_us)
        k = {name_: med(v) for name_, v in ks.items()}
        tiles = (nb + 4095) // 4096
        emit_gbs = 16 * n / (k["k_raw_emit"][0] * 1e-6) / 1e9
        print("    %-18s reduce %7.1f us (reads %d B) | scan %6.1f us (%d B) | emit %7.1f us (%.1f - %.1f; reads %d B, writes %d B: "
              "the stores %6.0f GB/s = %4.1f %% of HBM) | call %8.1f us (%.1f - %.1f) = %7.1f Mev/s"
              % (src, k["k_raw_reduce"][0], nb, k["k_raw_scan"][0], 64 * tiles, k["k_raw_emit"][0], k["k_raw_emit"][1], k["k_raw_emit"][2],
                 nb + 32 * tiles, 16 * n, emit_gbs, 100 * emit_gbs / HBM_GBS, c[0], c[1], c[2], n / c[0]))
        rows.append(dict(batch=tag, encoding=name, n=n, word_bytes=nb, bytes_per_event=nb / n, source=src, kernels_us=k, call_us=c,
                         emit_store_gbs=emit_gbs, emit_hbm_frac=emit_gbs / HBM_GBS, mev_s_call=n / c[0]))
    trigger_bench(L, ft, tag, name, fmt, words, base, arena, rows)
    if os.path.exists(SEQ) and fmt != FE.RAW_EVT21 and not DEVICE_ONLY:  # the path without the call: one core decodes, then the records are uploaded
        with tempfile.NamedTemporaryFile(suffix=".words") as f:
            f.write(words.tobytes())
            f.flush()
            line = subprocess.check_output([SEQ, str(fmt), f.name, str(base), "6"]).decode().split()
        seq = dict(zip(line[::2], line[1::2]))
        assert int(seq["events"]) == n
        up = []
        for _ in range(BLOCKS):
            t1 = time.perf_counter()
            assert L.esvio_fe_mem_upload(ddst, C.c_void_p(rec.ctypes.data), rec.nbytes) == 0
            up.append((time.perf_counter() - t1) * 1e6)
        u = med(up)
        print("    sequential decoder on one core %.0f us (%s - %s) + esvio_fe_mem_upload of the records %.0f us (%.0f - %.0f) = %.1f Mev/s"
              % (float(seq["us_median"]), seq["us_min"], seq["us_max"], u[0], u[1], u[2], n / (float(seq["us_median"]) + u[0])))
        rows.append(dict(batch=tag, encoding=name, n=n, source="sequential decoder + esvio_fe_mem_upload", decode_us=float(seq["us_median"]),
                         decode_us_min=float(seq["us_min"]), decode_us_max=float(seq["us_max"]), upload_us=u,
                         mev_s_call=n / (float(seq["us_median"]) + u[0])))


def pinned_sweep(L, ft, ft_copy, tag, name, fmt, words, n, base, arena, rows):
    """where reading page-locked words in place stops paying: the first kb KiB of the stream, in place against copied
    first, the whole call's wall time"""
    pin, pinned, _, ddst = arena
    info = FE.RawInfo()
    for kb in (4, 16, 32, 64, 128, 256, 512):
        nb = kb * 1024
        if nb > words.nbytes:
            break
        pinned[:nb] = words.view(np.uint8)[:nb]
        res = {}
        for src, tr in (("in place", ft), ("copy first", ft_copy)):
            def call():
                tr.decode_reset()
                assert L.esvio_fe_decode_raw(tr._hd.h, 0, fmt, pin, nb, FE.HOST, base, ddst, min(nb // 2, n), FE.DEVICE, C.byref(info)) == 0
            for _ in range(REPS):
                call()
            us = []
            for _ in range(BLOCKS):
                t0 = time.perf_counter()
                for _ in range(5 * REPS):
                    call()
                us.append((time.perf_counter() - t0) / (5 * REPS) * 1e6)
            res[src] = med(us)
        print("%s %s pinned %4d KiB: in place %6.1f us (%.1f - %.1f) | copy first %6.1f us (%.1f - %.1f)"
              % ((tag, name, kb) + res["in place"] + res["copy first"]))
        rows.append(dict(batch=tag, encoding=name, sweep="pinned", kib=kb, in_place_us=res["in place"], copy_first_us=res["copy first"]))


def track_ab(tag, W, H, frames, base, rows):
    """esvio_fe_track_raw on pageable words against esvio_fe_track_event on pageable records: the same frames through two
    handles of one configuration, alternating; per call the median over the frames behind the first one"""
    a, b = FE.FeatureTracker(FE.make_config(W, H)), FE.FeatureTracker(FE.make_config(W, H))
    res = {}
    try:
        for name in ("track_event, records", "EVT3, read-out order, vectors", "EVT3, no vectors", "EVT2"):
            res[name] = []
        for _ in range(ROUNDS + 1):  # (the first round warms up: allocations, clocks)
            for name in res:
                ft = a if name.startswith("track_event") else b
                ft.reset()
                per = []
                for i, fr in enumerate(frames):
                    L_, R_ = fr["rec"]
                    t0 = time.perf_counter()
                    if ft is a:
                        ft.trackEvent(float(event_times(L_[-1:])[0]), L_, R_, i % 2 == 0, copy=False)
                    else:
                        fmt, wl, wr = fr["words"][name]
                        ft.track_raw(fmt, wl, wr, base, i % 2 == 0, copy=False)
                    per.append((time.perf_counter() - t0) * 1e6)
                res[name].append(float(np.median(per[1:])) if len(per) > 1 else per[0])
        n = sum(len(fr["rec"][0]) + len(fr["rec"][1]) for fr in frames) / len(frames)
        for name, v in res.items():
            m = med(v[1:])
            nbytes = sum(fr["words"][name][1].nbytes + fr["words"][name][2].nbytes for fr in frames) / len(frames) if name in frames[0]["words"] else 16 * n
            print("%s track A/B  %-30s %8.1f us per call (%.1f - %.1f), %.2f MB of %s per call" % (tag, name, m[0], m[1], m[2], nbytes / 1e6, "words" if name in frames[0]["words"] else "records (packed to half before they cross PCIe)"))
            rows.append(dict(batch=tag, ab="track", path=name, call_us=m, link_bytes=nbytes, events_per_call=n))
    finally:
        a.close()
        b.close()


def main():
    L = FE.load_library()
    global FORMATS, DEVICE_ONLY
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    if "--formats" in sys.argv:
        FORMATS = set(sys.argv[sys.argv.index("--formats") + 1].split(","))
    DEVICE_ONLY = "--device-only" in sys.argv
    rows = []
    for tag, W, H, rate, n_frames in SHAPES:
        if only and tag != only:
            continue
        st = SceneStream(W=W, H=H, rate=rate, seed=3)
        base = st.t_us - 1000
        frames = []
        for _ in range(1 if DEVICE_ONLY else n_frames):
            left, right, _ = st.next_batch()
            fr = dict(rec=[], words={})
            encs = []
            for ev in (left, right):
                rec, enc = encodings(ev, base)
                fr["rec"].append(rec)
                encs.append(enc)
            for (name, fmt, wl), (_, _, wr) in zip(*encs):
                fr["words"][name] = (fmt, wl, wr)
            frames.append(fr)
        os.environ["ESVIO_FE_RAW_PINNED_COPY"] = "0"
        ft = FE.FeatureTracker(FE.make_config(W, H))
        os.environ["ESVIO_FE_RAW_PINNED_COPY"] = "1"
        ft_copy = FE.FeatureTracker(FE.make_config(W, H))
        del os.environ["ESVIO_FE_RAW_PINNED_COPY"]
        rec = frames[0]["rec"][0]
        cap = max(w.nbytes for _, w, _ in frames[0]["words"].values()) + 64
        pin, dsrc, ddst = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.HOST, cap, C.byref(pin)) == 0
        assert L.esvio_fe_mem_alloc(FE.DEVICE, cap, C.byref(dsrc)) == 0
        assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * len(rec), C.byref(ddst)) == 0
        pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(cap,))
        for name, (fmt, wl, _) in frames[0]["words"].items():
            stage_bench(L, ft, ft_copy, tag, rec, name, fmt, wl, base, (pin, pinned, dsrc, ddst), rows)
            if fmt == FE.RAW_EVT21:
                drec, dwords = dense_evt21(len(rec), W, base)
                stage_bench(L, ft, ft_copy, tag, drec, "EVT2.1, full masks", fmt, dwords, base, (pin, pinned, dsrc, ddst), rows)
            if tag == "C3" and name != "EVT3, no vectors" and not DEVICE_ONLY:
                pinned_sweep(L, ft, ft_copy, tag, name, fmt, wl, len(rec), base, (pin, pinned, dsrc, ddst), rows)
        L.esvio_fe_mem_free(FE.HOST, pin)
        L.esvio_fe_mem_free(FE.DEVICE, dsrc)
        L.esvio_fe_mem_free(FE.DEVICE, ddst)
        ft.close()
        ft_copy.close()
        if not DEVICE_ONLY:
            track_ab(tag, W, H, frames, base, rows)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
