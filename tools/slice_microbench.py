"""esvio_fe_slice_events / esvio_fe_feed_* micro-benchmark.  The bench's scene stream at C3's batch (640x480, 5 Mev/s:
~167 k events per camera and window) and C5's (1280x720, 100 Mev/s: ~3.3 M), 30 Hz.

Stage: STAGE_WINDOWS consecutive batches of the left camera as ONE call (so the call closes windows, as a chunk of a
recording does).  Per launch of the chain the time from the LIBRARY'S OWN TIMERS (esvio_fe_get_kernel_stats: HIP events
around each launch — not a rocprofv3 summary); 2 x 16 B x events (the records are read twice) over the three launches'
time as a share of the HBM copy rate; the call's wall time from device and from pageable memory.  For context, the path
without the call: the records downloaded, then cut on one core by the plain sequential loop (tools/slice_seq_cut.cpp,
if it has been built) and, beside it, by numpy's vectorised form of the rule (stamps, searchsorted in the boundary
table, maximum.accumulate, the rises); the cuts of all three are compared.

Feed against its alternative (C3 only): FEED_WINDOWS windows of both cameras as EVT2 words in chunks of CHUNK_BYTES,
(a) pushed through the feed and tracked where the windows lie, (b) decoded chunk by chunk into host records
(esvio_fe_decode_raw), cut on the host as above and tracked from host records (esvio_fe_track_event).  Two handles of one
configuration, both in one process, alternating, ROUNDS times; the results of the two are compared.  Per figure: the
median of the blocks / rounds and their min - max.  One process, one pass, no retries; run it under a time limit:

    g++ -O2 -std=c++17 -ffp-contract=off tools/slice_seq_cut.cpp -o tools/_bin/slice_seq_cut
    timeout -k 10 600 python tools/slice_microbench.py [--json out.json] [--only C3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import slice_ref as S  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import EVENT_DTYPE, event_times  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402
from raw_microbench import encode_evt2_np, fields_of  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (8 TB/s spec)
BLOCKS, REPS, ROUNDS = 5, 20, 5
STAGE_WINDOWS, FEED_WINDOWS, CHUNK_BYTES = 3, 8, 256 << 10
SHAPES = (("C3", 640, 480, 5e6), ("C5", 1280, 720, 100e6))
SEQ = os.path.join(ROOT, "tools", "_bin", "slice_seq_cut")
KERNELS = ("k_slice_reduce", "k_slice_scan", "k_slice_cuts")
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def cat(parts):
    """np.concatenate packs a padded record dtype (16 -> 13 bytes): join the batches keeping EVENT_DTYPE"""
    out = np.zeros(sum(len(p) for p in parts), EVENT_DTYPE)
    at = 0
    for p in parts:
        out[at:at + len(p)] = p
        at += len(p)
    return out


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def host_cut(rec, bounds):
    """the rule on one core, vectorised: -> cuts (as esvio_fe_slice_events', for a fresh camera)"""
    c = np.searchsorted(bounds, event_times(rec), side="right")
    m = np.maximum.accumulate(c)
    prev = np.concatenate(([0], m[:-1]))
    rise = np.flatnonzero(m > prev)
    return np.repeat(rise, (m - prev)[rise])


def boundaries(first, frequency, upto):
    s = S.Slicer(frequency, (int(first["sec"]), int(first["nsec"])))
    k = 0
    while S.to_sec(*s.boundary(k)) <= upto:
        k += 1
    return np.array([S.to_sec(*s.boundary(j)) for j in range(k + 1)])


def stage_bench(tag, W, H, rate, rows):
    st = SceneStream(W=W, H=H, rate=rate, seed=12345)
    rec = cat([st.next_batch()[0] for _ in range(STAGE_WINDOWS)])
    n = len(rec)
    ft = FE.FeatureTracker(FE.make_config(W, H))
    L, h = ft._hd.L, ft._hd.h
    hip = C.CDLL("libamdhip64.so")
    dev = FE.EventBuffer(rec, FE.DEVICE)
    bounds = boundaries(rec[0], 30.0, float(event_times(rec).max()))
    want = host_cut(rec, bounds)
    print("%s: %d events in one call, %d windows closed" % (tag, n, len(want)))
    for src, arg in (("device", dev.arg), ("pageable", rec)):
        def call():
            ft.slice_reset()
            return ft.slice_events(0, arg, 30.0)

        for _ in range(3):
            cuts, info = call()
        assert np.array_equal(cuts, want) and info.closed == len(want) >= STAGE_WINDOWS - 1
        reps = REPS if n < 1_000_000 or src == "device" else 5
        ks, call_us = {k: [] for k in KERNELS}, []
        for _ in range(BLOCKS):
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            call_us.append((time.perf_counter() - t0) / reps * 1e6)
            stats = ft.kernel_stats(stages=True)
            ft.set_profiling(False)
            for k in ks:
                assert stats[k]["launches"] == reps
                ks[k].append(stats[k]["ms"] / reps * 1e3)
        k = {name: med(v) for name, v in ks.items()}
        chain = sum(k[name][0] for name in KERNELS)
        gbs = 2 * 16 * n / (chain * 1e-6) / 1e9
        c = med(call_us)
        print("    %-9s reduce %7.1f us | scan %5.1f us | cuts %7.1f us | chain %7.1f us: 2 x 16 B x events = %6.0f GB/s = %4.1f %% of HBM | "
              "call %8.1f us (%.1f - %.1f) = %7.1f Mev/s" % (src, k[KERNELS[0]][0], k[KERNELS[1]][0], k[KERNELS[2]][0], chain, gbs,
                                                              100 * gbs / HBM_GBS, c[0], c[1], c[2], n / c[0]))
        rows.append(dict(batch=tag, n=n, windows=len(want), source=src, kernels_us=k, chain_us=chain, read_gbs=gbs, hbm_frac=gbs / HBM_GBS,
                         call_us=c))
    # the path without the call: download, then one core
    back = np.zeros(n, rec.dtype)
    down, cut = [], []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(dev.arg[0]), C.c_size_t(16 * n), 2) == 0
        t1 = time.perf_counter()
        got = host_cut(back, bounds)
        t2 = time.perf_counter()
        down.append((t1 - t0) * 1e6), cut.append((t2 - t1) * 1e6)
    assert np.array_equal(got, want)
    d, q = med(down), med(cut)
    print("    without the call: download %8.1f us (%.1f - %.1f) + numpy on one core %9.1f us (%.1f - %.1f)" % (d + q))
    row = dict(batch=tag, n=n, source="download + one core", download_us=d, host_cut_us=q)
    if os.path.exists(SEQ):  # the plain loop on one core, over the downloaded records (a fresh camera, as the calls above)
        with tempfile.NamedTemporaryFile(suffix=".rec") as f:
            f.write(back.tobytes())
            f.flush()
            line = subprocess.check_output([SEQ, f.name, "30", "7"]).decode().split()
        assert (int(line[0]), int(line[1]), int(line[2])) == (n, len(want), int(want.sum())), line
        row["seq_loop_us"] = tuple(float(v) for v in line[3:6])
        print("                      the sequential loop on one core %9.1f us (%.1f - %.1f)" % row["seq_loop_us"])
    rows.append(row)
    dev.free()
    ft.close()


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def feed_bench(tag, W, H, rate, rows):
    st = SceneStream(W=W, H=H, rate=rate, seed=12345)
    base = st.t_us - 1000
    recs, words = [[], []], []
    for _ in range(FEED_WINDOWS + 1):
        left, right, _ = st.next_batch()
        recs[0].append(left), recs[1].append(right)
    recs = [cat(r) for r in recs]
    for cam in range(2):
        x, y, p, t = fields_of(recs[cam])
        words.append(encode_evt2_np(x, y, p, t - base))
    wpc = CHUNK_BYTES // 4
    a, b = FE.FeatureTracker(FE.make_config(W, H)), FE.FeatureTracker(FE.make_config(W, H))
    bounds = boundaries(recs[0][0], 30.0, float(max(event_times(recs[0]).max(), event_times(recs[1]).max())))

    def via_feed():
        a.reset()
        a.feed_open(30.0)
        snaps, pos = [], [0, 0]
        while pos[0] < len(words[0]) or pos[1] < len(words[1]):
            for cam in range(2):
                if pos[cam] < len(words[cam]):
                    a.feed_push_raw(cam, FE.RAW_EVT2, words[cam][pos[cam]:pos[cam] + wpc], base)
                    pos[cam] += wpc
                while a.feed_peek() is not None:
                    if a.feed_track(True).tracked:
                        snaps.append(results(a))
        a.feed_close()
        return snaps

    def via_host():
        b.reset()
        got, pos = [[], []], [0, 0]
        for cam in range(2):
            while pos[cam] < len(words[cam]):
                rec, _ = b.decode_raw(cam, FE.RAW_EVT2, words[cam][pos[cam]:pos[cam] + wpc], base)
                got[cam].append(rec)
                pos[cam] += wpc
        full = [cat(g) for g in got]
        cuts = [host_cut(full[cam], bounds) for cam in range(2)]
        snaps, lo = [], [0, 0]
        for k in range(min(len(cuts[0]), len(cuts[1]))):
            Lw, Rw = full[0][lo[0]:cuts[0][k]], full[1][lo[1]:cuts[1][k]]
            lo = [cuts[0][k], cuts[1][k]]
            if len(Lw):
                b.trackEvent(float(event_times(Lw[-1:])[0]), Lw, Rw, True)
                snaps.append(results(b))
        return snaps

    assert via_feed() == via_host()  # (warm-up, and the two paths track the same windows to the same results)
    tf, th = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        sa = via_feed()
        t1 = time.perf_counter()
        sb = via_host()
        t2 = time.perf_counter()
        tf.append((t1 - t0) * 1e3), th.append((t2 - t1) * 1e3)
    assert sa == sb and len(sa) >= FEED_WINDOWS - 1
    f, hh = med(tf), med(th)
    print("%s feed A/B: %d + %d events as EVT2 words in chunks of %d KiB, %d windows tracked: feed %8.2f ms (%.2f - %.2f) | decode to host, "
          "cut on the host, track from host records %8.2f ms (%.2f - %.2f)" % ((tag, len(recs[0]), len(recs[1]), CHUNK_BYTES >> 10, len(sa)) + f + hh))
    rows.append(dict(batch=tag, feed_ab=True, events=[len(recs[0]), len(recs[1])], windows=len(sa), chunk_bytes=CHUNK_BYTES, feed_ms=f,
                     host_path_ms=hh))
    a.close()
    b.close()


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    rows = []
    for tag, W, H, rate in SHAPES:
        if only and tag != only:
            continue
        stage_bench(tag, W, H, rate, rows)
        if tag == "C3":
            feed_bench(tag, W, H, rate, rows)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
