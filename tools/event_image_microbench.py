"""Event-image micro-benchmark (esvio_fe_set_event_images).  Three batches — C1 346x260 (2 x 68 k events), C3 640x480
(2 x 167 k), C5 1280x720 (2 x 3.3 M) — of the scene stream and of the uniform (Poisson) stream, in device memory.  Per
batch, from the LIBRARY'S OWN TIMERS (HIP events around every launch; esvio_fe_event_image_kernel_stats for the two new
kernels, esvio_fe_get_kernel_stats for the rest), per launch:
  k_evimg_mark and k_evimg_emit in its ACCUMULATE form under esvio_fe_create_sae_stereo (one launch each per call, both
  cameras), and in its FRESH form under esvio_fe_track_event (pub 0; a plain call on device events is split by camera:
  two launches of each per call, one camera each);
  beside them the SAE chain of the same calls (k_tile_hist + k_tile_scan + k_tile_scatter + k_tile_apply per call);
  the bytes each kernel moves (mark: the 16-byte record in, one atomic word out; emit: four mark words in, three image
  words out per group of four pixels) as a share of the measured copy rate.
The getters' wall time: one camera's image and the canvas into pageable, pinned and device memory.
Per figure: the median of BLOCKS blocks of REPS after a warm-up block, and the blocks' min - max.  One process, one pass,
no retries; run it under a time limit:

    timeout -k 10 600 python tools/event_image_microbench.py > profiles/event_image_microbench.txt
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import event_times  # noqa: E402
from esvio_amd.synth import PoissonStream, SceneStream  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (KERNELS.md)
BLOCKS, REPS = 5, 10
SHAPES = (("C1", 346, 260, 2.05e6), ("C3", 640, 480, 5e6), ("C5", 1280, 720, 100e6))
CHAIN = ("k_tile_hist", "k_tile_scan", "k_tile_scatter", "k_tile_apply")


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def evimg_stats(ft, which):
    ms, n = C.c_double(0), C.c_uint64(0)
    ft._hd.check(ft._hd.L.esvio_fe_event_image_kernel_stats(ft._hd.h, which, C.byref(ms), C.byref(n), None))
    return ms.value, n.value


def timed_blocks(ft, call):
    """per block: (mark us / launch, emit us / launch, SAE chain us / call, mark launches / call, emit launches / call)"""
    rows = []
    for blk in range(BLOCKS + 1):
        ft.reset_kernel_stats()
        for _ in range(REPS):
            call()
        (mm, mn), (em, en) = evimg_stats(ft, 0), evimg_stats(ft, 1)
        st = ft.kernel_stats()
        chain = sum(st[k]["ms"] for k in CHAIN)
        if blk:
            rows.append((mm / mn * 1e3, em / en * 1e3, chain / REPS * 1e3, mn / REPS, en / REPS))
    return [med([r[k] for r in rows]) for k in range(3)] + [rows[0][3], rows[0][4]]


def wall_us(call):
    laps = []
    for _ in range(BLOCKS + 1):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        laps.append((time.perf_counter() - t0) / REPS * 1e6)
    return med(laps[1:])


def main():
    L_ = FE.load_library()
    for tag, W, H, rate in SHAPES:
        for sname, S in (("scene", SceneStream), ("uniform", PoissonStream)):
            L, R, _ = S(W, H, rate=rate, seed=4).next_batch()
            nL, nR, P = len(L), len(R), W * H
            ft = FE.FeatureTracker(FE.make_config(W, H))
            ft.set_event_images(True)
            ft.reserve(nL, nR)
            dL, dR = FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(R, FE.DEVICE)
            ft.set_profiling(True)
            groups = (P + 3) // 4
            print("%s %dx%d %s stream: %d + %d events, %d pixels" % (tag, W, H, sname, nL, nR, P))
            t = [event_times(L)[-1]]

            def stage():
                ft.detector.createSAE_stereo(dL.arg, dR.arg)

            def track():
                t[0] += 1.0 / 30
                ft.trackEvent(t[0], dL.arg, dR.arg, False)

            for label, call in (("stage call, ACCUMULATE", stage), ("track call, FRESH", track)):
                mark, emit, chain, mpc, epc = timed_blocks(ft, call)
                n_launch = (nL + nR) / mpc  # events per mark launch
                mark_gbs = n_launch * 20 / (mark[0] * 1e-6) / 1e9
                cams = 2 / epc  # cameras per emit launch
                emit_gbs = groups * 28 * cams / (emit[0] * 1e-6) / 1e9
                print("    %-24s k_evimg_mark %7.1f us (%.1f - %.1f) per launch, %.0f per call: %5.0f GB/s = %4.1f %% of the copy rate | "
                      "k_evimg_emit %6.1f us (%.1f - %.1f) per launch, %.0f per call, %.0f camera(s) each: %5.0f GB/s = %4.1f %% | "
                      "SAE chain %7.1f us (%.1f - %.1f) per call | mark + emit = %4.1f %% of the chain"
                      % (label, mark[0], mark[1], mark[2], mpc, mark_gbs, 100 * mark_gbs / HBM_GBS, emit[0], emit[1], emit[2], epc, cams,
                         emit_gbs, 100 * emit_gbs / HBM_GBS, chain[0], chain[1], chain[2],
                         100 * (mark[0] * mpc + emit[0] * epc) / chain[0]))
            ft.set_profiling(False)
            # the getters: wall time with their wait
            img, canvas = np.zeros((H, W, 3), np.uint8), np.zeros((H, 2 * W, 3), np.uint8)
            pin, dev = C.c_void_p(), C.c_void_p()
            assert L_.esvio_fe_mem_alloc(FE.HOST, canvas.nbytes, C.byref(pin)) == 0 and L_.esvio_fe_mem_alloc(FE.DEVICE, canvas.nbytes, C.byref(dev)) == 0
            h = ft._hd.h
            for what, nbytes, calls in (
                    ("image ", img.nbytes, (("pageable", lambda: L_.esvio_fe_get_event_image(h, 0, FE._p(img), FE.HOST)),
                                            ("pinned", lambda: L_.esvio_fe_get_event_image(h, 0, pin, FE.HOST)),
                                            ("device", lambda: L_.esvio_fe_get_event_image(h, 0, dev, FE.DEVICE)))),
                    ("canvas", canvas.nbytes, (("pageable", lambda: L_.esvio_fe_get_event_canvas(h, FE._p(canvas), FE.HOST)),
                                               ("pinned", lambda: L_.esvio_fe_get_event_canvas(h, pin, FE.HOST)),
                                               ("device", lambda: L_.esvio_fe_get_event_canvas(h, dev, FE.DEVICE))))):
                parts = []
                for where, call in calls:
                    assert call() == 0
                    w = wall_us(call)
                    parts.append("%s %7.1f us (%.1f - %.1f) = %5.1f GB/s" % (where, w[0], w[1], w[2], nbytes / w[0] / 1e3))
                print("    getter, %s %8d bytes: %s" % (what, nbytes, " | ".join(parts)))
            L_.esvio_fe_mem_free(FE.HOST, pin)
            L_.esvio_fe_mem_free(FE.DEVICE, dev)
            dL.free()
            dR.free()
            ft.close()


if __name__ == "__main__":
    main()
