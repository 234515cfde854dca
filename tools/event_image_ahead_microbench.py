"""What the event images cost the replay schedule (esvio_fe_set_event_images, ESVIO_FE_EVENT_IMAGES_AHEAD).  Two shapes —
C3 640x480 (2 x 167 k events a batch) and C5's batch 1280x720 (2 x 3.3 M) — of the scene stream, device-resident
events, the schedule the README's headline is measured in: batches announced 3 ahead, lazy returns, the launch thread,
publish every other frame.  Per shape, wall ms per step (esvio_fe_set_next_batch + esvio_fe_track_event) as the
calling thread sees it:
  off        the setting off
  ahead      mode 2, nobody fetches
  ahead+get  mode 2, esvio_fe_get_event_canvas into device memory after every call
Each figure: the median of PASSES passes over the shape's batches after a warm-up pass, and the passes' min - max; a
pass starts from esvio_fe_reset.  The three handles run their passes in turn (off, ahead, ahead+get, off, ...), so a drift
of the machine meets all three.  One process, no retries; run it under a time limit:

    timeout -k 10 600 python tools/event_image_ahead_microbench.py > profiles/event_image_ahead_microbench.txt
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import event_times  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

PASSES, AHEAD = 7, 3
SHAPES = (("C3", 640, 480, 5e6, 40), ("C5 batch", 1280, 720, 100e6, 8))


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def one_pass(ft, args, canvas):
    """ms per step of one pass over the batches from a reset handle"""
    ft.reset()
    nxt, h, L_ = 1, ft._hd.h, ft._hd.L
    t0 = time.perf_counter()
    for k, (dl, dr, t) in enumerate(args):
        while nxt < len(args) and nxt <= k + AHEAD:
            ft.set_next_batch(args[nxt][2], args[nxt][0], args[nxt][1], nxt % 2 == 0)
            nxt += 1
        ft.trackEvent(t, dl, dr, k % 2 == 0, copy=False)
        if canvas is not None:
            ft._hd.check(L_.esvio_fe_get_event_canvas(h, canvas, FE.DEVICE))
    ft.finish(copy=False)
    return (time.perf_counter() - t0) / len(args) * 1e3


def main():
    L_ = FE.load_library()
    for tag, W, H, rate, n in SHAPES:
        s = SceneStream(W, H, rate=rate, seed=4, n_rect=12, size=(30.0, 90.0))
        bufs, args, nl, nr = [], [], 0, 0
        for _ in range(n):
            L, R, _ = s.next_batch()
            bufs += [FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(R, FE.DEVICE)]
            args.append((bufs[-2].arg, bufs[-1].arg, event_times(L)[-1]))
            nl, nr = max(nl, len(L)), max(nr, len(R))
        canvas = C.c_void_p()
        assert L_.esvio_fe_mem_alloc(FE.DEVICE, W * H * 6, C.byref(canvas)) == 0
        runs = []
        for name, mode, dst in (("off", 0, None), ("ahead", FE.EVENT_IMAGES_AHEAD, None), ("ahead+get", FE.EVENT_IMAGES_AHEAD, canvas)):
            ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=300, min_dist=10, f_ransac=1))
            free0 = ft.device_memory()[0]
            ft.set_event_images(mode)
            held = free0 - ft.device_memory()[0]
            ft.set_lazy_new_stereo(True)
            ft.set_launch_thread(True)
            ft.reserve(nl, nr)
            runs.append((name, ft, dst, held, []))
        for p in range(PASSES + 1):
            for name, ft, dst, held, laps in runs:
                ms = one_pass(ft, args, dst)
                if p:
                    laps.append(ms)
        print("%s %dx%d scene stream, %d batches of up to %d + %d events, announced %d ahead, lazy, launch thread" % (tag, W, H, n, nl, nr, AHEAD))
        base = med(runs[0][4])[0]
        for name, ft, dst, held, laps in runs:
            m = med(laps)
            print("    %-10s %7.4f ms/step (%.4f - %.4f)  %+7.4f ms = %+5.1f %% against off | the setting holds %5.1f MB = %4.1f bytes per pixel"
                  % (name, m[0], m[1], m[2], m[0] - base, 100 * (m[0] - base) / base, held / 1e6, held / (W * H)))
            ft.close()
        L_.esvio_fe_mem_free(FE.DEVICE, canvas)
        for b in bufs:
            b.free()


if __name__ == "__main__":
    main()
