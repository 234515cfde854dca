"""trackEvent with ESVIO_FE_DETECT_FAST beside the default (Arc*): the candidate pass's per-launch times
(esvio_fe_get_kernel_stats) and the plain call's time per step, from one run at 640 x 480 on bench.py's scene stream
(5 Mev/s per camera, 30 Hz batches, every second frame published, max_cnt 300, events in device memory).

Schedule: PLAIN calls — nothing announced, one batch in flight; the candidate pass runs on the side stream beside
the temporal LK.  Per detector one handle: warm-up, a timed pass with the profiler off (ms_per_step: host clock
around calls that each end in a device synchronisation), then a pass with the per-kernel hipEvent brackets on (each
bracket adds 4-5 us to its figure, KERNELS.md "FAST").  One process, no retries; run it under a time limit:

    timeout -k 10 300 python tools/fast_detect_timing.py [--json out.json] [--barrier 20]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import event_times  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

W, H, WARMUP, STEPS, PROFILED = 640, 480, 20, 60, 40
PASS = {"arc": ("k_arc_map", "k_arc_ev", "k_dedup", "k_compact", "k_select_mw"),
        "fast": ("k_fast_score", "k_fast_collect", "k_compact", "k_radix_pass", "k_select_mw")}


def main():
    barrier = int(sys.argv[sys.argv.index("--barrier") + 1]) if "--barrier" in sys.argv else 20
    s = SceneStream(W, H, rate=5e6, batch_hz=30.0, seed=12345)
    host = [s.next_batch()[:2] for _ in range(WARMUP + STEPS + PROFILED)]
    bufs = [(FE.EventBuffer(L, FE.DEVICE), FE.EventBuffer(R, FE.DEVICE)) for L, R in host]
    times = [event_times(L)[-1] for L, _ in host]
    out = {}
    for name, det in (("arc", FE.DETECT_ARC), ("fast", FE.DETECT_FAST), ("arc again", FE.DETECT_ARC)):
        ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=300))
        ft.reserve(max(len(L) for L, _ in host), max(len(R) for _, R in host))
        ft.set_detector(det, barrier)

        def run(lo, hi):
            new = 0
            for f in range(lo, hi):
                ft.trackEvent(times[f], bufs[f][0].arg, bufs[f][1].arg, f % 2 == 0, copy=False)
                new += int((ft.track_cnt == 1).sum())
            return new

        run(0, WARMUP)
        t0 = time.perf_counter()
        new = run(WARMUP, WARMUP + STEPS)
        ms = (time.perf_counter() - t0) / STEPS * 1e3
        ft.set_profiling(True)
        ft.reset_kernel_stats()
        run(WARMUP + STEPS, WARMUP + STEPS + PROFILED)
        st = ft.kernel_stats()
        ft.set_profiling(False)
        n_tracks = len(ft.ids)
        ft.close()
        key = name.split()[0]
        us = {k: (st[k]["ms"] / st[k]["launches"] * 1e3, int(st[k]["launches"])) for k in PASS[key] if st[k]["launches"]}
        out[name] = dict(ms_per_step=ms, new_corners_per_published_frame=new / (STEPS / 2), tracks=n_tracks,
                         us_per_launch={k: v[0] for k, v in us.items()}, launches={k: v[1] for k, v in us.items()})
        print("%-9s plain call %.4f ms/step, %.1f new corners per published frame, %d tracks at the end | %s"
              % (name, ms, new / (STEPS / 2), n_tracks,
                 ", ".join("%s %.2f us x %d" % (k, v[0], v[1]) for k, v in us.items())))
    for bl, br in bufs:
        bl.free()
        br.free()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(dict(width=W, height=H, barrier=barrier, schedule="plain calls", runs=out), f, indent=1)


if __name__ == "__main__":
    main()
