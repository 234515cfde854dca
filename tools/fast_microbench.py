"""esvio_fe_fast_corners micro-benchmark: per-kernel time (esvio_fe_get_kernel_stats) of k_fast_score, k_fast_collect
and the k_compact that follows them, on the scene stream's time surface at the sensor sizes of C1 / C3 / C5, barrier
20, arc 10, non-max on / off (and arc 9), with the bytes each launch has to move and the share of the HBM / L2 rate
that is.  One process, one pass, no retries; run it under a time limit:

    timeout -k 10 300 python tools/fast_microbench.py [--json out.json]

The reference's one-core CPU time (plain C++, from tests/golden/fast_ref_*.npz: another machine, context only) is
printed beside each size."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import event_times  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

HBM_GBS = 6290.0   # measured float4 copy rate of an MI355X (8 TB/s spec)
L2_GBS = 34500.0   # aggregate L2 rate
REPS = 200
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
CPU_REF = {(346, 260): ("fast_ref_ts_346x260.npz", "ts346"), (640, 480): ("fast_ref_ts_640x480.npz", "ts640"),
           (1280, 720): ("fast_ref_ts_1280x720.npz", "ts1280")}


def main():
    rows = []
    for (W, H), rate in (((346, 260), 1e6), ((640, 480), 5e6), ((1280, 720), 6e6)):
        s = SceneStream(W, H, rate=rate, seed=12345)
        ft = FE.FeatureTracker(FE.make_config(W, H))
        for _ in range(3):
            L, R, _ = s.next_batch()
            ft.trackEvent(event_times(L)[-1], L, R, True)
        P = W * H
        z = np.load(os.path.join(GOLDEN, CPU_REF[(W, H)][0]))
        cpu = z[CPU_REF[(W, H)][1] + "_cpu_ms"]  # detect_9, detect_10, score_10, nonmax_3x3 at barrier 20
        print("%dx%d  reference, one CPU core (%s): detect_9 %.3f ms, detect_10 %.3f, score_10 %.3f, nonmax_3x3 %.3f"
              % (W, H, str(z["compiler"]), cpu[0], cpu[1], cpu[2], cpu[3]))
        for arc, nonmax in ((10, True), (10, False), (9, False)):
            ft.fast_corners(arc=arc, nonmax=nonmax)  # (first call: allocations)
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            t0 = time.perf_counter()
            for _ in range(REPS):
                xy, sc, (n, nd) = ft.fast_corners(arc=arc, barrier=20, nonmax=nonmax, capacity=0, want_count=True)
            call_us = (time.perf_counter() - t0) / REPS * 1e6
            st = ft.kernel_stats()
            ft.set_profiling(False)
            us = {k: st[k]["ms"] / max(st[k]["launches"], 1) * 1e3 for k in ("k_fast_score", "k_fast_collect", "k_compact")}
            # bytes a launch has to move: the image read once + the map written; the map read once + 8 B per corner
            # written; 8 B per corner read and written + the block counts
            nblk = (P + 255) // 256
            by = {"k_fast_score": 2 * P, "k_fast_collect": P + 8 * n + 4 * nblk, "k_compact": 16 * n + 4 * nblk}
            row = dict(W=W, H=H, arc=arc, nonmax=int(nonmax), corners=int(n), detected=int(nd), call_us=call_us,
                       cpu_ref_ms=[float(v) for v in cpu])
            line = "  arc %2d nonmax %d: %6d corners (%6d detected)" % (arc, nonmax, n, nd)
            for k in us:
                gbs = by[k] / (us[k] * 1e-6) / 1e9 if us[k] > 0 else 0.0
                row[k] = dict(us=us[k], bytes=by[k], gbs=gbs, hbm_frac=gbs / HBM_GBS, l2_frac=gbs / L2_GBS)
                line += " | %s %.2f us %.0f KB %.0f GB/s = %.1f %% HBM, %.1f %% L2" % (
                    k, us[k], by[k] / 1e3, gbs, 100 * gbs / HBM_GBS, 100 * gbs / L2_GBS)
            print(line + " | whole call (capacity 0) %.1f us" % call_us)
            rows.append(row)
        ft.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
