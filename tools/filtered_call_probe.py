"""Host time of esvio_fe_track_event_filtered from the call to the start of tracking: both cameras of a C3-sized scene
batch (640 x 480, ~167 k events each, device memory) filtered with a rule that keeps nothing (window 1 ns, support 8),
so that the call returns where tracking would start — both chains enqueued, their result blocks read, every wait the
call makes.  Median of BLOCKS blocks of REPS calls after a warm-up block, min - max; one JSON line.  Works on any tree
that has the entry point (ESVIO_FE_LIB or the tree's own library):

    timeout -k 10 120 python tools/filtered_call_probe.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402

BLOCKS, REPS = 5, 10


def main():
    w, h = 640, 480
    left, right, _ = SceneStream(W=w, H=h, rate=167_000 * 30.0, seed=11).next_batch()
    tr = FE.FeatureTracker(FE.make_config(w, h))
    bl, br = FE.EventBuffer(left, FE.DEVICE), FE.EventBuffer(right, FE.DEVICE)
    us = []
    for b in range(BLOCKS + 1):
        t = 0.0
        for _ in range(REPS):
            tr.filter_reset()
            t0 = time.perf_counter()
            kept, _ = tr.trackEventFiltered(bl.arg, br.arg, 1, 8)
            t += time.perf_counter() - t0
            assert kept[0] == 0
        if b:
            us.append(t / REPS * 1e6)
    print(json.dumps(dict(probe="track_event_filtered to the start of tracking", nL=len(left), nR=len(right),
                          us_median=float(np.median(us)), us_min=float(np.min(us)), us_max=float(np.max(us)), blocks=us)))
    bl.free(), br.free()
    tr.close()


if __name__ == "__main__":
    main()
