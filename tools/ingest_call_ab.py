"""Per-call wall time of the ingest entry points of ONE built tree, for comparing two trees (a parent commit's export
and this one) by alternating processes: host-side call overhead is what a refactoring of fe_api.cpp can move.  Per
figure: the caller's clock around the Python wrapper's call (every call ends in the library's own stream wait), 20 calls
of warm-up, then BLOCKS blocks of REPS calls; printed: the median, min and max of the blocks' means, in us per call.
One 640 x 480 handle; EVT2 words, AEDAT packets of 1000 events and a bag chunk of one message per camera, of 1000
events (a 4 KiB chunk: the call's overhead is nearly all there is) and of 167 000 (C3's batch); esvio_fe_track_raw /
_track_aedat on 167 000 left and 120 000 right events; esvio_fe_feed_push_raw of 1000-event chunks.

    for i in 1 2 3 4; do
      timeout -k 10 100 python tools/ingest_call_ab.py <parent tree> parent$i [only]
      timeout -k 10 100 python tools/ingest_call_ab.py . new$i [only]
    done

<tree>: a checkout with its libesvio_fe.so built; the label is printed in front of every line; `only`: time just the
rows whose name contains it.  profiles/ingest_refactor_ab.txt is a record of such a run."""
import os
import sys
import time

tree = os.path.abspath(sys.argv[1])
label = sys.argv[2]
only = sys.argv[3] if len(sys.argv) > 3 else ""
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(tree, "tests"))
import numpy as np  # noqa: E402

import aedat_ref as A  # noqa: E402
import bag_ref as B  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402

assert os.path.abspath(FE.__file__).startswith(tree), FE.__file__
BLOCKS, REPS = 7, 150
W, H = 640, 480


def evt2_words(n, rng):
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    t = 1_000_000 + np.sort(rng.integers(0, 33_000, n))
    ev = ((p.astype(np.int64) << 28) | ((t & 63) << 22) | (x << 11) | y).astype(np.int64)
    th = t >> 6
    new = np.ones(n, bool)
    new[1:] = th[1:] != th[:-1]
    pos = np.arange(n) + np.cumsum(new)  # each event behind the TIME_HIGH words in front of it
    out = np.zeros(n + int(new.sum()), np.int64)
    out[pos] = ev
    out[pos[new] - 1] = 0x80000000 | th[new]
    return out.astype("<u4")


def aedat_bytes(n, rng):
    out = []
    for k in range(0, n, 1000):
        m = min(1000, n - k)
        data = (1 | (rng.integers(0, 2, m) << 1) | (rng.integers(0, H, m) << 2) | (rng.integers(0, W, m) << 17)).astype("<u4")
        ts = (1_000_000 + 33 * k // 1000 * 1000 + np.sort(rng.integers(0, 33, m))).astype("<i4")
        rec = np.empty((m, 2), "<u4")
        rec[:, 0], rec[:, 1] = data, ts.view("<u4")
        out.append(A.HEADER.pack(1, 1, 8, 4, 0, m, m, m) + rec.tobytes())
    return b"".join(out)


def bag_bytes(n, rng):
    conns = B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5) + B.connection_record(1, B.RIGHT, B.EVENT_TYPE, B.EVENT_MD5)
    body = conns
    for cam in (0, 1):
        t = 1000 + np.sort(rng.integers(0, 33_000_000, n))
        wire = B.wire_events(rng.integers(0, 346, n), rng.integers(0, 260, n), 7 + t // 10 ** 9, t % 10 ** 9, rng.integers(0, 2, n))
        body += B.message_record(cam, (7, 1), B.event_array(1, (7, 1), wire))
    return B.chunk_record(body)


def timed(name, n, call):
    if only not in name:
        return
    try:
        for _ in range(20):
            call()
    except Exception as e:  # (a call this driver set up wrongly: said, not timed)
        print("%s %-28s n=%-7d not timed: %s" % (label, name, n, str(e)[:120]), flush=True)
        return
    meds = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        meds.append((time.perf_counter() - t0) / REPS * 1e6)
    print("%s %-28s n=%-7d us/call median %.2f min %.2f max %.2f" % (label, name, n, float(np.median(meds)), min(meds), max(meds)), flush=True)


rng = np.random.default_rng(5)
ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=150))
ft.bag_set_topics(*B.TOPICS)
for n in (1000, 167_000):  # a 4 KiB chunk (the call's overhead is all there is) and C3's batch
    w = evt2_words(n, rng)
    timed("decode_raw evt2 host->host", n, lambda: ft.decode_raw(0, FE.RAW_EVT2, w))
    timed("decode_raw evt2 host->device", n, lambda: ft.decode_raw(0, FE.RAW_EVT2, w, device=True)[0].free())
    timed("decode_triggers evt2", n, lambda: ft.decode_triggers(0, FE.RAW_EVT2, w))
    a = aedat_bytes(n, rng)
    timed("decode_aedat host->host", n, lambda: ft.decode_aedat(0, a))
    b = bag_bytes(n, rng)
    timed("decode_bag host->host", n, lambda: ft.decode_bag(b))
ft.close()
# decode and track, and the feed: C3's batch per camera, plain calls
ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=150))
wl, wr = evt2_words(167_000, rng), evt2_words(120_000, rng)
timed("track_raw evt2", 167_000, lambda: ft.track_raw(FE.RAW_EVT2, wl, wr, 0, True))
al, ar = aedat_bytes(167_000, rng), aedat_bytes(120_000, rng)
ft.reset()
timed("track_aedat", 167_000, lambda: ft.track_aedat(al, ar, 0))
ft.reset()
ft.feed_open(30.0)
small = evt2_words(1000, rng)
timed("feed_push_raw evt2 (no window)", 1000, lambda: ft.feed_push_raw(0, FE.RAW_EVT2, small))
ft.close()
