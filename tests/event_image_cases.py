"""Designed inputs for the event images (include/esvio_fe.h "event images"): each takes the mark / emit kernels to one
edge — the emit's tail group, a contended pixel, stamps that disagree with stream order, events the SAE update skips, a
warp that moves the pixel.  tests/test_event_image_ref.py checks that each reaches the edge it is named for."""
import numpy as np

from esvio_amd.events import make_events

W, H = 43, 45            # 1935 pixels: no multiple of four, rows of 129 bytes
SMALL = (42, 42)         # the smallest handle
COUNTS = (0, 1, 255, 256, 257, 5000)  # around k_evimg_mark's 256-lane blocks, and many blocks
# k_evimg_mark takes its skipping form (the stream walked from its end) for more than one event per pixel of the cameras
# that have events: the counts on both sides of that threshold, for one camera and for two
THRESHOLD = ((W * H, 0), (W * H + 1, 0), (W * H, W * H), (W * H + 1, W * H))
T0_US = 5_000_000
HOT = (21, 22)           # the contended pixel


def uniform(n, seed, w=W, h=H, t0_us=T0_US, region=None):
    """n events, uniform over the sensor (or over region = (x0, y0, x1, y1), exclusive ends), strictly increasing stamps"""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = region if region else (0, 0, w, h)
    x, y = rng.integers(x0, x1, n), rng.integers(y0, y1, n)
    t = t0_us + np.arange(n, dtype=np.int64) * 3 + 1
    return make_events(x, y, t, rng.integers(0, 2, n))


def counts():
    """name -> (left, right): every count of COUNTS in both cameras, the two cameras' events unrelated"""
    return {"n%d" % n: (uniform(n, 100 + n), uniform(n, 200 + n)) for n in COUNTS}


def contention(last_on):
    """5000 events on ONE pixel, polarity alternating, the last one ON or OFF"""
    n = 5000
    pol = (np.arange(n) + (n - 1) + (1 if last_on else 0)) % 2
    return make_events(np.full(n, HOT[0]), np.full(n, HOT[1]), T0_US + np.arange(n, dtype=np.int64), pol)


def stamps():
    """name -> events: one set of (x, y, polarity) on an 8 x 8 patch — every pixel is hit many times, by both polarities —
    under stamps that are all equal, strictly decreasing, and stepping back a second half way"""
    base = uniform(2000, 7, region=(10, 10, 18, 18))
    n = len(base)
    out = {}
    t = {"equal": np.full(n, T0_US, np.int64),
         "decreasing": T0_US + (n - np.arange(n, dtype=np.int64)) * 5,
         "step_back": T0_US + np.arange(n, dtype=np.int64) * 7 - np.where(np.arange(n) >= n // 2, 1_000_000, 0)}
    for name, tt in t.items():
        out[name] = make_events(base["x"], base["y"], tt, base["polarity"])
    return out


def corners(w=W, h=H):
    """the four corner pixels, one event each, polarities mixed (one with the polarity byte 255: non-zero is ON)"""
    ev = make_events([0, w - 1, 0, w - 1], [0, 0, h - 1, h - 1], T0_US + np.arange(4), [1, 0, 0, 1])
    ev["polarity"][3] = 255
    return ev


def last_pixel(w=W, h=H):
    """one event on the last pixel alone: the emit's tail group, where the padded planes end"""
    return make_events([w - 1], [h - 1], [T0_US], [0])


def out_of_sensor(w=W, h=H):
    """events at x = W, y = H and 65535 between in-sensor ones: they write nothing, not even where x or y alone fits"""
    x = [3, w, 5, 65535, 7, 2, w - 1, 65535]
    y = [4, 4, h, 6, 65535, 9, h, 65535]
    return make_events(x, y, T0_US + np.arange(8), [1, 1, 1, 0, 0, 0, 1, 1])


# ---- motion compensation: |accel| > 5 and an omega large enough that most events land on another pixel
MC = dict(v=(0.05, -0.02, 0.01), v_pre=(0.04, -0.01, 0.0), accel=(0.3, -0.2, 9.8), omega=(4.0, -3.0, 12.0),
          fx=0.9 * W, fy=0.9 * W, cx=W / 2.0, cy=H / 2.0)
MC_SPAN_US = 20_000


def mc_batch(n=2000, seed=31):
    """(left, right, t1): both cameras' events spread over 20 ms, the header stamp just behind the last one (so that
    every event takes the warp's branch), one out-of-sensor event in each camera.  2 x 2000 events are more than one per
    pixel (the mark kernel's skipping form), their first 2 x 1000 are not."""
    out = []
    for cam in range(2):
        rng = np.random.default_rng(seed + cam)
        t = T0_US + np.sort(rng.choice(MC_SPAN_US, n, replace=False)).astype(np.int64)
        if cam == 0:
            t[0] = T0_US  # t_0 is the first LEFT event's stamp
        ev = make_events(rng.integers(0, W, n), rng.integers(0, H, n), t, rng.integers(0, 2, n))
        ev["x"][n // 2] = W  # skipped by the update
        out.append(ev)
    return out[0], out[1], (T0_US + MC_SPAN_US + 500) * 1e-6


def oracle_pixels(O, ev, first_left, motion, cam, w=W, h=H):
    """Where the oracle's motion-compensated update writes each event: the events go one at a time (their stamps are
    unique) into ONE fresh oracle.Detector's create_sae_mc, and event i's pixel is where sae_latest[polarity] equals its
    stamp afterwards; (-1, -1) for an event that left no such pixel (dropped)."""
    from esvio_amd.events import event_times
    t = event_times(ev)
    assert len(np.unique(t)) == len(t)
    det = O.Detector(w, h)
    px = np.full((len(ev), 2), -1, np.int64)
    for i in range(len(ev)):
        det.create_sae_mc(cam, ev[i:i + 1], first_left, motion)
        latest = det.get_sae(cam)[1 if ev["polarity"][i] else 0]
        hit = np.argwhere(latest == t[i])
        assert len(hit) <= 1
        if len(hit):
            px[i] = (hit[0][1], hit[0][0])
    return px


_mc_cache = {}


def mc_case(O):
    """(left, right, t1, oracle motion, left pixels, right pixels) of mc_batch(), computed once per process"""
    if "v" not in _mc_cache:
        L, R, t1 = mc_batch()
        m = O.make_motion(t1, MC["v"], MC["v_pre"], MC["accel"], MC["omega"], MC["fx"], MC["fy"], MC["cx"], MC["cy"])
        _mc_cache["v"] = (L, R, t1, m, oracle_pixels(O, L, L[:1], m, 0), oracle_pixels(O, R, L[:1], m, 1))
    return _mc_cache["v"]
