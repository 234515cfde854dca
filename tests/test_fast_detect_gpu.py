"""GPU: ESVIO_FE_DETECT_FAST — esvio_fe_set_detector, esvio_fe_features_to_track_fast and trackEvent with FAST
candidates (k_fast_score<10> + k_fast_collect + k_compact + k_fast_keys + one k_radix_pass, then the selection kernels
unchanged) — against the numpy restatement tests/fast_select_ref.py of the definition in include/esvio_fe.h.
Integers and positions that are integers: every comparison is equality, element for element and in order."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import fast_select_ref as R
from esvio_amd import frontend as FE
from esvio_amd.events import event_times
from esvio_amd.synth import SceneStream
from test_fast_gpu import DeviceImage

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEMBERS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
LEFT = MEMBERS[:5]

# ---- 1. the stage tap against the restatement ---------------------------------------------------------------------
TAP_MAX_CNT = 6000  # above every image's candidate count + 1 (5330 at barrier 0 on the 346 x 260 time surface)
BARRIERS, MIN_DISTS = (0, 20, 60), (3, 10, 30, 63)
# non-max survivors at barriers 0 / 20 / 60, worked out with the restatement when the test was written.  grid301:
# 2301 / 2301 / 1862 — beyond one 256-entry compaction block and one 2048-pair radix-sort tile; ts346: several of each
N_CANDIDATES = {"edges": (2, 2, 2), "plateaus": (1, 1, 1), "constant": (0, 0, 0), "blocks": (102, 83, 56),
                "ts346": (5330, 3322, 1646), "flat": (0, 0, 0), "blob": (1, 1, 1), "grid": (48, 48, 48),
                "grid301": (2301, 2301, 1862)}


def _tap_images():
    out = {}
    z = np.load(os.path.join(GOLDEN, "fast_ref_small.npz"))
    for n in map(str, z["names"]):
        if min(z[n + "_img"].shape) >= 42:  # (the 7 x 7 / 6 x 9 images are below the smallest handle)
            out[n] = z[n + "_img"]
    out["ts346"] = np.load(os.path.join(GOLDEN, "fast_ref_ts_346x260.npz"))["ts346_img"]
    out["flat"] = np.full((48, 64), 90, np.uint8)
    out["blob"] = np.zeros((48, 64), np.uint8)
    out["blob"][20:23, 30:33] = 200
    out["blob"][21, 31] = 255
    g = np.zeros((48, 64), np.uint8)  # identical single-pixel blobs, 7 apart: equal scores everywhere
    g[5:44:7, 5:60:7] = 180
    out["grid"] = g
    rng = np.random.default_rng(3)  # ... and blobs of seeded heights, 5 apart, at a size no tile divides
    g = np.zeros((203, 301), np.uint8)
    ys, xs = np.mgrid[4:199:5, 4:297:5]
    g[ys, xs] = rng.integers(30, 200, ys.shape)
    out["grid301"] = g
    return out


def _tap_masks(shape, rng):
    H, W = shape
    discs = np.zeros(shape, np.uint8)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(6):
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(3, max(H // 5, 4))
        discs[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255
    discs[rng.random(shape) < 0.05] = 200  # (any value but 255 blocks nothing)
    return {"none": None, "discs": discs, "all": np.full(shape, 255, np.uint8)}


@pytest.mark.parametrize("name", sorted(N_CANDIDATES))
def test_stage_tap_equals_restatement(name):
    """positions, scores, n_out and n_candidates for every barrier x mask x max_corners x min_dist row, the image in
    host and in device memory by turns.  Where an image has two candidates or more, some rows are cut by max_corners
    and some are not (checked below, and on the CPU when the rows were chosen)."""
    img = _tap_images()[name]
    H, W = img.shape
    masks = _tap_masks(img.shape, np.random.default_rng(W * 7 + H))
    cands = {b: R.candidates(img, b) for b in BARRIERS}
    assert tuple(len(cands[b][0]) for b in BARRIERS) == N_CANDIDATES[name]
    dev = DeviceImage(img)
    n_cut = n_uncut = n_rows = 0
    for md in MIN_DISTS:
        ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=TAP_MAX_CNT, min_dist=md))
        for b, (mname, mask) in itertools.product(BARRIERS, masks.items()):
            nc = len(cands[b][0])
            for mc in sorted({1, 7, nc - 1, nc + 1, TAP_MAX_CNT}):
                if mc < 1:
                    continue
                wxy, wsc, wn = R.select(img, b, mc, md, mask, cand=cands[b])
                arg = img if n_rows % 2 else dev.ptr.value
                gxy, gsc, gn = ft.features_to_track_fast(arg, barrier=b, maxCorners=mc, mask=mask, want_count=True)
                tag = (name, "min_dist", md, "barrier", b, "mask", mname, "max_corners", mc)
                assert gn == wn == nc, tag + (gn, wn)
                assert len(gxy) == len(wxy), tag + (len(gxy), len(wxy))
                assert gxy.dtype == np.float32 and np.array_equal(gxy, wxy), tag
                assert gsc.dtype == np.int32 and np.array_equal(gsc, wsc), tag
                more = len(R.select(img, b, mc + 1, md, mask, cand=cands[b])[0]) > len(wxy)
                n_cut += more
                n_uncut += not more
                n_rows += 1
        ft.close()
    dev.free()
    print(name, img.shape, "rows", n_rows, "cut by max_corners", n_cut, "not cut", n_uncut)
    assert n_uncut > 0 and (n_cut > 0 or max(N_CANDIDATES[name]) < 2)


def test_list_pass_counts_big_small_big_on_one_handle():
    """the list pass sorts in scratch of the detector's own (fastc[].hist), its launch sized for the sensor's bound and
    the count read on the device: k_fast_keys clears the look-back words, a memset the histograms and the ticket.  On
    one handle the time surface at barrier 0 (5330 candidates: three sort tiles), at 60 (1646: one), a constant image
    (none), and barrier 0 again; positions and scores as the restatement's, in order.  One digit width (1 x 8 bits) and
    one launch size per handle: neither can change within one."""
    img = _tap_images()["ts346"]
    H, W = img.shape
    flat = np.full_like(img, 90)
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=TAP_MAX_CNT, min_dist=3))
    try:
        for k, (im, b) in enumerate([(img, 0), (img, 60), (img, 0), (flat, 20), (img, 0), (img, 60)]):
            wxy, wsc, wn = R.select(im, b, TAP_MAX_CNT, 3, None)
            gxy, gsc, gn = ft.features_to_track_fast(im, barrier=b, maxCorners=TAP_MAX_CNT, mask=None, want_count=True)
            assert gn == wn == (0 if im is flat else N_CANDIDATES["ts346"][BARRIERS.index(b)]), (k, gn, wn)
            assert np.array_equal(gxy, wxy) and np.array_equal(gsc, wsc), (k, b)
    finally:
        ft.close()


def test_tap_rejects_bad_arguments_and_needs_no_detector_setting():
    ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=50))
    hd, L = ft._hd, ft._hd.L
    img = _tap_images()["grid"]
    xy, sc, n = np.zeros((64, 2), np.float32), np.zeros(64, np.int32), C.c_int32(-1)

    def call(barrier=20, mc=10, space=FE.HOST, out=xy, n_out=n):
        return L.esvio_fe_features_to_track_fast(hd.h, img.ctypes.data_as(C.c_void_p), space, barrier, mc, None,
                                                 out.ctypes.data_as(C.c_void_p) if out is not None else None,
                                                 sc.ctypes.data_as(C.c_void_p), C.byref(n_out) if n_out is not None else None,
                                                 None)

    assert call() == 0 and n.value == 10  # (the detector is still Arc*: the tap does not depend on it)
    assert call(mc=0) == 0 and n.value == 0 and call(mc=-3) == 0 and n.value == 0
    for kw in (dict(barrier=-1), dict(barrier=256), dict(space=5), dict(mc=51)):
        assert call(**kw) == -1 and L.esvio_fe_last_error(hd.h), kw  # ESVIO_FE_EINVAL
    assert call(out=None) == -1 and call(n_out=None) == -1
    ft.close()


# ---- 2. img == NULL ----------------------------------------------------------------------------------------------
def test_tap_reads_the_handles_time_surface_in_place():
    W, H = 346, 260
    Lb, Rb, _ = SceneStream(W, H, rate=2e6, seed=9).next_batch()
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=150))
    ft.detector.createSAE_stereo(Lb, Rb)
    t = event_times(Lb)[-1]
    ft.detector.SAEtoTimeSurface_right(t)
    ts = ft.detector.SAEtoTimeSurface_left(t)
    assert np.array_equal(ft.gettimesurface(0), ts)
    want = R.select(ts, 20, 150, 10)
    assert len(want[0]) == 150 and want[2] > 1000
    dev = DeviceImage(ts)
    for arg in (None, ts, dev.ptr.value):
        gxy, gsc, gn = ft.features_to_track_fast(arg, barrier=20, maxCorners=150, want_count=True)
        assert np.array_equal(gxy, want[0]) and np.array_equal(gsc, want[1]) and gn == want[2], type(arg)
    dev.free()
    ft.close()


# ---- 3. - 6. trackEvent ---------------------------------------------------------------------------------------------
W, H, FRAMES, MAX_CNT, MIN_DIST = 192, 144, 12, 60, 10
PUBS = [f % 2 == 0 for f in range(FRAMES)]
# chosen on the CPU: the first published frame has no kept points, so its new corners are a function of the oracle's
# rendered left time surface alone — 1491 FAST candidates and 60 corners (the whole budget) at this barrier
BARRIER = 20
CFG = dict(max_cnt=MAX_CNT, min_dist=MIN_DIST, equalize=0, median_blur_kernel_size=0)


@pytest.fixture(scope="module")
def scene():
    """the synth scene stream: per frame (time, left, right) in device memory, and the host arrays"""
    s = SceneStream(W, H, rate=1.5e6, seed=21)
    host = [s.next_batch()[:2] for _ in range(FRAMES)]
    bufs = [(FE.EventBuffer(Lb, FE.DEVICE), FE.EventBuffer(Rb, FE.DEVICE)) for Lb, Rb in host]
    yield [(event_times(Lb)[-1], bl.arg, br.arg) for (Lb, Rb), (bl, br) in zip(host, bufs)], host
    for bl, br in bufs:
        bl.free()
        br.free()


def _snapshot(ft, members=MEMBERS):
    return [getattr(ft, k).copy() for k in members]


def _tracker(detector=FE.DETECT_FAST, lk_accum=FE.DEFAULT_LK_ACCUM):
    ft = FE.FeatureTracker(FE.make_config(W, H, lk_accum=lk_accum, **CFG))
    if detector is not None:
        ft.set_detector(detector, BARRIER)
    return ft


_plain_runs = {}


def _plain(scene, lk_accum=FE.DEFAULT_LK_ACCUM):
    """plain calls, computed once per LK mode: per frame every result member, then the two time surfaces"""
    if lk_accum not in _plain_runs:
        ft = _tracker(lk_accum=lk_accum)
        out = []
        for f, (t, Lb, Rb) in enumerate(scene[0]):
            ft.trackEvent(t, Lb, Rb, PUBS[f])
            out.append(_snapshot(ft))
        out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
        ft.close()
        _plain_runs[lk_accum] = out
    return _plain_runs[lk_accum]


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (ra, rb) in enumerate(zip(got, want)):
        assert len(ra) == len(rb), (tag, f)
        for k, (va, vb) in enumerate(zip(ra, rb)):
            assert va.dtype == vb.dtype and va.shape == vb.shape, (tag, f, k, va.shape, vb.shape)
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), (tag, f, k)


@pytest.mark.parametrize("lk_accum", [2, 1])
def test_track_event_new_corners_equal_restatement(scene, lk_accum):
    """from the outputs alone: after a published call the entries with track_cnt >= 2 are Event_setMask's survivors,
    their discs the mask, max_cnt minus their number the budget, esvio_fe_get_time_surface(0) the image — the entries
    with track_cnt 1 must be the restatement's selection, in order.  In both LK modes: the selection does not care."""
    ft = _tracker(lk_accum=lk_accum)
    added, n_pub = 0, 0
    for f, (t, Lb, Rb) in enumerate(scene[0]):
        ft.trackEvent(t, Lb, Rb, PUBS[f])
        if not PUBS[f]:
            assert not np.any(ft.track_cnt == 1), f
            continue
        cnt, pts = ft.track_cnt, ft.cur_pts
        kept = cnt >= 2
        n_kept = int(kept.sum())
        assert np.all(kept[:n_kept]) and np.all(cnt[n_kept:] == 1), f  # (kept points first, new corners behind them)
        ts = ft.gettimesurface(0)
        want_xy, _, n_cand = R.select(ts, BARRIER, MAX_CNT - n_kept, MIN_DIST, R.kept_mask(ts.shape, pts[:n_kept], MIN_DIST))
        print("frame", f, "kept", n_kept, "FAST candidates", n_cand, "new", len(pts) - n_kept, "restatement", len(want_xy))
        assert np.array_equal(pts[n_kept:], want_xy), (f, n_kept, len(pts) - n_kept, len(want_xy))
        if f == 0:
            assert n_kept == 0 and len(want_xy) >= 20
        added += len(want_xy) > 0
        n_pub += 1
    assert n_pub == FRAMES // 2 and 2 * added >= n_pub, (added, n_pub)  # (an empty comparison cannot pass)
    # the stream is the one the plain reference run of the other tests tracks
    _same([_snapshot(ft)], [_plain(scene, lk_accum)[FRAMES - 1]], "last frame")
    ft.close()


def _announced(scene, finish_every_frame):
    """three batches announced ahead with exact hints, lazy returns, the launch thread"""
    frames = scene[0]
    ft = _tracker()
    ft.set_lazy_new_stereo(True)
    ft.set_launch_thread(True)
    out, announced = [], 0
    for f, (t, Lb, Rb) in enumerate(frames):
        while announced < min(f + 3, FRAMES - 1):
            announced += 1
            ta, La, Ra = frames[announced]
            ft.set_next_batch(ta, La, Ra, PUBS[announced])
        ft.trackEvent(t, Lb, Rb, PUBS[f])
        if finish_every_frame:
            ft.finish()
        out.append(_snapshot(ft, MEMBERS if finish_every_frame else LEFT))
    ft.finish()
    out.append(_snapshot(ft))
    out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    dc = ft.debug_counters()
    ft.close()
    return out, dc


def test_schedules_agree(scene):
    """plain calls; batches announced three ahead (exact pub hints, lazy new-corner stereo, the launch thread,
    esvio_fe_finish at the end); the motion-compensated overload with a zero esvio_fe_motion: every result member of
    every frame bit for bit, and no device-side wait expired"""
    a = _plain(scene)
    assert len(a[FRAMES - 1][0]) > 20 and len(a[FRAMES - 1][5]) > 5  # (tracks in both cameras)
    # (b) a lazily returned frame's right-camera members are completed by the next call or by finish: with finish only
    # at the end the left members of every frame and everything of the last are there to compare, with finish after
    # every frame everything is
    b, dc = _announced(scene, False)
    _same(b[:FRAMES], [r[:len(LEFT)] for r in a[:FRAMES]], "announced, left members")
    _same(b[FRAMES:], [a[FRAMES - 1], a[FRAMES]], "announced, after finish")
    assert dc["spec_redone"] == 0 and dc["chain_redone"] == 0, dc
    b, dc = _announced(scene, True)
    _same(b[:FRAMES], a[:FRAMES], "announced, finish after every frame")
    assert dc["spec_redone"] == 0 and dc["chain_redone"] == 0, dc
    # (c)
    ft = _tracker()
    c = []
    for f, (t, Lb, Rb) in enumerate(scene[0]):
        ft.trackEvent(t, Lb, Rb, PUBS[f], measurements=FE.Motion())
        c.append(_snapshot(ft))
    c.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    dc = ft.debug_counters()
    ft.close()
    _same(c, a, "motion-compensated overload, zero motion")
    assert dc["spec_redone"] == 0 and dc["chain_redone"] == 0, dc


def test_detector_scratch_is_its_own(scene):
    """plain calls with an esvio_fe_fast_corners call (arc 9, barrier 5) and a stage-tap call on a foreign image
    between every two of them: nothing changes"""
    foreign = _tap_images()["grid301"][:H, :W].copy()
    want_tap = R.select(foreign, 20, MAX_CNT, MIN_DIST)
    ft = _tracker()
    out = []
    for f, (t, Lb, Rb) in enumerate(scene[0]):
        ft.trackEvent(t, Lb, Rb, PUBS[f])
        out.append(_snapshot(ft))
        xy, _ = ft.fast_corners(arc=9, barrier=5, nonmax=False)
        assert len(xy) > 100
        gxy, gsc = ft.features_to_track_fast(foreign, barrier=20, maxCorners=MAX_CNT)
        assert np.array_equal(gxy, want_tap[0]) and np.array_equal(gsc, want_tap[1]) and len(gxy) > 20
    out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    ft.close()
    _same(out, _plain(scene), "fast_corners + tap between the calls")


def test_arc_is_untouched(scene):
    """a default handle and one told ESVIO_FE_DETECT_ARC give the same results (and not those of FAST)"""
    runs = []
    for det in (None, FE.DETECT_ARC):
        ft = _tracker(det)
        out = []
        for f, (t, Lb, Rb) in enumerate(scene[0][:6]):
            ft.trackEvent(t, Lb, Rb, PUBS[f])
            out.append(_snapshot(ft))
        ft.close()
        runs.append(out)
    _same(runs[1], runs[0], "ESVIO_FE_DETECT_ARC against the default")
    assert len(runs[0][0][0]) > 20
    assert not np.array_equal(runs[0][0][2], _plain(scene)[0][2])  # (frame 0's corners: Arc*'s are not FAST's)


def test_set_detector_validation(scene):
    ft = FE.FeatureTracker(FE.make_config(W, H, **CFG))
    hd, L = ft._hd, ft._hd.L
    for det, bar in ((2, 20), (-1, 20), (FE.DETECT_FAST, -1), (FE.DETECT_FAST, 256)):
        assert L.esvio_fe_set_detector(hd.h, det, bar) == -1, (det, bar)  # ESVIO_FE_EINVAL
        assert b"set_detector" in L.esvio_fe_last_error(hd.h), (det, bar)
    assert L.esvio_fe_set_detector(hd.h, FE.DETECT_ARC, 999) == 0  # (the barrier is ignored for Arc*)
    t0, L0, R0 = scene[0][0]
    t1, L1, R1 = scene[0][1]
    ft.set_next_batch(t0, L0, R0, True)
    assert L.esvio_fe_set_detector(hd.h, FE.DETECT_FAST, BARRIER) == -1
    assert b"announced" in L.esvio_fe_last_error(hd.h)
    ft.trackEvent(t0, L0, R0, True)  # (tracked with Arc*: the refused call changed nothing)
    arc_pts = ft.cur_pts.copy()
    ft.set_detector(FE.DETECT_FAST, BARRIER)
    # the setting survives esvio_fe_reset: the first frame after it is the plain FAST run's first frame
    ft.reset()
    ft.trackEvent(t0, L0, R0, True)
    want = _plain(scene)[0]
    assert np.array_equal(ft.cur_pts, want[2]) and not np.array_equal(arc_pts, want[2])
    ft.close()
