"""goodFeaturesToTrack on the device (k_gftt_cov, k_gftt_rowsum, k_gftt_eig, k_gftt_collect, k_compact, k_gftt_sortprep,
four k_radix_pass, the Euclidean-disc selection) held to the oracle on the designed inputs of tests/gftt_cases.py: the
response map at the smallest handle and around the 64-lane, 4-row and 8-row blocks, with negative, exactly-zero and
border responses; candidate counts of 0, 1, 2 and around the 256-wide lists and the 2048-key radix tile; a threshold
that equals a candidate bit for bit; tie groups over many rows and more than three radix tiles; masks that move the
threshold, leave nothing, or sit on the bitmap's word edges; the sort's scratch shared with the SAE update; trackImage's
ids in tie order.  Everything is equality: the map as bits, the corners as arrays, so count and order are included.
tests/test_gftt_cases.py shows on the CPU that the cases reach the edges they are for."""
import numpy as np
import pytest

from esvio_amd import frontend as FE
from esvio_amd.synth import uniform_batch

import gftt_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's (corners, map) of a case, computed once per case"""
    done = {}

    def get(c):
        key = (c.name, c.img.shape, c.img.tobytes(), None if c.mask is None else c.mask.tobytes(), c.quality,
               c.min_distance, c.max_corners)
        if key not in done:
            done[key] = oracle.good_features_to_track(c.img, c.max_corners, c.quality, c.min_distance, c.mask, want_eig=True)
        return done[key]
    return get


@pytest.fixture(scope="module")
def cases(oracle):
    return GC.build(lambda img: oracle.good_features_to_track(img, 1, 0.01, 1, want_eig=True)[1])


def _handle(size, max_cnt):
    return FE.FeatureTracker(FE.make_config(size[0], size[1], max_cnt=max_cnt, min_dist=10))


def _describe(c, e, i):
    if i >= len(c):
        return "nothing"
    x, y = int(c[i, 0]), int(c[i, 1])
    return "(%d, %d) response 0x%08x" % (x, y, int(e.view(np.uint32)[y, x]))


def check(ft, want, c, tag=""):
    """one call against the oracle: the response map as bits, the corners as an array"""
    got, eig = ft.goodFeaturesToTrack(c.img, c.max_corners, c.quality, c.min_distance, c.mask, want_eig=True)
    exp, exp_eig = want(c)
    name = "%s%s" % (c.name, tag and " [%s]" % tag)
    bad = np.argwhere(eig.view(np.uint32) != exp_eig.view(np.uint32))
    assert bad.size == 0, "%s: the response differs at %d pixels; first (x, y) = (%d, %d): 0x%08x, the oracle's 0x%08x" % (
        name, len(bad), bad[0][1], bad[0][0], eig.view(np.uint32)[tuple(bad[0])], exp_eig.view(np.uint32)[tuple(bad[0])])
    if got.shape != exp.shape or not np.array_equal(got, exp):
        n = min(len(got), len(exp))
        diff = np.flatnonzero((got[:n] != exp[:n]).any(1))
        i = int(diff[0]) if diff.size else n
        raise AssertionError("%s: %d corners, the oracle's %d; first difference at index %d: %s, the oracle's %s" % (
            name, len(got), len(exp), i, _describe(got, eig, i), _describe(exp, exp_eig, i)))
    return got


# ------------------------------------------------------------------ a. response map
@pytest.mark.parametrize("W,H", GC.RESPONSE_SIZES)
def test_response_map(want, cases, W, H):
    """every image of the size in sequence on one handle, then the first one again"""
    lst = cases["response"][(W, H)]
    assert len(lst) == len(GC.RESPONSE_KINDS)
    ft = _handle((W, H), GC.RESPONSE_MAX_CNT)
    try:
        for c in lst + lst[:1]:
            check(ft, want, c)
    finally:
        ft.close()


# ------------------------------------------------------------------ b. counts, threshold
def test_counts_and_threshold(want, cases):
    """n = 0 (three ways) and n = 1 first on a fresh handle, the counts upwards, n = 0 and n = 1 again right after 2049
    — the lists shrink from call to call —, the threshold on a candidate and one double below, the counts downwards"""
    count, thr = cases["count"], cases["threshold"]
    assert len(count) == len(GC.COUNT_NAMES) and len(thr) == len(GC.THRESHOLD_NAMES)
    by_n = dict(zip([0, "q2", "const"] + list(GC.COUNT_NS), count))
    ft = _handle(GC.COUNT_SIZE, GC.COUNT_MAX_CNT)
    try:
        for k, c in enumerate(count):
            assert len(check(ft, want, c, "upwards")) == ([0, 0, 0] + list(GC.COUNT_NS))[k]
        for key in (0, 2049, 1, 2049, "const", 2049, "q2", 2048, 1, 0, 2049, 1):
            check(ft, want, by_n[key], "after 2049")
        assert len(check(ft, want, thr[0])) == GC.THRESHOLD_K and len(check(ft, want, thr[1])) == GC.THRESHOLD_K + 1
        check(ft, want, thr[0], "again")
        for c in count[::-1]:
            check(ft, want, c, "downwards")
    finally:
        ft.close()
    fresh = _handle(GC.COUNT_SIZE, GC.COUNT_MAX_CNT)  # n = 1 as a handle's first call: nothing sorted before
    try:
        assert len(check(fresh, want, by_n[1], "first call")) == 1
        check(fresh, want, by_n[0], "second call")
    finally:
        fresh.close()


# ------------------------------------------------------------------ c. ties
@pytest.mark.parametrize("serial", [False, True])
def test_ties(want, cases, monkeypatch, serial):
    """value descending, then address descending, over tie groups that span rows and radix tiles; with
    ESVIO_FE_SELECT_SERIAL the one-wave selection takes the checker's and the tiled patch's lists"""
    if serial:
        monkeypatch.setenv("ESVIO_FE_SELECT_SERIAL", "1")  # (read when the handle is created)
    else:
        monkeypatch.delenv("ESVIO_FE_SELECT_SERIAL", raising=False)
    lst = cases["tie"]
    assert len(lst) == GC.N_TIE_CASES
    if serial:
        lst = [c for c in lst if c.name.split()[0] in ("checker", "tiled")]
        assert len(lst) == 2 * GC.N_TIE_CASES // len(GC.TIE_KINDS)
    ft = _handle(GC.TIE_SIZE, GC.TIE_MAX_CNT)
    try:
        for c in lst:
            got = check(ft, want, c, "serial" if serial else "")
            assert len(got) > 100 or c.max_corners < GC.TIE_MAX_CNT
    finally:
        ft.close()


# ------------------------------------------------------------------ d. masks
def _mask_sequence(ft, want, lst):
    """mask, None, mask per case — the unmasked call sees the last mask's bits in d_mask_bits — then everything
    masked and an unmasked call behind it, for a max_key left at zero"""
    for c in lst:
        check(ft, want, c, "mask")
        check(ft, want, c._replace(name=c.name + ", unmasked", mask=None), "None after a mask")
        check(ft, want, c, "mask again")
    c = lst[0]
    nothing = c._replace(name=c.name + ", all masked", mask=np.zeros_like(c.mask))
    assert len(check(ft, want, nothing)) == 0
    assert len(check(ft, want, c._replace(name=c.name + ", unmasked", mask=None), "after all masked")) > 0


def test_masks(want, cases):
    assert len(cases["mask"]) == len(GC.MASK_NAMES)
    ft = _handle(GC.MASK_SIZE, GC.MASK_MAX_CNT)
    try:
        _mask_sequence(ft, want, cases["mask"])
    finally:
        ft.close()


@pytest.mark.parametrize("W", GC.WORD_EDGE_WIDTHS)
def test_masks_on_the_bitmaps_word_edges(want, cases, W):
    lst = [c for c in cases["word_edge"] if c.img.shape[1] == W]
    assert len(lst) == len(GC.WORD_EDGE_COLUMNS)
    ft = _handle((W, GC.WORD_EDGE_H), GC.MASK_MAX_CNT)
    try:
        _mask_sequence(ft, want, lst)
    finally:
        ft.close()


def test_negative_maximum(want, cases):
    """only pixels with a negative response allowed: the maximum's key, the threshold and the corners' values are
    below zero; with several values among them the sort orders keys of negative floats"""
    lst = cases["negative_max"]
    assert len(lst) == len(GC.NEGATIVE_MAX_NAMES)
    ft = _handle(GC.TIE_SIZE, GC.MASK_MAX_CNT)
    try:
        _mask_sequence(ft, want, lst)
        assert len(check(ft, want, lst[1])) > 20 and len(check(ft, want, lst[2])) == 14
    finally:
        ft.close()


# ------------------------------------------------------------------ state shared with other stages
def test_sort_scratch_shared_with_the_sae_update(oracle, want, cases, monkeypatch):
    """gftt_run borrows the SAE update's histogram, keys and values and leaves the sort head as k_sae_apply does: the
    radix-sort form of the update and goodFeaturesToTrack on the checker in turn, two rounds, each after the other"""
    monkeypatch.setenv("ESVIO_FE_SAE_SORT", "1")  # (read when the handle is created)
    W, H = GC.TIE_SIZE
    checker = [c for c in cases["tie"] if c.name == "checker whole list"][0]
    dots = [c for c in cases["tie"] if c.name == "dots whole list"][0]
    rng = np.random.default_rng(21)
    ft = _handle(GC.TIE_SIZE, GC.TIE_MAX_CNT)
    det = oracle.Detector(W, H)
    try:
        t0 = 1_700_000_000_000_000
        for k in range(2):
            L = uniform_batch(W, H, 3000 + 2500 * k, t0 + k * 33333, 33333, rng)
            R = uniform_batch(W, H, 1500 + 2500 * k, t0 + k * 33333, 33333, rng)
            assert ft.detector.createSAE_stereo(L, R) == 0
            det.create_sae(0, L)
            det.create_sae(1, R)
            for cam in (0, 1):
                for name, a, b in zip(("L0", "L1", "S0", "S1"), ft.detector.get_sae(cam), det.get_sae(cam)):
                    assert np.array_equal(a, b), "round %d, camera %d: plane %s differs at %d pixels" % (k, cam, name, (a != b).sum())
            assert len(check(ft, want, checker, "round %d" % k)) >= 3 * 2048
            assert 1 < len(check(ft, want, dots, "round %d" % k)) <= 2048   # (three sort tiles and more, one tile, and again)
    finally:
        ft.close()


def test_sae_gftt_and_fast_in_turn_on_one_handle(oracle, want, monkeypatch):
    """The radix-sort form of the SAE update and goodFeaturesToTrack sort in the handle's one scratch (hist, keys, vals);
    each leaves the histograms and tickets clear for whoever comes next and clears the look-back words of its OWN tile
    count and digit width (3 x 6 bits against 4 x 8) itself.  The FAST list pass sorts in scratch of the detector's own
    and runs between them.  One handle: SAE big, goodFeaturesToTrack, FAST, SAE small, FAST, goodFeaturesToTrack, SAE
    big — planes as the oracle's, corners as the oracle's, FAST corners as tests/fast_select_ref.py's, at every step."""
    import os

    import fast_select_ref as FR
    monkeypatch.setenv("ESVIO_FE_SAE_SORT", "1")
    ts = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_ref_ts_346x260.npz"))["ts346_img"]
    H, W = ts.shape
    many = GC.Case("noise", GC.mask_noise(W, H), None, 0.01, 3, 3000)
    few = GC.Case("sparse dots", GC.dot_lattice(W, H, pitch=24), None, 0.01, 3, 3000)
    rng = np.random.default_rng(23)
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=6000, min_dist=3))
    det = oracle.Detector(W, H)
    t0, step = 1_700_000_000_000_000, [0]

    def sae(nL, nR):
        L = uniform_batch(W, H, nL, t0 + step[0] * 33333, 33333, rng)
        R = uniform_batch(W, H, nR, t0 + step[0] * 33333, 33333, rng)
        step[0] += 1
        assert ft.detector.createSAE_stereo(L, R) == 0
        det.create_sae(0, L)
        det.create_sae(1, R)
        for cam in (0, 1):
            for name, a, b in zip(("L0", "L1", "S0", "S1"), ft.detector.get_sae(cam), det.get_sae(cam)):
                assert np.array_equal(a, b), "step %d, camera %d: plane %s differs at %d pixels" % (step[0], cam, name, (a != b).sum())

    def fast(barrier, n_tiles):
        wxy, wsc, wn = FR.select(ts, barrier, 6000, 3, None)
        gxy, gsc, gn = ft.features_to_track_fast(ts, barrier=barrier, maxCorners=6000, mask=None, want_count=True)
        assert gn == wn and (wn + 2047) // 2048 == n_tiles, (barrier, gn, wn)
        assert np.array_equal(gxy, wxy) and np.array_equal(gsc, wsc), barrier

    try:
        sae(7000, 4100)
        n_many = len(oracle.good_features_to_track(many.img, 1 << 20, 0.01, 1, None))
        assert n_many > 2 * 2048   # (the whole list, before the distance rule: what the sort is given; 5955)
        check(ft, want, many, "behind the big update")
        fast(0, 3)
        sae(300, 0)
        fast(60, 1)
        assert 1 < len(check(ft, want, few, "behind the small update")) <= 2048
        sae(7000, 4100)
        check(ft, want, many, "again")
    finally:
        ft.close()


def _compare_tracks(ft, r, tag):
    assert np.array_equal(ft.ids, r.ids) and np.array_equal(ft.track_cnt, r.track_cnt), tag
    assert np.array_equal(ft.ids_right, r.ids_right), tag
    for k in ("cur_pts", "cur_un_pts", "pts_velocity", "cur_right_pts", "cur_un_right_pts", "right_pts_velocity"):
        a, b = getattr(ft, k), getattr(r, k)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, k)


def test_track_image_ids_follow_the_tie_order(oracle):
    """trackImage on the square lattice, whose corners all have one response, then on a copy shifted by one pixel: the
    first frame's ids are handed out in the tie order, the second frame tracks them and fills up from the same list"""
    W, H = GC.TIE_SIZE
    kw = dict(max_cnt=60, min_dist=5, flow_back=1)
    frames = [(GC.square_lattice(W, H), GC.square_lattice(W, H, shift=2)), (GC.square_lattice(W, H, shift=1), GC.square_lattice(W, H, shift=3))]
    ft = FE.FeatureTracker(FE.make_config(W, H, **kw))
    tr = oracle.Tracker(oracle.make_config(W, H, **kw))
    try:
        for f, (L, R) in enumerate(frames):
            ft.trackImage(0.05 * (f + 1), L, R, True)
            _compare_tracks(ft, tr.track_image(0.05 * (f + 1), L, R, True), "frame %d" % f)
            if f == 0:  # the first 60 of the 108 tied corners: from the last row upwards, from right to left
                assert len(ft.ids) == 60 and ft.ids.tolist() == list(range(int(ft.ids[0]), int(ft.ids[0]) + 60))
                p = ft.cur_pts
                assert (np.diff(p[:, 1] * W + p[:, 0]) < 0).all()
        assert len(ft.ids) > 0
    finally:
        ft.close()
