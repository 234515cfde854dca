"""Arc* on the device (k_arc_mark, k_arc_map, k_arc_ev, k_dedup) held to the oracle on the planted planes of
tests/arc_cases.py: rings with ties, arcs at every length and rotation, stamps one ulp apart, the pre-check and the
border limit at their comparisons' edges, events outside the sensor, batches around the block size, the flag bytes and
the bitmap from call to call, and the selection with the per-pixel first-candidate map over its epoch wrap.  Everything
is equality: no tolerance.  tests/test_arc_cases.py shows that the cases reach the edges they are for."""
import numpy as np
import pytest

from esvio_amd import frontend as FE

import arc_cases as AC

pytestmark = pytest.mark.gpu

DEDUP_OPTIONS = ("ESVIO_FE_DEDUP", "ESVIO_FE_NO_DEDUP")
DEDUP_MODES = {"default": {}, "dedup": {"ESVIO_FE_DEDUP": "1"}, "no_dedup": {"ESVIO_FE_NO_DEDUP": "1"}}


def _setenv(monkeypatch, env):
    for o in DEDUP_OPTIONS:
        monkeypatch.delenv(o, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _pair(oracle, W, H, **kw):
    """a handle and an oracle detector of one configuration"""
    cfg = dict(dict(min_dist=AC.MIN_DIST, max_cnt=300), **kw)
    ft = FE.FeatureTracker(FE.make_config(W, H, **cfg))
    det = oracle.Detector(W, H, min_dist=cfg["min_dist"], filter_threshold=cfg.get("feature_filter_threshold", 0.01),
                          decay_ms=1000 * AC.DECAY_S)
    return ft, det


def _plant(ft, det, L0, L1, S0, S1):
    ft.detector.set_sae(0, L0, L1, S0, S1)
    det.set_sae(0, L0, L1, S0, S1)


def _same_flags(got, want, ev, tag):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d flags differ; first (event, x, y, polarity, got, want): %s" % (
        tag, bad.size, len(want), [(int(i), int(ev["x"][i]), int(ev["y"][i]), int(ev["polarity"][i]), int(got[i]),
                                    int(want[i])) for i in bad[:6]])


# ------------------------------------------------------------------ 1. ring families
@pytest.mark.parametrize("name,W,H", [(f, W, H) for f in AC.FAMILIES for W, H in AC.family_sizes(f)])
def test_ring_families(oracle, monkeypatch, name, W, H):
    """the N = 16 rings of the family on the polarity-1 plane, its N = 20 rings on the polarity-0 plane"""
    _setenv(monkeypatch, {})
    ft, det = _pair(oracle, W, H)
    try:
        n_corner = 0
        for k, page in enumerate(AC.family_pages(name, W, H)):
            _plant(ft, det, *page[:4])
            got, want = ft.detector.isCorner(page.events), det.corner_flags(page.events)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s %dx%d page %d: %d of %d flags differ\n%s" % (
                name, W, H, k, bad.size, len(want),
                "\n".join(AC.describe(page, int(i), int(got[i]), int(want[i])) for i in bad[:4]))
            n_corner += int(want.sum())
        assert n_corner > 0 or name in ("perm", "ternary")
    finally:
        ft.close()


# ------------------------------------------------------------------ 2. pre-check, border and event tables
@pytest.mark.parametrize("thr", AC.THRESHOLDS)
def test_precheck(oracle, monkeypatch, thr):
    _setenv(monkeypatch, {})
    ft, det = _pair(oracle, AC.PRE_W, AC.PRE_H, feature_filter_threshold=thr)
    try:
        L0, L1, S0, S1, evs = AC.precheck_planes(thr)
        _plant(ft, det, L0, L1, S0, S1)
        for which in ("own", "other", "both", "own"):
            _same_flags(ft.detector.isCorner(evs[which]), det.corner_flags(evs[which]), evs[which],
                        "pre-check thr %r, events of %s" % (thr, which))
    finally:
        ft.close()


@pytest.mark.parametrize("min_dist", AC.BORDER_MIN_DISTS)
def test_border(oracle, monkeypatch, min_dist):
    _setenv(monkeypatch, {})
    ft, det = _pair(oracle, AC.BORDER_W, AC.BORDER_H, min_dist=min_dist)
    try:
        L0, L1, S0, S1, ev = AC.border_planes(min_dist)
        _plant(ft, det, L0, L1, S0, S1)
        _same_flags(ft.detector.isCorner(ev), det.corner_flags(ev), ev, "border min_dist %d" % min_dist)
    finally:
        ft.close()


def test_event_batches(oracle, monkeypatch):
    """records outside the sensor, one pixel over more than three blocks, batch sizes around the block, a permutation"""
    _setenv(monkeypatch, {})
    ft, det = _pair(oracle, AC.EV_W, AC.EV_H)
    try:
        page = AC.event_page()
        _plant(ft, det, *page[:4])
        full = det.corner_flags(page.events)
        ev = AC.outside_events(page)
        _same_flags(ft.detector.isCorner(ev), det.corner_flags(ev), ev, "records outside the sensor")
        ev = AC.repeated_pixel_events(page)
        _same_flags(ft.detector.isCorner(ev), det.corner_flags(ev), ev, "one pixel repeated")
        for n in AC.BATCH_SIZES:
            for start in (0, 300):
                ev = page.events[start:start + n]
                _same_flags(ft.detector.isCorner(ev), full[start:start + n], ev, "n = %d from %d" % (n, start))
        order = np.random.default_rng(5).permutation(len(page.events))
        ev = page.events[order]
        got = ft.detector.isCorner(ev)
        _same_flags(got, full[order], ev, "the batch permuted")
        _same_flags(ft.detector.isCorner(page.events), full, page.events, "the batch in order")
    finally:
        ft.close()


# ------------------------------------------------------------------ 3. flag state between calls
def _halves(page):
    """two batches on disjoint pixels: the page's centres of even and of odd index"""
    idx = np.array([r[0] for r in page.rings])
    return page.events[idx % 2 == 0], page.events[idx % 2 == 1]


def _selection_args():
    L0, L1, S0, S1, ev, mask, t = AC.selection_case()
    return (L0, L1, S0, S1), ev, mask, t


def test_flag_state_between_calls(oracle, monkeypatch):
    """batch A, then batch B on other pixels, then B again: the flag bytes were consumed and the bitmap cleared; after a
    set_sae with other planes the same events follow the new planes"""
    _setenv(monkeypatch, {})
    W, H = AC.EV_W, AC.EV_H
    ft, det = _pair(oracle, W, H)
    try:
        page = AC.event_page()
        other = AC.family_pages("overlap", W, H)[0]
        A, B = _halves(page)
        _plant(ft, det, *page[:4])
        wantA, wantB = det.corner_flags(A), det.corner_flags(B)
        assert wantA.sum() > 50 and wantB.sum() > 50
        _same_flags(ft.detector.isCorner(A), wantA, A, "A")
        _same_flags(ft.detector.isCorner(B), wantB, B, "B after A")
        _same_flags(ft.detector.isCorner(B), wantB, B, "B again")
        _same_flags(ft.detector.isCorner(A), wantA, A, "A after B")
        _plant(ft, det, *other[:4])
        newB = det.corner_flags(B)
        assert (newB != wantB).sum() > 50  # (the new planes decide otherwise for many of the same events)
        _same_flags(ft.detector.isCorner(B), newB, B, "B after set_sae")
        _same_flags(ft.detector.isCorner(A), det.corner_flags(A), A, "A after set_sae")
    finally:
        ft.close()


def test_flag_state_with_selection_interleaved(oracle, monkeypatch):
    """Event_FeaturesToTrack and isCorner in turn on one handle, on batches of other pixels: neither leaves the other
    a flag byte, a bitmap bit or a candidate"""
    _setenv(monkeypatch, {})
    W, H = AC.SEL_W, AC.SEL_H
    ft, det = _pair(oracle, W, H, min_dist=AC.SEL_MIN_DIST)
    try:
        planes, ev, mask, t = _selection_args()
        _plant(ft, det, *planes)
        ts = ft.detector.SAEtoTimeSurface_left(t)
        assert np.array_equal(ts, det.time_surface(0, t))
        once = ev[:len(ev) // 2]  # (the first copy of the shuffled events)
        chequer = ((once["x"] - 4) // AC.GRID + (once["y"] - 4) // AC.GRID) % 2 == 0
        A, B = once[chequer], once[~chequer]  # disjoint pixels
        batches = {"A": A, "B": B}

        def expected():
            return {k: (det.corner_flags(b), det.features_to_track(b, 300, AC.SEL_MIN_DIST, mask, ts)) for k, b in batches.items()}

        def run(want, order, tag):
            for step, k in enumerate(order):
                flags, (xy, idx) = want[k]
                g_xy, g_idx = ft.Event_FeaturesToTrack(batches[k], 300, mask)
                assert np.array_equal(g_idx, idx) and np.array_equal(g_xy, xy), "%s: selection %s at step %d" % (tag, k, step)
                o = "B" if k == "A" else "A"
                _same_flags(ft.detector.isCorner(batches[o]), want[o][0], batches[o], "%s: isCorner %s at step %d" % (tag, o, step))
                _same_flags(ft.detector.isCorner(batches[k]), flags, batches[k], "%s: isCorner %s at step %d" % (tag, k, step))

        first = expected()
        assert all(len(first[k][1][1]) > 20 and first[k][0].sum() > 100 for k in batches)
        run(first, "ABBAB", "planted")
        # other planes under the same events: the overlap rings, the centres' own stamps kept
        other = AC.family_pages("overlap", W, H)[0]
        S0, S1 = other.S0.copy(), other.S1.copy()
        cy, cx = np.array(AC.centres(W, H)).T[::-1]
        S0[cy, cx], S1[cy, cx] = planes[2][cy, cx], planes[3][cy, cx]
        _plant(ft, det, other.L0, other.L1, S0, S1)
        ts = ft.detector.SAEtoTimeSurface_left(t)
        assert np.array_equal(ts, det.time_surface(0, t))
        second = expected()
        assert all((second[k][0] != first[k][0]).sum() > 50 and len(second[k][1][1]) > 5 for k in batches)
        run(second, "BAAB", "after set_sae")
    finally:
        ft.close()


# ------------------------------------------------------------------ 4. selection on planted planes
@pytest.mark.parametrize("max_cnt", [300, 600])
@pytest.mark.parametrize("mode", list(DEDUP_MODES))
def test_selection_on_planted_planes(oracle, monkeypatch, mode, max_cnt):
    """Event_FeaturesToTrack against the oracle with centres that render to TS_LK_THRESHOLD and next to it, a pre-blocked
    mask and every pixel's candidates twice, in different blocks; the per-pixel dedup as the handle decides (off at
    max_cnt 300, on at 600), forced on and forced off"""
    _setenv(monkeypatch, DEDUP_MODES[mode])  # (read when the handle is created)
    W, H = AC.SEL_W, AC.SEL_H
    ft, det = _pair(oracle, W, H, min_dist=AC.SEL_MIN_DIST, max_cnt=max_cnt)
    try:
        planes, ev, mask, t = _selection_args()
        _plant(ft, det, *planes)
        ts = ft.detector.SAEtoTimeSurface_left(t)
        assert np.array_equal(ts, det.time_surface(0, t))
        empty = np.zeros_like(mask)
        for m, tag in ((mask, "mask"), (empty, "no mask"), (None, "None")):
            for maxc in (1, 37, max_cnt):
                for batch, btag in ((ev, "twice"), (ev[:len(ev) // 2], "once"), (ev[:257], "257")):
                    xy, idx = det.features_to_track(batch, maxc, AC.SEL_MIN_DIST, empty if m is None else m, ts)
                    g_xy, g_idx = ft.Event_FeaturesToTrack(batch, maxc, m)
                    what = "%s, %s, maxCorners %d, batch %s" % (mode, tag, maxc, btag)
                    assert np.array_equal(g_idx, idx), "%s: indices %s..., want %s..." % (what, g_idx[:8], idx[:8])
                    assert np.array_equal(g_xy, xy), what
    finally:
        ft.close()


def test_first_candidate_map_over_its_epoch_wrap(oracle, monkeypatch):
    """dedup forced on, more than 2 x 254 selections on one handle, every one compared: the map's keys count down over 254
    launches, then it is cleared — twice here"""
    _setenv(monkeypatch, DEDUP_MODES["dedup"])
    W, H = AC.SEL_W, AC.SEL_H
    ft, det = _pair(oracle, W, H, min_dist=AC.SEL_MIN_DIST)
    try:
        planes, ev, mask, t = _selection_args()
        _plant(ft, det, *planes)
        ts = ft.detector.SAEtoTimeSurface_left(t)
        batches = AC.epoch_batches()
        want = [det.features_to_track(b, 300, AC.SEL_MIN_DIST, mask, ts) for b in batches]
        assert all(len(idx) > 10 for _, idx in want)
        for call in range(2 * 254 + 12):
            k = call % len(batches)
            g_xy, g_idx = ft.Event_FeaturesToTrack(batches[k], 300, mask)
            assert np.array_equal(g_idx, want[k][1]) and np.array_equal(g_xy, want[k][0]), "call %d, batch %d" % (call, k)
    finally:
        ft.close()
