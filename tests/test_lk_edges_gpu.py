"""calcOpticalFlowPyrLK on the device against the oracle, bit for bit, on the inputs of tests/lk_cases.py: re-staged
tiles, windows at the image's limits, every exit of the iteration, |delta|^2 within an ulp of eps^2, sums at the top of
their range, blocks with idle waves, small and odd images — in both modes of the sums (lk_accum 2: k_lk_f32, 1: k_lk).
tests/test_lk_cases.py shows (without a GPU) that the inputs reach those places."""
import numpy as np
import pytest

from esvio_amd import frontend as FE
from test_parity_gpu import _compare_tracks

import lk_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[2, 1])
def handle(request):
    ft = FE.FeatureTracker(FE.make_config(LC.LARGEST[0], LC.LARGEST[1], lk_accum=request.param, max_cnt=LC.MAX_POINTS))
    yield ft, request.param
    ft.close()


def _check(oracle, ft, accum, c):
    g_pts, g_st = ft.calcOpticalFlowPyrLK(c.prev, c.next, c.pts, c.init, maxLevel=c.max_level, max_count=c.max_count,
                                          eps=c.eps, flags=c.flags)
    c_pts, c_st, t = oracle.lk_trace(c.prev, c.next, c.pts, c.init, max_level=c.max_level, max_count=c.max_count,
                                     eps=c.eps, flags=c.flags, accum=accum)
    bad = np.nonzero((g_st != c_st) | (g_pts.view(np.uint32) != c_pts.view(np.uint32)).any(1))[0]
    if len(bad):
        for i in bad[:8]:
            print("%s accum %d point %d %s: device %s st %d, oracle %s st %d; per level (exit, iterations): %s" % (
                c.name, accum, i, c.pts[i], g_pts[i], g_st[i], c_pts[i], c_st[i],
                [(L, t.exit_name(i, L), int(t.iters[i, L])) for L in range(3, -1, -1) if t.exit[i, L] >= 0]))
    assert not len(bad), "%s accum %d: %d of %d points differ (first: %d)" % (c.name, accum, len(bad), len(c.pts), bad[0])


@pytest.mark.parametrize("cls", ["restage", "borders", "termination", "saturated", "sizes"])
def test_lk_edge_class(oracle, handle, cls):
    ft, accum = handle
    cases = [c for c in LC.all_cases_without_oracle() if c.name.startswith(cls + "/")]
    assert cases
    for c in cases:
        _check(oracle, ft, accum, c)


def test_lk_tiebreak(oracle, handle):
    ft, accum = handle
    for c, _, _, _, _ in LC.tiebreak_cases(oracle, accum):
        _check(oracle, ft, accum, c)


@pytest.mark.parametrize("lk_accum", [2, 1])
def test_lk_counts(oracle, lk_accum):
    """blocks whose last waves have no point, on a handle made for 12 points; a thirteenth is refused and the handle
    goes on working"""
    ft = FE.FeatureTracker(FE.make_config(96, 80, lk_accum=lk_accum, max_cnt=LC.COUNTS_MAX_CNT))
    cases, too_many = LC.counts_cases()
    for c in cases[:5]:
        _check(oracle, ft, lk_accum, c)
    with pytest.raises(FE.FrontendError, match="rc=-1"):  # ESVIO_FE_EINVAL
        ft.calcOpticalFlowPyrLK(too_many.prev, too_many.next, too_many.pts, None, maxLevel=too_many.max_level)
    for c in cases:
        _check(oracle, ft, lk_accum, c)
    ft.close()


@pytest.mark.parametrize("lk_accum", [2, 1])
@pytest.mark.parametrize("kind", ["blocks", "noise"])
def test_track_image_on_saturated_frames(oracle, kind, lk_accum):
    """the fused forward / backward pair launch of trackImage on 0 / 255 data"""
    kw = dict(lk_accum=lk_accum, **LC.SEQUENCE_CONFIG)
    ft = FE.FeatureTracker(FE.make_config(160, 120, **kw))
    tr = oracle.Tracker(oracle.make_config(160, 120, **kw))
    for f, img in enumerate(LC.saturated_sequence(kind)):
        t = 0.05 * (f + 1)
        ft.trackImage(t, img, None, True)
        _compare_tracks(ft, tr.track_image(t, img, None, True), ("saturated sequence", kind, lk_accum, f))
    assert (ft.track_cnt >= 3).sum() >= 20
    ft.close()
