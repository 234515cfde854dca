"""CPU: the restatement of ESVIO_FE_DETECT_FAST (tests/fast_select_ref.py) against answers worked out by hand, and the
two new C ABI symbols (exported, refusing a NULL handle before anything touches a device).

The hand-made images are single bright pixels on a black background.  For such a pixel of value v every ring byte is
0, so min over any 10 ring positions of (centre - ring) is v: it is a FAST-10 corner with score_10 = v - 1 at every
barrier below v.  A pixel that has the bright one ON its ring sees one brighter ring byte among sixteen (no run of
10), every other pixel sees a flat ring: the bright pixel is the image's only corner, and the non-max has nothing to
suppress.  The expected values below follow from that, not from the restatement."""
import ctypes as C

import numpy as np

import fast_select_ref as R
from esvio_amd import frontend as FE

W, H, MIN_DIST, BARRIER = 64, 48, 10, 20


def _img(*pixels):
    img = np.zeros((H, W), np.uint8)
    for x, y, v in pixels:
        img[y, x] = v
    return img


def _check(got, xy, score, n_cand):
    gxy, gsc, gn = got
    assert gxy.dtype == np.float32 and gsc.dtype == np.int32
    assert gxy.tolist() == [list(map(float, p)) for p in xy], gxy.tolist()
    assert gsc.tolist() == score and gn == n_cand


def test_higher_score_wins_although_later_in_raster_order():
    img = _img((20, 10, 100), (25, 12, 200))  # 5.4 pixels apart, min_dist 10
    _check(R.select(img, BARRIER, 60, MIN_DIST), [(25, 12)], [199], 2)
    # ... and with more room between them both are taken, the stronger one first
    img = _img((20, 10, 100), (25, 30, 200))
    _check(R.select(img, BARRIER, 60, MIN_DIST), [(25, 30), (20, 10)], [199, 99], 2)


def test_equal_scores_keep_raster_order():
    _check(R.select(_img((26, 10, 150), (20, 10, 150)), BARRIER, 60, MIN_DIST), [(20, 10)], [149], 2)
    # (y before x: the upper one wins although it lies further right)
    _check(R.select(_img((20, 14, 150), (24, 10, 150)), BARRIER, 60, MIN_DIST), [(24, 10)], [149], 2)
    # far apart: both, in raster order
    _check(R.select(_img((50, 30, 150), (10, 30, 150)), BARRIER, 60, MIN_DIST), [(10, 30), (50, 30)], [149, 149], 2)


def test_corner_on_a_blocked_pixel_is_skipped_and_blocks_nothing():
    img = _img((20, 10, 200), (26, 12, 100))
    mask = np.zeros((H, W), np.uint8)
    mask[10, 20] = 255
    _check(R.select(img, BARRIER, 60, MIN_DIST, mask), [(26, 12)], [99], 2)
    # a mask value other than 255 does not block
    mask[10, 20] = 254
    _check(R.select(img, BARRIER, 60, MIN_DIST, mask), [(20, 10)], [199], 2)


def test_corner_whose_centre_byte_is_the_threshold_is_skipped():
    img = _img((20, 10, 128), (26, 12, 100))
    _check(R.select(img, BARRIER, 60, MIN_DIST), [(26, 12)], [99], 2)
    _check(R.select(img, BARRIER, 60, MIN_DIST, ts_lk_threshold=100.0), [(20, 10)], [127], 2)


def test_cut_at_max_corners():
    img = _img((10, 40, 90), (50, 8, 250), (30, 24, 170))
    _check(R.select(img, BARRIER, 3, MIN_DIST), [(50, 8), (30, 24), (10, 40)], [249, 169, 89], 3)
    _check(R.select(img, BARRIER, 2, MIN_DIST), [(50, 8), (30, 24)], [249, 169], 3)
    _check(R.select(img, BARRIER, 1, MIN_DIST), [(50, 8)], [249], 3)
    _check(R.select(img, BARRIER, 0, MIN_DIST), [], [], 3)
    # the barrier takes the weakest out of C itself
    _check(R.select(img, 90, 3, MIN_DIST), [(50, 8), (30, 24)], [249, 169], 2)


def test_flat_image_has_no_corners():
    _check(R.select(np.full((H, W), 77, np.uint8), 0, 60, MIN_DIST), [], [], 0)


def test_the_disc_is_cv_circle_not_the_open_euclidean_one():
    # cv::circle(r = 3) holds (3, 0); goodFeaturesToTrack's distance test, dx*dx + dy*dy < 3*3, would let it pass
    _check(R.select(_img((20, 10, 200), (23, 10, 100)), BARRIER, 60, 3), [(20, 10)], [199], 2)
    _check(R.select(_img((20, 10, 200), (20, 13, 100)), BARRIER, 60, 3), [(20, 10)], [199], 2)
    # ... and not (3, 1) or (4, 0)
    _check(R.select(_img((20, 10, 200), (23, 11, 100)), BARRIER, 60, 3), [(20, 10), (23, 11)], [199, 99], 2)
    _check(R.select(_img((20, 10, 200), (24, 10, 100)), BARRIER, 60, 3), [(20, 10), (24, 10)], [199, 99], 2)


def test_kept_mask_rounds_to_even():
    m = R.kept_mask((H, W), [(20.5, 10.5)], 3)  # cvRound: (20, 10)
    assert m[10, 20] == 255 and m[10, 17] == 255 and m[10, 23] == 255 and m[10, 24] == 0 and m[14, 20] == 0


def test_symbols_and_validation():
    assert "esvio_fe_set_detector" in FE.ABI_SYMBOLS and "esvio_fe_features_to_track_fast" in FE.ABI_SYMBOLS
    L = FE.load_library()
    assert hasattr(L, "esvio_fe_set_detector") and hasattr(L, "esvio_fe_features_to_track_fast")
    assert len(L.esvio_fe_set_detector.argtypes) == 3 and len(L.esvio_fe_features_to_track_fast.argtypes) == 10
    n = C.c_int32(-7)
    # a NULL handle is refused before anything touches a device
    assert L.esvio_fe_set_detector(None, FE.DETECT_FAST, 20) == -1  # ESVIO_FE_EINVAL
    assert L.esvio_fe_features_to_track_fast(None, None, 0, 20, 10, None, None, None, C.byref(n), None) == -1
