"""numpy restatement of ESVIO_FE_DETECT_FAST (include/esvio_fe.h: esvio_fe_set_detector), the definition a FAST handle's
trackEvent and esvio_fe_features_to_track_fast are tested against.

Test infrastructure, not product code.  Built from tests/fast_ref.py::fast_corners (tied to the reference's compiled
FAST by tests/test_fast_ref.py) and oracle.circle_fill (the cv::circle restatement the Arc* selection is tested with);
tests/test_fast_select_ref.py checks it against answers worked out by hand.

    1. C = fast_corners(img, arc 10, barrier, non-max), with their score_10
    2. C by score, descending; equal scores stay in raster order (the list is in raster order, the sort is stable)
    3. Event_FeaturesToTrack's scan (feature_tracker.cpp:13-38) from a copy of the mask: skip a blocked pixel, skip a
       pixel whose byte is (uint8_t)ts_lk_threshold, else accept ((float)x, (float)y) and block cv::circle(min_dist);
       stop at max_corners
"""
import numpy as np

import fast_ref
from oracle import oracle as O


def candidates(img, barrier):
    """steps 1 and 2: (xy int16 [n, 2], score int32 [n]) in scan order"""
    xy, sc, _ = fast_ref.fast_corners(img, 10, barrier, True)
    order = np.argsort(-sc.astype(np.int64), kind="stable")
    return xy[order], sc[order]


def select(img, barrier, max_corners, min_dist, mask=None, ts_lk_threshold=128.0, cand=None):
    """-> (xy float32 [k, 2], score int32 [k], n_candidates); mask: (H, W) u8, 255 = blocked, or None;
    cand: candidates(img, barrier) computed before (they do not depend on the other arguments)"""
    img = np.ascontiguousarray(img, np.uint8)
    xy, sc = cand if cand is not None else candidates(img, barrier)
    work = np.zeros(img.shape, np.uint8) if mask is None else (np.asarray(mask) == 255).astype(np.uint8) * 255
    work = np.ascontiguousarray(work)
    skip = int(ts_lk_threshold) & 255
    out_xy, out_sc = [], []
    for (x, y), s in zip(xy.tolist(), sc.tolist()):
        if len(out_xy) >= max_corners:
            break
        if work[y, x] == 255 or img[y, x] == skip:
            continue
        out_xy.append((x, y))
        out_sc.append(s)
        O.circle_fill(work, x, y, min_dist, 255)
    return (np.asarray(out_xy, np.float32).reshape(-1, 2), np.asarray(out_sc, np.int32), len(xy))


def kept_mask(shape, pts, min_dist):
    """Event_setMask's blocked pixels (255) for the points it kept: cv::circle(cvRound(pt), min_dist), filled"""
    m = np.zeros(shape, np.uint8)
    for x, y in np.asarray(pts, np.float32).reshape(-1, 2):
        O.circle_fill(m, int(np.rint(x)), int(np.rint(y)), min_dist, 255)  # cvRound: to nearest, ties to even
    return m
