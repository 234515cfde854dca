"""The pin kit of the two rules the keyframe stage restates from recall (include/esvio_fe.h "keyframes": B and F are
UNPINNED): where OpenCV's Python module is at hand, tests/kf_ref.py's blur and corners are held against
cv2.GaussianBlur(9x9, sigma 2) and cv2.FastFeatureDetector_create(threshold, True, TYPE_9_16) on the committed images of
tests/golden/kf_cv2_inputs.npz.  Skipped where cv2 is absent.  INTEGRATION.md section 7 lists it."""
import os

import numpy as np
import pytest

import kf_ref as K

cv2 = pytest.importorskip("cv2")
INPUTS = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kf_cv2_inputs.npz"))


@pytest.mark.parametrize("name", ["random", "blocky", "smooth"])
def test_blur_is_cv2_gaussian_blur(name):
    img = INPUTS[name]
    assert np.array_equal(K.blur(img), cv2.GaussianBlur(img, (9, 9), 2, sigmaY=2, borderType=cv2.BORDER_REFLECT_101))


@pytest.mark.parametrize("threshold", [0, 1, 20, 60])
@pytest.mark.parametrize("name", ["random", "blocky", "smooth"])
def test_corners_are_cv2_fast(name, threshold):
    img = INPUTS[name]
    kps = cv2.FastFeatureDetector_create(threshold, True, cv2.FAST_FEATURE_DETECTOR_TYPE_9_16).detect(img)
    xy, score, _ = K.fast(img, threshold)
    assert [(kp.pt[0], kp.pt[1], kp.response) for kp in kps] == [(float(x), float(y), float(s)) for (x, y), s in zip(xy, score)]
