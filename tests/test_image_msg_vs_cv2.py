"""The pin kit of the "rosbag images" gray (include/esvio_fe.h): cv2.cvtColor's 8-bit gray against the rule's 15-bit form
on a seeded 64 x 64 image per encoding class.  Skipped without cv2."""
import numpy as np
import pytest

import bag_image_ref as I

cv2 = pytest.importorskip("cv2")


@pytest.mark.parametrize("name", ["mono8", "8UC1", "bgr8", "8UC3", "rgb8"])
def test_the_rules_gray_equals_cv2s(name):
    cls = I.CLASSES[name.encode()]
    px = I.test_image(64, 64, cls, 300 + cls)
    ours = I.convert(px.tobytes(), 64, 64, 64 * I.BPP[cls], name)
    if cls == 1:
        theirs = px.copy()  # (toCvCopy of an unchanged encoding: the bytes)
    else:
        theirs = cv2.cvtColor(px.reshape(64, 64, 3), cv2.COLOR_BGR2GRAY if cls == 2 else cv2.COLOR_RGB2GRAY)
    if not np.array_equal(ours, theirs):
        a = px.reshape(64, 64, 3).astype(np.int64)
        r, g, b = (a[..., 2], a[..., 1], a[..., 0]) if cls == 2 else (a[..., 0], a[..., 1], a[..., 2])
        form14 = ((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14).astype(np.uint8)
        raise AssertionError("cv2 %s gives another gray on %d pixels; it %s the 14-bit form's" % (
            cv2.__version__, int((ours != theirs).sum()), "is" if np.array_equal(form14, theirs) else "is not"))
