"""The pyramids a track call builds, read back level by level (esvio_fe_export_level) and compared with the oracle byte
for byte: image interior, the whole 24-pixel BORDER_REFLECT_101 ring, and the derivative plane with its zero ring — for
both cameras, every level, every size x content of tests/pyr_cases.py and every path into build_lk_images / pyr_build:
the fused kernels per camera (camera split) and for both cameras in one launch, `equalize` (k_clahe_lut, k_clahe_interp,
k_norm_pyr), the unfused kernels (ESVIO_FE_NO_FUSE), a median in front of them, an imported right image, and trackImage
with and without CLAHE.  Everything is integer: no tolerance.  tests/test_pyr_cases.py shows that the inputs reach the
edges they are for."""
import numpy as np
import pytest

from esvio_amd import frontend as FE

import pyr_cases as PC

pytestmark = pytest.mark.gpu

# path -> (environment, config, what the oracle makes of the rendered surface)
EVENT_PATHS = {
    "camsplit": ({}, {}, "plain"),
    "one_launch": ({"ESVIO_FE_NO_CAMSPLIT": "1"}, {}, "plain"),
    "equalize": ({}, {"equalize": 1}, "equalize"),
    "nofuse": ({"ESVIO_FE_NO_FUSE": "1"}, {}, "plain"),
    "nofuse_equalize": ({"ESVIO_FE_NO_FUSE": "1"}, {"equalize": 1}, "equalize"),
    "median1": ({}, {"median_blur_kernel_size": 1}, "median1"),
    "median2": ({}, {"median_blur_kernel_size": 2}, "median2"),
}
ENV_OPTIONS = ("ESVIO_FE_NO_CAMSPLIT", "ESVIO_FE_NO_FUSE")
CFG = dict(max_cnt=50, min_dist=10)

_REF = {}  # (W, H, frame, camera, kind) -> expected pyramid, computed once and shared by the paths


def _expected(oracle, W, H, name, cam, kind, surface):
    key = (W, H, name, cam, kind)
    if key not in _REF:
        _REF[key] = PC.expected_pyramid(oracle, PC.level0(oracle, kind, surface))
    return _REF[key]


def _first_difference(got, want):
    y, x = np.argwhere(got != want)[0][:2]
    return int(y), int(x), got[y, x].tolist(), want[y, x].tolist()


def _compare(ft, want_by_cam, tag, cams=(0, 1)):
    bad = []
    for cam in cams:
        want = want_by_cam[cam]
        for level, (w_im, w_dv) in enumerate(want):
            im, dv, top = ft.export_level(cam, level)
            assert top == len(want) - 1 and im.shape == w_im.shape, (tag, cam, level, top, im.shape, w_im.shape)
            P = PC.PAD
            ring = np.ones(im.shape, bool)
            ring[P:-P, P:-P] = False
            for what, g, w in (("image interior", im[P:-P, P:-P], w_im[P:-P, P:-P]),
                               ("image ring", np.where(ring, im, 0), np.where(ring, w_im, 0)),
                               ("derivatives", dv, w_dv)):
                if not np.array_equal(g, w):
                    y, x, gv, wv = _first_difference(g, w)
                    if what == "image interior":
                        y, x = y + P, x + P
                    bad.append("%s cam %d level %d %s: %d differ, first at padded (y %d, x %d): got %s, want %s" % (
                        tag, cam, level, what, int((g != w).sum()), y, x, gv, wv))
    assert not bad, "\n".join(bad[:12])


def _setenv(monkeypatch, env):
    for o in ENV_OPTIONS:
        monkeypatch.delenv(o, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _track_frame(oracle, ft, W, H, frame, k):
    """the frame's planes into the handle, one track call with one event per camera -> the oracle's surfaces"""
    t, evL, evR, planes, ts = PC.oracle_surfaces(oracle, W, H, frame, k)
    Z = np.zeros((H, W))
    for cam in range(2):
        ft.detector.set_sae(cam, Z, Z, planes[cam][0], planes[cam][1])
    return t, evL, evR, ts


@pytest.mark.parametrize("W,H", list(PC.FOUR_LEVEL))
@pytest.mark.parametrize("path", list(EVENT_PATHS))
def test_track_event_pyramids(oracle, monkeypatch, path, W, H):
    env, cfg, kind = EVENT_PATHS[path]
    _setenv(monkeypatch, env)  # (read when the handle is created)
    ft = FE.FeatureTracker(FE.make_config(W, H, **dict(CFG, **cfg)))
    try:
        for k, f in enumerate(PC.frames(oracle, W, H, clahe=kind == "equalize")):
            t, evL, evR, ts = _track_frame(oracle, ft, W, H, f, k)
            if path == "camsplit":  # (a plain call is split by camera for a batch in device memory or a staged one)
                bufs = [FE.EventBuffer(ev, FE.DEVICE) for ev in (evL, evR)]
                ft.trackEvent(t, bufs[0].arg, bufs[1].arg, k % 3 != 2)
                for b in bufs:
                    b.free()
            else:
                ft.trackEvent(t, evL, evR, k % 3 != 2)
            want = [_expected(oracle, W, H, f.name, cam, kind, ts[cam]) for cam in range(2)]
            _compare(ft, want, "%dx%d %s %s" % (W, H, path, f.name))
        calls = ft.plain_call_counters()  # the path the name promises
        assert calls["plain_calls"] == k + 1 and calls["split_by_camera"] == (k + 1 if path == "camsplit" else 0), calls
    finally:
        ft.close()


@pytest.mark.parametrize("W,H", list(PC.FOUR_LEVEL))
def test_imported_right_image_gets_its_pyramid(oracle, monkeypatch, W, H):
    """esvio_fe_import_image, then a track call: the left pyramid from the planes, the right one from the image"""
    _setenv(monkeypatch, {})
    ft = FE.FeatureTracker(FE.make_config(W, H, **CFG))
    try:
        for k, f in enumerate(PC.frames(oracle, W, H)):
            t, evL, evR, ts = _track_frame(oracle, ft, W, H, f, k)
            ft.import_image(1, f.right)
            ft.trackEvent(t, evL, evR, k % 3 != 2)
            want = [_expected(oracle, W, H, f.name, 0, "plain", ts[0]),
                    _expected(oracle, W, H, f.name + "/image", 1, "plain", f.right)]
            _compare(ft, want, "%dx%d import %s" % (W, H, f.name))
    finally:
        ft.close()


@pytest.mark.parametrize("W,H", list(PC.FOUR_LEVEL) + list(PC.SMALL))
@pytest.mark.parametrize("equalize", [0, 1])
def test_track_image_pyramids(oracle, monkeypatch, equalize, W, H):
    """image handles: the caller's images (CLAHE without normalisation with `equalize`), then pyr_build — also on the
    one- and two-level sizes"""
    _setenv(monkeypatch, {})
    kind = "image_equalize" if equalize else "plain"
    ft = FE.FeatureTracker(FE.make_config(W, H, equalize=equalize, **CFG))
    try:
        for k, f in enumerate(PC.frames(oracle, W, H, clahe=bool(equalize))):
            ft.trackImage(0.05 * (k + 1), f.left, f.right, k % 3 != 2)
            want = [_expected(oracle, W, H, f.name + "/image", cam, kind, img) for cam, img in enumerate((f.left, f.right))]
            _compare(ft, want, "%dx%d trackImage equalize %d %s" % (W, H, equalize, f.name))
    finally:
        ft.close()


def test_export_level_after_a_lazy_call(oracle, monkeypatch):
    """with set_lazy_new_stereo a published call returns before the stereo LK of its new corners; the tap completes what
    is open and reads the same pyramids"""
    _setenv(monkeypatch, {})
    W, H = 176, 176
    ft = FE.FeatureTracker(FE.make_config(W, H, **CFG))
    try:
        ft.set_lazy_new_stereo(True)
        for k, f in enumerate(PC.frames(oracle, W, H)[:3]):
            t, evL, evR, ts = _track_frame(oracle, ft, W, H, f, k)
            ft.trackEvent(t, evL, evR, True)
            want = [_expected(oracle, W, H, f.name, cam, "plain", ts[cam]) for cam in range(2)]
            _compare(ft, want, "%dx%d lazy %s" % (W, H, f.name))
    finally:
        ft.close()


def test_export_level_refuses_what_it_cannot_read(oracle, monkeypatch):
    _setenv(monkeypatch, {})
    W, H = 176, 176
    ft = FE.FeatureTracker(FE.make_config(W, H, **CFG))
    try:
        f = PC.frames(oracle, W, H)[0]
        t, evL, evR, ts = _track_frame(oracle, ft, W, H, f, 0)
        ft.trackEvent(t, evL, evR, True)
        for cam, level in ((2, 0), (-1, 0), (0, 4), (0, -1)):
            with pytest.raises(FE.FrontendError, match="rc=-1"):
                ft.export_level(cam, level)
        t2, t2_us = PC.frame_time(1)
        ft.set_next_batch(t2, *PC.frame_events(W, H, t2_us))
        with pytest.raises(FE.FrontendError, match="rc=-1"):  # a batch is announced
            ft.export_level(0, 0)
        ft.reset()
    finally:
        ft.close()
