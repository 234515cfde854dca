"""The min-distance selection on the device — k_select_mw (16 waves), k_select (one wave), k_select_gbm (one wave, the
bitmap in device memory), and the half-width table path none of their callers takes — held to tests/select_ref.py over
the case families of tests/select_cases.py through esvio_fe_select_candidates.  Everything is equality: the accepted
points as bits, their payloads, the three counts, the poisoned output behind the last accepted point untouched, and the
name of the kernel that ran.  tests/test_select_cases.py shows on the CPU that the families reach their edges.

One handle per sensor size serves every case, a few thousand calls in a row: state that leaked from call to call
would show as a mismatch somewhere down the line."""
import numpy as np
import pytest

from esvio_amd import frontend as FE

import select_cases as SC

pytestmark = pytest.mark.gpu

POISON_XY, POISON_IDX = -12345.5, -987654321
# (variant, table flag) -> the kernel a small handle must report
MODES = {"handle": (0, False, "k_select_mw"), "one_wave": (1, False, "k_select"), "device_bitmap": (2, False, "k_select_gbm"),
         "handle_table": (0, True, "k_select_mw"), "one_wave_table": (1, True, "k_select")}


@pytest.fixture(scope="module")
def handles():
    """one handle per size, made when first asked for"""
    made = {}

    def get(size):
        if size not in made:
            made[size] = FE.FeatureTracker(FE.make_config(size[0], size[1], max_cnt=SC.MAX_CNT[size], min_dist=10))
        return made[size]
    yield get
    for ft in made.values():
        ft.close()


def run(ft, case, variant, table):
    return ft.select_candidates(case["xy"], case["payload"], case["d"], euclid=case["kind"] == "euclid", table=table,
                                mask=case["mask"], stamp_pts=case["stamps"], max_corners=case["max_corners"],
                                out_base=case["out_base"], variant=variant, poison=(POISON_XY, POISON_IDX))


def check(ft, case, variant, table, kernel):
    out_xy, out_idx, counts, name = run(ft, case, variant, table)
    pts, idx, cnt = SC.expected(case)
    tag = "%s [variant %d%s]" % (case["name"], variant, ", table" if table else "")
    assert name == kernel, "%s ran %s, not %s" % (tag, name, kernel)
    assert counts.tolist() == cnt.tolist(), "%s: counts %s, reference %s" % (tag, counts.tolist(), cnt.tolist())
    n, b = int(cnt[0]), case["out_base"]
    assert np.array_equal(out_xy[b:b + n].view(np.uint32), pts.view(np.uint32)), "%s: points differ, first at %s" % (
        tag, np.flatnonzero((out_xy[b:b + n] != pts).any(1))[:3].tolist())
    assert np.array_equal(out_idx[:n], idx), "%s: payloads differ" % tag
    assert (out_xy[:b] == np.float32(POISON_XY)).all() and (out_xy[b + n:] == np.float32(POISON_XY)).all(), \
        "%s: written outside out_xy[out_base : out_base + accepted]" % tag
    assert (out_idx[n:] == POISON_IDX).all(), "%s: written behind out_idx[accepted]" % tag


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("family", list("abcdefghi"))
def test_family_on_small_handles(handles, family, mode):
    variant, table, kernel = MODES[mode]
    cases = SC.small_cases()[family]
    assert cases
    for case in cases:
        check(handles((case["W"], case["H"])), case, variant, table, kernel)


@pytest.mark.parametrize("size,kernel", [(SC.LARGE_ONE_WAVE, "k_select"), (SC.LARGE_GBM, "k_select_gbm")])
def test_other_kernels_the_natural_way(handles, size, kernel):
    """1280x960 with max_cnt 300: the bitmap fits LDS, the 16-wave kernel's queue beside it does not; 1440x1080: the
    bitmap is in device memory — variant 0 must reach them, with and without the table"""
    ft = handles(size)
    for fam in ("a", "i"):
        for case in SC.large_cases(size)[fam]:
            check(ft, case, 0, False, kernel)
    for case in SC.large_cases(size)["a"][:8] + SC.large_cases(size)["i"]:
        check(ft, case, 0, True, kernel)


def test_no_state_from_call_to_call(handles):
    """a heavy case, the empty list, the heavy case again, on every kernel: identical results, the empty call's
    output untouched"""
    ft = handles((346, 260))
    heavy = [c for c in SC.small_cases()["i"] if (c["W"], c["kind"], c["d"]) == (346, "circle", 3)][0]
    empty = [c for c in SC.small_cases()["d"] if c["xy"].size == 0][0]
    stamped = [c for c in SC.small_cases()["g"] if c["W"] == 346 and c["name"].endswith("c16 both")][0]
    for variant, table, kernel in MODES.values():
        first = run(ft, heavy, variant, table)
        check(ft, stamped, variant, table, kernel)  # (leaves a mask and kept points behind)
        check(ft, empty, variant, table, kernel)
        again = run(ft, heavy, variant, table)
        assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and first[3] == again[3] == kernel
        check(ft, heavy, variant, table, kernel)


def test_bad_arguments_are_refused(handles):
    ft = handles((64, 48))
    ok = dict(xy=SC.pack_xy([3], [4]), payload=[1], disc=3)
    ft.select_candidates(**ok)
    for bad in (dict(ok, xy=SC.pack_xy([64], [4])), dict(ok, xy=SC.pack_xy([3], [48])), dict(ok, disc=0), dict(ok, disc=64),
                dict(ok, disc=3.5), dict(ok, disc=0.5, euclid=True), dict(ok, variant=3), dict(ok, max_corners=SC.MAX_CNT_SMALL + 1),
                dict(ok, max_corners=SC.MAX_CNT_SMALL, out_base=1), dict(ok, out_base=-1),
                dict(ok, stamp_pts=[(64.0, 3.0)]), dict(ok, stamp_pts=[(3.0, 47.6)]), dict(ok, stamp_pts=[(-0.6, 3.0)]),
                dict(ok, stamp_pts=[(float("nan"), 3.0)]), dict(ok, stamp_pts=np.zeros((SC.MAX_CNT_SMALL + 1, 2)))):
        with pytest.raises(FE.FrontendError):
            ft.select_candidates(**bad)
    ft.select_candidates(**dict(ok, disc=3.5, euclid=True))
    ft.select_candidates(**dict(ok, stamp_pts=[(-0.5, 47.4)]))


def test_public_entry_points_after_tap_calls(oracle):
    """Event_FeaturesToTrack with a mask and goodFeaturesToTrack at min_distance 1 and 63 on a handle that has served
    tap calls on every kernel — the device-memory bitmap is allocated by the first forced call — give what a fresh
    handle gives"""
    from esvio_amd.events import event_times
    from esvio_amd.synth import ImageStream, SceneStream
    W, H = 346, 260
    L, R, _ = SceneStream(W, H, rate=1e6, seed=3, n_rect=12, size=(30.0, 90.0)).next_batch()
    img = ImageStream(W, H, seed=5).next_frame()[0]
    mask = np.zeros((H, W), np.uint8)
    mask[60:140, 100:220] = 255
    case = [c for c in SC.small_cases()["g"] if c["W"] == W and c["name"].endswith("e33 both")][0]

    def public(ft):
        ft.detector.createSAE_stereo(L, R)
        ft.detector.SAEtoTimeSurface_left(event_times(L)[-1])
        a = ft.Event_FeaturesToTrack(L, 150, mask)
        return a + (ft.goodFeaturesToTrack(img, 150, 0.01, 1), ft.goodFeaturesToTrack(img, 150, 0.01, 63))
    kw = dict(max_cnt=150, min_dist=10)
    fresh = FE.FeatureTracker(FE.make_config(W, H, **kw))
    used = FE.FeatureTracker(FE.make_config(W, H, **kw))
    try:
        want = public(fresh)
        assert len(want[0]) > 5 and len(want[2]) > len(want[3]) > 0
        small = dict(case, max_corners=150)
        small.pop("_expected", None)
        for variant, table, kernel in MODES.values():
            check(used, small, variant, table, kernel)
            got = public(used)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (variant, table)
    finally:
        fresh.close()
        used.close()
