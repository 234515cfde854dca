"""GPU: the shared stable radix sort alone — k_radix_pass through radix_sort_pairs, reached by the tap esvio_fe_sort_pairs
— against numpy.argsort(keys & mask, kind="stable") on the designed inputs of tests/sort_cases.py: exact equality of keys
(whole, the bits above the sorted range included) and values, the positions no pass may write, the expired-wait flag and
the tickets every pass hands out.  tests/test_sort_cases.py shows on the CPU what the inputs contain and that a wrong
pass would differ on them."""
import numpy as np
import pytest

import sort_cases as K
from esvio_amd import frontend as FE
from esvio_amd.events import event_times
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

W, H = 346, 260


@pytest.fixture(scope="module")
def ft():
    t = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    yield t
    t.close()


def run_case(ft, c):
    return ft.sort_pairs(c.keys, c.vals, c.passes, c.bits, -1 if c.n_dev is None else c.n_dev, K.FILL_KEY, K.FILL_VAL)


def check(ft, name):
    c = K.CASES[name]()
    want_k, want_v = K.reference(c)
    rc, k, v, err, tickets = run_case(ft, c)
    assert rc == 0 and err == 0, (name, rc, err)
    assert np.array_equal(tickets, K.tickets(c)), (name, tickets)
    bad = np.flatnonzero((k != want_k) | (v != want_v))
    assert not len(bad), "%s: %d of %d positions differ, the first at %d: (%#x, %#x), expected (%#x, %#x)" % (
        name, len(bad), len(k), bad[0], k[bad[0]], v[bad[0]], want_k[bad[0]], want_v[bad[0]])


@pytest.mark.parametrize("name", K.NAMES)
def test_sort_equals_stable_argsort(ft, name):
    check(ft, name)


def test_device_count_zero_writes_nothing(ft):
    """no pair takes part: both buffers come back as they went in, whichever holds the result"""
    for name, buf in (("n_dev_0_1x8", 1), ("n_dev_0_3x7", 1), ("n_dev_0_2x6", 0)):
        c = K.CASES[name]()
        rc, k, v, err, tickets = run_case(ft, c)
        want = K.tap_buffers(c)[buf]
        assert rc == 0 and err == 0 and np.array_equal(k, want[0]) and np.array_equal(v, want[1]), name
        assert np.array_equal(tickets, K.tickets(c))


@pytest.mark.parametrize("name,between", [("lookback_41_tiles_1x8", "size_513_3x7"), ("partial_ff_some_4x8", "width_1x3")])
def test_tap_leaves_nothing_behind(ft, name, between):
    """the same case twice on one handle with a call of another n and another bits in between"""
    a, b = K.CASES[name](), K.CASES[between]()
    assert len(a.keys) != len(b.keys) and a.bits != b.bits
    check(ft, name)
    check(ft, between)
    check(ft, name)


def test_arguments_are_checked(ft):
    k = np.arange(8, dtype=np.uint32)
    for passes, bits in ((0, 8), (5, 8), (1, 0), (1, 9), (-1, 4), (2, -3)):
        assert ft.sort_pairs(k, k, passes, bits)[0] == -1, (passes, bits)
    L, h = FE.load_library(), ft._hd.h
    out = np.zeros(8, np.uint32)
    err, tick = np.zeros(1, np.int32), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data
    assert L.esvio_fe_sort_pairs(h, p(k), p(k), 1 << 30, 1, 8, -1, p(out), p(out), err.ctypes.data_as(FE.C.POINTER(FE.C.c_int32)), p(tick)) == -1
    assert L.esvio_fe_sort_pairs(h, p(k), p(k), -1, 1, 8, -1, p(out), p(out), err.ctypes.data_as(FE.C.POINTER(FE.C.c_int32)), p(tick)) == -1
    assert L.esvio_fe_sort_pairs(h, p(k), p(k), 8, 1, 8, -2, p(out), p(out), err.ctypes.data_as(FE.C.POINTER(FE.C.c_int32)), p(tick)) == -1
    assert L.esvio_fe_sort_pairs(h, None, p(k), 8, 1, 8, -1, p(out), p(out), err.ctypes.data_as(FE.C.POINTER(FE.C.c_int32)), p(tick)) == -1
    rc, sk, sv, e, t = ft.sort_pairs(k[::-1].copy(), k, 1, 8)   # and the handle goes on working
    assert rc == 0 and e == 0 and np.array_equal(sk, k) and np.array_equal(sv, k[::-1]) and t[0] == 1


def test_track_calls_do_not_see_the_tap(monkeypatch):
    """two handles on the SAE sort path (the handle's own sort scratch in use) take the same three stereo batches; one of
    them makes tap calls of several shapes between its track calls: time surfaces, ids, counts and points stay equal"""
    monkeypatch.setenv("ESVIO_FE_SAE_SORT", "1")
    kw = dict(max_cnt=60, min_dist=10, f_ransac=1)
    plain, tapped = (FE.FeatureTracker(FE.make_config(W, H, **kw)) for _ in range(2))
    s = SceneStream(W, H, rate=1e6, seed=5, n_rect=12, size=(30.0, 90.0))
    for f in range(3):
        L, R, _ = s.next_batch()
        t = event_times(L)[-1]
        for name in ("size_4097_3x7", "n_dev_2049_1x8", "high_bits_dups_2x5")[f:f + 2]:
            check(tapped, name)
        for tr in (plain, tapped):
            tr.trackEvent(t, L, R, True)
        for cam in (0, 1):
            assert np.array_equal(plain.gettimesurface(cam), tapped.gettimesurface(cam)), (f, cam)
            for a, b in zip(plain.detector.get_sae(cam), tapped.detector.get_sae(cam)):
                assert np.array_equal(a, b), (f, cam)
        assert np.array_equal(plain.ids, tapped.ids) and np.array_equal(plain.track_cnt, tapped.track_cnt)
        assert np.array_equal(plain.ids_right, tapped.ids_right)
        assert np.array_equal(plain.cur_pts, tapped.cur_pts) and np.array_equal(plain.cur_right_pts, tapped.cur_right_pts)
    assert len(plain.ids) > 10
    plain.close()
    tapped.close()
