"""CPU: the sequential restatement of the filter rule with esvio_fe_filter_params (tests/ba_filter2_ref.py) against
the restatement of esvio_fe_filter_events where the two rules coincide, against answers derived by hand from the text
of include/esvio_fe.h, and the parameters the GPU test uses against its two non-vacuity conditions."""
import numpy as np
import pytest

import ba_filter2_ref as R2
import ba_filter_cases as K
import ba_filter_ref as R

MS = 1_000_000


@pytest.mark.parametrize("name", sorted(K.HAND))
def test_equals_the_first_restatement_on_the_hand_cases(name):
    ev, min_support, want, rejected = K.hand_case(name)
    B1, B2 = R.fresh_plane(K.W, K.H), R2.fresh_plane(K.W, K.H)
    f1, r1 = R.filter_events(B1, K.W, K.H, ev, K.WINDOW, min_support)
    f2, r2 = R2.filter_events(B2, K.W, K.H, ev, K.WINDOW, min_support, 0)
    assert f2.tolist() == f1.tolist() == want.tolist() and r1 == r2 == rejected and np.array_equal(B1, B2)


@pytest.mark.parametrize("n", K.SWEEP_SIZES)
def test_equals_the_first_restatement_on_the_sweep_streams(n):
    ev = K.sweep_events(n)
    B1, B2 = R.fresh_plane(K.W, K.H), R2.fresh_plane(K.W, K.H)
    for min_support, window in ((1, MS), (2, 3 * MS)):  # (the second call runs on the plane the first left)
        f1, r1 = R.filter_events(B1, K.W, K.H, ev, window, min_support)
        f2, r2 = R2.filter_events(B2, K.W, K.H, ev, window, min_support, 0)
        assert np.array_equal(f1, f2) and r1 == r2 and np.array_equal(B1, B2)


# name -> (rows (x, y, sec, nsec), window, min_support, refractory, flags, n_rejected): derived by hand from the header
HAND2 = {
    # the dropped second event stamped the pixel (1200 - 600 < 1000); [1,0,1] would mean it had not
    "dropped_event_stamps": ([(5, 5, 0, 100), (5, 5, 0, 600), (5, 5, 0, 1200)], 1, 0, 1000, [1, 0, 0], 0),
    # 1000 < 1000 is false
    "at_the_period": ([(5, 5, 0, 100), (5, 5, 0, 1100)], 1, 0, 1000, [1, 1], 0),
    # a negative difference counts
    "pixel_stamped_later": ([(5, 5, 0, 5000), (5, 5, 0, 1000)], 1, 0, 1000, [1, 0], 0),
    # stamp 0 is a stamp
    "stamp_zero": ([(3, 3, 0, 0), (3, 3, 0, 500)], 1, 0, 1000, [1, 0], 0),
    # no refractory test, no support test: everything in the sensor is kept
    "both_off": ([(5, 5, 0, 100), (5, 5, 0, 200), (5, 5, 0, 300)], 1, 0, 0, [1, 1, 1], 0),
    # the third has support ((10,10) is 999 ns older) but is refractory (its own pixel was stamped 499 ns before)
    "supported_but_refractory": ([(10, 10, 0, 5000), (11, 10, 0, 5500), (11, 10, 0, 5999)], 1000, 1, 1000, [0, 1, 0], 0),
    # an out-of-sensor event between two same-pixel events is rejected, flag 0, and neither reads nor writes B: x = 42
    # would land on pixel (0, 6) = 42 + 5*42 if it were written — (0,6) at 900 ns is not refractory; the third event
    # is refractory against the first (700 < 1000), across the rejected one
    "rejected_between": ([(5, 5, 0, 100), (42, 5, 0, 400), (5, 5, 0, 800), (0, 6, 0, 900)], 1, 0, 1000, [1, 0, 0, 1], 1),
}


@pytest.mark.parametrize("name", sorted(HAND2))
def test_hand_derived_refractory_cases(name):
    rows, window, min_support, refractory, want, rejected = HAND2[name]
    ev = K.records(rows)
    B = R2.fresh_plane(K.W, K.H)
    flags, rej = R2.filter_events(B, K.W, K.H, ev, window, min_support, refractory)
    assert flags.tolist() == want and rej == rejected
    # step 5: every in-sensor event has stamped its pixel — kept or not, refractory or not; nothing else is stamped
    want_plane = R2.fresh_plane(K.W, K.H)
    for x, y, sec, nsec in rows:
        if x < K.W and y < K.H:
            want_plane[x + y * K.W] = sec * 10 ** 9 + nsec
    assert np.array_equal(B, want_plane)


def fractions(ev, w, h, window, min_support, refractory):
    """(kept fraction, the share of the events the support test alone keeps that the refractory test drops)"""
    flags, _, sup, refr = R2.filter_events(R2.fresh_plane(w, h), w, h, ev, window, min_support, refractory, want_parts=True)
    return float(flags.mean()), float((sup & refr).sum()) / max(int(sup.sum()), 1)


def test_the_gpu_tests_parameters_are_not_vacuous():
    """every random case of tests/test_batch_gpu.py keeps between 10 % and 90 %, and its refractory test drops at
    least 10 % of what the support test alone keeps"""
    for n in K.SWEEP_SIZES:
        if n >= 63:
            kept, dropped = fractions(K.sweep_events(n), K.W, K.H, MS, 1, 4 * MS)
            assert 0.1 <= kept <= 0.9 and dropped >= 0.1, (n, kept, dropped)
            kept, _ = fractions(K.sweep_events(n), K.W, K.H, 0, 0, 4 * MS)
            assert 0.1 <= kept <= 0.9, (n, kept)
    kept, dropped = fractions(K.hot_pixel_events(), K.W, K.H, 2000, 1, 4000)
    assert 0.1 <= kept <= 0.9 and dropped >= 0.1, (kept, dropped)
    kept, dropped = fractions(K.uniform_events(3000, 64, 48, 24000, seed=40), 64, 48, MS, 1, 8 * MS)
    assert 0.1 <= kept <= 0.9 and dropped >= 0.1, (kept, dropped)
