"""CPU: the sequential restatement of the background-activity filter (tests/ba_filter_ref.py) against answers derived
by hand from the text of include/esvio_fe.h, and the library's side of the boundary that needs no device: the three
entry points are exported and refuse a null handle."""
import numpy as np
import pytest

import ba_filter_cases as K
import ba_filter_ref as R
from esvio_amd import frontend as FE


@pytest.mark.parametrize("name", sorted(K.HAND))
def test_restatement_gives_the_hand_derived_answers(name):
    ev, min_support, want, rejected = K.hand_case(name)
    B = R.fresh_plane(K.W, K.H)
    flags, rej = R.filter_events(B, K.W, K.H, ev, K.WINDOW, min_support)
    assert flags.tolist() == want.tolist() and rej == rejected
    # step 5: every in-sensor event has stamped its pixel, kept or not; nothing else is stamped
    stamped = {}
    for e in ev:
        if e["x"] < K.W and e["y"] < K.H:
            stamped[int(e["x"]) + int(e["y"]) * K.W] = int(e["sec"]) * 10 ** 9 + int(e["nsec"])
    want_plane = R.fresh_plane(K.W, K.H)
    for q, t in stamped.items():
        want_plane[q] = t
    assert np.array_equal(B, want_plane)


def test_the_plane_carries_over_and_kept_records_are_in_order():
    """the second call's first event finds the support the first call left; a stamp-0 plane entry is not `none`"""
    B = R.fresh_plane(K.W, K.H)
    first = K.records([(10, 10, 0, 0)])
    flags, _ = R.filter_events(B, K.W, K.H, first, K.WINDOW)
    assert flags.tolist() == [0] and B[10 + 10 * K.W] == 0
    second = K.records([(11, 11, 0, 999), (30, 30, 0, 999), (12, 12, 0, 1500)])
    flags, _ = R.filter_events(B, K.W, K.H, second, K.WINDOW)
    assert flags.tolist() == [1, 0, 1]
    kept, last = R.kept_of(second, flags)
    assert kept.tobytes() == R.raw_records(second)[[0, 2]].tobytes() and last.tobytes() == R.raw_records(second)[2].tobytes()
    assert R.kept_of(first, np.zeros(1, np.uint8))[1] is None


def test_generated_streams_are_not_vacuous():
    """the sweep and the hot-pixel stream keep neither nothing nor everything (the GPU test asserts the same of every
    stream it compares)"""
    for n in K.SWEEP_SIZES:
        if n >= 63:
            flags, rej = R.filter_events(R.fresh_plane(K.W, K.H), K.W, K.H, K.sweep_events(n), 1_000_000)
            assert rej == 0 and 0.1 <= flags.mean() <= 0.9, (n, flags.mean())
    flags, _ = R.filter_events(R.fresh_plane(K.W, K.H), K.W, K.H, K.hot_pixel_events(), 2000)
    assert 0.1 <= flags.mean() <= 0.9, flags.mean()
    flags, _ = R.filter_events(R.fresh_plane(K.W, K.H), K.W, K.H, K.sweep_events(1), 1_000_000)
    assert flags.tolist() == [0]  # one event alone has no support, by definition


def test_entry_points_are_exported_and_refuse_a_null_handle():
    L = FE.load_library()
    for name in ("esvio_fe_filter_events", "esvio_fe_filter_reset", "esvio_fe_track_event_filtered"):
        assert hasattr(L, name), name
        assert name in FE.ABI_SYMBOLS
    assert L.esvio_fe_filter_events(None, 0, None, 0, FE.HOST, 1_000_000, 1, None, FE.HOST, None, None, None, None) == -1
    assert L.esvio_fe_filter_reset(None) == -1
    assert L.esvio_fe_track_event_filtered(None, None, 0, None, 0, FE.HOST, 1_000_000, 1, 1, None, None, None) == -1
