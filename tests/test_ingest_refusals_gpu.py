"""GPU: the refusals of the ingest entry points that no other suite asserts — BAD stamps in esvio_fe_track_raw and in the
feed's three byte pushes (raw words, AEDAT packets, a bag chunk) — each with the rule that goes with it: nothing is
appended or tracked, the info holds the exact BAD count, and the decoder or walker state is as it was, so that the same
bytes with a good offset (or good stamps) continue from the state before the failure.  (What the decode calls, the
trigger call and esvio_fe_track_aedat refuse is asserted in test_raw_gpu.py, test_evt21_gpu.py, test_triggers_gpu.py,
test_aedat_gpu.py and test_bag_gpu.py.)  The smallest shapes: a 346 x 260 handle, raw chunks of one tile plus one word,
AEDAT chunks of two packets of a few events, bag chunks of one message per camera."""
import numpy as np
import pytest

import aedat_ref as A
import bag_ref as B
import evt_ref as R
from esvio_amd import frontend as FE
from esvio_amd.events import make_events

pytestmark = pytest.mark.gpu

W, H = 346, 260


def tracker():
    return FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))


def raw_chunk(fmt, t0, seed):
    """one tile plus one word of EVT2: a TIME_HIGH word, then single events from t0 us on -> (words, records at offset 0)"""
    n = FE.load_library().esvio_fe_raw_tile_bytes() // 4
    rng = np.random.default_rng(seed)
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    t = t0 + np.arange(n) // 32  # (t0 a multiple of 64: inside one TIME_HIGH period, exactly one time word, n + 1 words)
    words = R.encode(fmt, x, y, p, t)
    assert words.nbytes == 4 * (n + 1)
    return words, make_events(x, y, t, p)


def test_track_raw_with_bad_stamps_in_the_right_camera_tracks_nothing_and_moves_neither_decoder():
    left, rec_l = raw_chunk(R.EVT2, 5_000_000, 1)
    right, rec_r = raw_chunk(R.EVT2, 1_024, 2)
    ft = tracker()
    try:
        with pytest.raises(FE.FrontendError, match="both cameras' decoder states are as they were") as e:
            ft.track_raw(R.EVT2, left, right, -2_000_000)  # the left stamps stay positive, every right one is negative
        assert (e.value.info.bad[0], e.value.info.bad[1]) == (0, len(rec_r)) and e.value.info.tracked == 0
        assert (e.value.info.kept[0], e.value.info.kept[1]) == (0, 0)
        assert (e.value.raw[0].events, e.value.raw[1].events, e.value.raw[1].bad) == (len(rec_l), len(rec_r), len(rec_r))
        assert len(ft.ids) == 0
        # a decoder that had taken the chunk over would hold its TIME_HIGH: events alone would then be timed
        for cam in (0, 1):
            rec, info = ft.decode_raw(cam, R.EVT2, left[1:])
            assert (len(rec), info.events, info.untimed) == (0, 0, len(rec_l))
        info, raw = ft.track_raw(R.EVT2, left, right, 0)
        assert info.tracked == 1 and (info.kept[0], info.kept[1]) == (len(rec_l), len(rec_r))
    finally:
        ft.close()


def test_feed_push_raw_with_bad_stamps_appends_nothing_and_leaves_the_decoder():
    words, rec = raw_chunk(R.EVT2, 1_024, 3)
    for filtered in (False, True):
        ft = tracker()
        try:
            ft.feed_open(1000.0, params=FE.FilterParams(1_000_000, 0) if filtered else None)
            with pytest.raises(FE.FrontendError, match="nothing was appended, the camera's decoder state is as it was") as e:
                ft.feed_push_raw(0, R.EVT2, words, -2_000_000)
            assert (e.value.info.appended, e.value.info.bad, e.value.info.closed) == (0, len(rec), 0)
            info = ft.feed_push_raw(0, R.EVT2, words[1:])  # no TIME_HIGH seen yet: nothing is timed, nothing appended
            assert (info.appended, info.bad) == (0, 0)
            info = ft.feed_push_raw(0, R.EVT2, words)
            assert (info.appended, info.bad) == (len(rec), 0)
        finally:
            ft.close()


def test_feed_push_aedat_with_bad_stamps_appends_nothing_and_leaves_the_walker():
    ev = [A.polarity(10 + k, 20, k & 1, 1000 + k) for k in range(5)]
    data = A.packet(1, ev[:3]) + A.packet(1, ev[3:])
    cut = len(data) - 4  # the last record waits in the walker
    ft = tracker()
    try:
        ft.feed_open(1000.0)
        assert ft.feed_push_aedat(0, data[:cut]).appended == 4
        with pytest.raises(FE.FrontendError, match="nothing was appended, the camera's state is as it was") as e:
            ft.feed_push_aedat(0, data[cut:] + A.packet(1, ev[:2]), -(2 ** 62))
        assert (e.value.info.appended, e.value.info.bad) == (0, 3)
        info = ft.feed_push_aedat(0, data[cut:] + A.packet(1, ev[:2]))  # the waiting record is still there
        assert (info.appended, info.bad) == (3, 0)
    finally:
        ft.close()


def test_feed_push_bag_with_bad_stamps_appends_nothing_to_either_camera_and_leaves_the_walker():
    conns = B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5) + B.connection_record(1, B.RIGHT, B.EVENT_TYPE, B.EVENT_MD5)
    n = 6
    wire = lambda nsec: B.wire_events(np.arange(n), np.arange(n), np.full(n, 7), nsec, np.ones(n, np.int64))
    good, bad = wire(1000 + np.arange(n)), wire(np.where(np.arange(n) == 2, 10 ** 9, 1000 + np.arange(n)))
    chunk = lambda right: B.chunk_record(B.message_record(0, (7, 1), B.event_array(1, (7, 1), good)) +
                                         B.message_record(1, (7, 2), B.event_array(1, (7, 2), right)))
    ft = tracker()
    try:
        ft.bag_set_topics(*B.TOPICS)
        ft.feed_open(1000.0)
        info = ft.feed_push_bag(B.chunk_record(conns))
        assert (info[0].appended, info[1].appended) == (0, 0)
        with pytest.raises(FE.FrontendError, match="nothing was appended, the walker's state is as it was") as e:
            ft.feed_push_bag(chunk(bad))
        assert [(i.appended, i.bad) for i in e.value.info] == [(0, 0), (0, 1)]
        info = ft.feed_push_bag(chunk(good))  # the connections of the first call are still known, nothing came twice
        assert [(i.appended, i.bad) for i in info] == [(n, 0), (n, 0)]
    finally:
        ft.close()
