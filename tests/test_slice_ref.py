"""CPU: the two sequential loops of tests/slice_ref.py — slice_windows(), the stream-slicing rule of include/esvio_fe.h,
and repack(), the reference's EventMessageEditor as it is written — against answers derived by hand, against each other
where the header says they agree, and repack() against recordings of the reference's compiled tool
(tests/golden/repack_ref_*.npz, made by tests/golden/make_repack_ref.py).  The recordings pin the tool's control flow —
first-event origin, >=, one advance per event, empty messages, the dropped tail — not roscpp's rounding, which the
generator's stand-in ros::Time restates as slice_ref.time_from_sec does."""
import glob
import os

import numpy as np
import pytest

import slice_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
# the hand-worked 1000 Hz chain: origin (10 s, 500 ns), period 0.001 -> E_k = 10 s + (k + 1) ms + 500 ns.  Worked: ts_origin
# = 10.0000005; 10.0000005 + 0.001 = 10.0010005 (+-2e-15); (d - 10) * 1e9 = 1000500.000000 +- 2e-6 -> 1000500; and so on,
# every step adds 1000000.000 +- 2e-6 to a whole number of nanoseconds
O1K = (10, 500)


def ev(*nsecs, sec=10):
    return [sec] * len(nsecs), list(nsecs)


def test_time_rounds_half_away_and_carries():
    assert S.time_from_sec(1.5) == (1, 500000000)
    assert S.time_from_sec(0.0) == (0, 0) and S.time_from_sec(7.25) == (7, 250000000)
    assert S.time_from_sec(3.9999999996) == (4, 0)           # nsec rounds to 10^9: the carry
    assert S.to_sec(4294967295, 999999999) == 4294967295.0 + 1e-9 * 999999999.0


def test_the_30_hz_chain_by_hand():
    """origin (0, 0); period = 1/30 = 0.0333333333333333328707...  E_0: round(33333333.33333333) = 33333333.  toSec(E_0) =
    0.033333333; + period = 0.0666666663333333 -> 66666666.  Every step adds 33333333.33 to a whole number of nanoseconds
    and rounds down: E_k = 33333333 * (k + 1) ns, drifting 1/3 ns per window against k / 30 — so E_29 = 999999990 ns and
    E_30 crosses the second: 1033333323 ns = (1, 33333323)."""
    s = S.Slicer(30.0, origin=(0, 0))
    assert [s.boundary(k) for k in range(4)] == [(0, 33333333), (0, 66666666), (0, 99999999), (0, 133333332)]
    assert s.boundary(29) == (0, 999999990) and s.boundary(30) == (1, 33333323)
    # the reference's loop makes the same chain from its first event
    msgs, tail = S.repack(*ev(0, 33333333, 66666666, 99999999, sec=0), 30.0)
    assert [m[0] for m in msgs] == [(0, 33333333), (0, 66666666), (0, 99999999)] and tail == [3]


def test_the_1000_hz_chain_by_hand():
    s = S.Slicer(1000.0, origin=O1K)
    assert [s.boundary(k) for k in range(3)] == [(10, 1000500), (10, 2000500), (10, 3000500)]
    assert s.boundary(998) == (10, 999000500) and s.boundary(999) == (11, 500)


def test_a_stamp_on_the_boundary_closes_and_one_ns_below_does_not():
    cuts, windows, E, tail = S.slice_windows(*ev(500, 1000500), 1000.0)
    assert (cuts, windows, E, tail) == ([1], [[0]], [(10, 1000500)], [1])
    cuts, windows, E, tail = S.slice_windows(*ev(500, 1000499), 1000.0)
    assert (cuts, windows, E, tail) == ([], [], [], [0, 1])
    # the reference's loop: the same, by its >=
    assert S.repack(*ev(500, 1000500), 1000.0) == ([((10, 1000500), [0])], [1])
    assert S.repack(*ev(500, 1000499), 1000.0) == ([], [0, 1])


def test_a_step_back_across_a_boundary_stays_in_the_open_window():
    sec, nsec = ev(500, 1000600, 900000, 2000500)
    cuts, windows, E, tail = S.slice_windows(sec, nsec, 1000.0)
    assert cuts == [1, 3] and windows == [[0], [1, 2]] and tail == [3]
    assert E == [(10, 1000500), (10, 2000500)]
    assert S.repack(sec, nsec, 1000.0) == ([((10, 1000500), [0]), ((10, 2000500), [1, 2])], [3])


def test_an_event_before_an_explicit_origin_belongs_to_window_0():
    cuts, windows, E, tail = S.slice_windows(*ev(100, 500, 1000400, 1000500), 1000.0, origin=O1K)
    assert cuts == [3] and windows == [[0, 1, 2]] and tail == [3]


def test_a_three_window_gap_and_where_the_reference_differs():
    """events at +0, +3.0001 ms, +3.0002 ms, +3.0003 ms of the origin.  The rule: the second event lies behind E_0, E_1
    and E_2, so it closes three windows — two of them empty — and windows 0..2 keep true end stamps.  The reference
    advances ONE window per event: its message stamped E_1 holds an event from behind E_2, its message stamped E_2 another
    one, and the window it has open at the end is stamped E_3."""
    sec, nsec = ev(500, 3000600, 3000700, 3000800)
    cuts, windows, E, tail = S.slice_windows(sec, nsec, 1000.0)
    assert cuts == [1, 1, 1] and windows == [[0], [], []] and tail == [1, 2, 3]
    assert E == [(10, 1000500), (10, 2000500), (10, 3000500)]
    msgs, rtail = S.repack(sec, nsec, 1000.0)
    assert msgs == [((10, 1000500), [0]), ((10, 2000500), [1]), ((10, 3000500), [2])] and rtail == [3]


def test_the_call_range_and_the_unchanged_state_after_a_failure():
    s = S.Slicer(1000.0)
    far = 1000500 + 4096 * 1000000  # E_4096 of the chain from (10, 500): the last boundary of the first call's range
    with pytest.raises(ValueError):
        s.push([10, 10 + far // 10**9], [500, far % 10**9])
    assert (s.seen, s.m, s.open, s.origin) == (False, 0, 0, None)
    cuts, info = s.push([10, 10 + (far - 1) // 10**9], [500, (far - 1) % 10**9])
    assert cuts == [1] * 4096 and info["closed"] == 4096 and info["open_events"] == 1
    assert info["first"] == (10, 1000500) and info["last"] == (14, 96000500)


def _nojump_stream(rng, n, frequency, back):
    period = 1e9 / frequency
    step = rng.integers(0, int(0.9 * period), n)
    step[rng.random(n) < 0.25] = 0
    b = (rng.random(n) < 0.2) & back
    b[0] = False
    step[b] = 0  # (an event that steps back adds nothing to the running maximum the next one steps from)
    ns = int(rng.integers(1, 3000)) * 10**9 + int(rng.integers(0, 10**9)) + np.cumsum(step)
    ns[b] -= rng.integers(0, int(1.5 * period), int(b.sum()))
    return ns // 10**9, ns % 10**9


@pytest.mark.parametrize("frequency", [30.0, 1000.0, 7.3])
@pytest.mark.parametrize("back", [False, True])
def test_both_loops_agree_where_no_event_jumps_a_window(frequency, back):
    rng = np.random.default_rng(int(frequency * 10) + back)
    for _ in range(6):
        sec, nsec = _nojump_stream(rng, 300, frequency, back)
        cuts, windows, E, tail = S.slice_windows(sec, nsec, frequency)
        assert len(cuts) > 20
        assert all(b > a for a, b in zip(cuts, cuts[1:]))  # no event closes two windows: the no-jump condition
        msgs, rtail = S.repack(sec, nsec, frequency)
        assert [m[0] for m in msgs] == E and [m[1] for m in msgs] == windows and rtail == tail


def test_slicing_in_parts_equals_slicing_the_whole():
    rng = np.random.default_rng(5)
    sec, nsec = _nojump_stream(rng, 40, 30.0, True)
    nsec[25:] += 200000000  # a gap of several windows as well
    sec, nsec = sec + nsec // 10**9, nsec % 10**9
    whole, winfo = S.Slicer(30.0).push(sec, nsec)
    for cut in range(0, 41):
        s = S.Slicer(30.0)
        a, ia = s.push(sec[:cut], nsec[:cut])
        b, ib = s.push(sec[cut:], nsec[cut:])
        assert a + [c + cut for c in b] == whole
        assert ib["count"] == winfo["count"] and ib["open_events"] == winfo["open_events"]
    f = s.flush()
    assert f["closed"] == 1 and f["first_window"] == winfo["count"] and f["open_events"] == 0


GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "repack_ref_*.npz")))


def test_the_recordings_are_there():
    assert len(GOLDEN) == 4


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_repack_equals_the_reference_tools_recorded_messages(path):
    z = np.load(path)
    frequency = float(z["frequency"])
    for t in range(4):
        sec, nsec = z["t%d_sec" % t], z["t%d_nsec" % t]
        msgs, tail = S.repack(sec, nsec, frequency)
        hdr, cnt, ids = z["t%d_header_stamp" % t], z["t%d_count" % t], z["t%d_events" % t]
        assert [list(m[0]) for m in msgs] == hdr.tolist()
        assert np.array_equal(hdr, z["t%d_bag_stamp" % t])  # bag->write is given the header stamp
        assert [len(m[1]) for m in msgs] == cnt.tolist()
        assert [i for m in msgs for i in m[1]] == ids.tolist()
        assert len(tail) == len(sec) - int(cnt.sum()) and len(tail) > 0  # the tail is never written
        # and where the file's streams jump no window, the project's rule gives the recorded messages too
        cuts, windows, E, wtail = S.slice_windows(sec, nsec, frequency)
        if "nojump" in path:
            assert [list(e) for e in E] == hdr.tolist() and [len(w) for w in windows] == cnt.tolist() and wtail == tail
        else:
            assert [len(w) for w in windows] != cnt.tolist()  # the gaps: the tool's windows lag, the rule's do not
