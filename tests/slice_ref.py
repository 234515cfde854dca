"""The stream-slicing rule of include/esvio_fe.h (esvio_fe_slice_events), read sequentially, beside the reference's own
loop as it is written (dependences/events_repacking_helper/src/EventMessageEditor.cpp: insertEvent / resetBuffer).

Stamps are (sec, nsec) pairs of integers; toSec is two roundings and no FMA (plain Python floats: CPython contracts
nothing); Time() is roscpp's ros::Time::fromSec RESTATED FROM RECALL — floor, round half away from zero, carry.  The
control flow of repack() is pinned by recordings of the reference's compiled code (tests/golden/repack_ref_*.npz); the
rounding of Time() is not: the recordings were made against a stand-in ros::Time that restates it the same way."""
import math

MAX_WINDOWS = 4096  # ESVIO_FE_SLICE_MAX_WINDOWS


def to_sec(sec, nsec):
    return float(sec) + 1e-9 * float(nsec)


def time_from_sec(d):
    fl = math.floor(d)
    x = (d - float(fl)) * 1e9
    r = math.floor(x)
    if x - float(r) >= 0.5:  # (exact: x and floor(x) are neighbours) halves away from zero
        r += 1
    sec, nsec = int(fl), int(r)
    if nsec >= 1000000000:
        sec, nsec = sec + 1, nsec - 1000000000
    return sec, nsec


def repack(sec, nsec, frequency):
    """EventMessageEditor over one topic: returns (messages, tail) — messages = [((sec, nsec) header stamp, [event
    indices])] in the order bag->write is called, tail = the events left in eArray_ when the input ends (never written)."""
    duration_threshold = 1 / frequency
    first_message = True
    end_time, stamp, events, messages = None, None, [], []

    def reset_buffer(start):
        nonlocal end_time, stamp, events
        end_time = time_from_sec(to_sec(*start) + duration_threshold)
        events = []
        stamp = end_time

    for i in range(len(sec)):
        ts = (int(sec[i]), int(nsec[i]))
        if first_message:
            reset_buffer(ts)
            first_message = False
        if to_sec(*ts) >= to_sec(*end_time):
            messages.append((stamp, events))
            reset_buffer(end_time)
        events.append(i)
    return messages, events


class Slicer:
    """one camera's slicer state and the rule: push() is one esvio_fe_slice_events call, flush() esvio_fe_slice_flush"""

    def __init__(self, frequency, origin=None):
        assert 1e-3 <= frequency <= 1e6
        self.period = 1.0 / frequency
        self.origin = None if origin is None else (int(origin[0]), int(origin[1]))
        self.seen, self.m, self.open = False, 0, 0  # seen: a call with events has succeeded
        self.E = []

    def boundary(self, k):
        """E_k as (sec, nsec); sec may leave 32 bits: then it is no boundary"""
        while len(self.E) <= k:
            prev = to_sec(*self.E[-1]) if self.E else to_sec(*self.origin)
            self.E.append(time_from_sec(prev + self.period))
        return self.E[k]

    def _info(self, closed, first):
        info = dict(closed=closed, first_window=first, count=self.m, open_events=self.open)
        if closed:
            info["first"], info["last"] = self.boundary(first), self.boundary(first + closed - 1)
        return info

    def push(self, sec, nsec):
        """-> (cuts, info); raises ValueError — the state as it was — when an event lies at or beyond the last boundary
        of the call's range"""
        n = len(sec)
        if n == 0:
            return [], self._info(0, self.m)
        saved = self.origin
        if self.origin is None:
            self.origin = (int(sec[0]), int(nsec[0]))
        m_start, m, cuts = self.m, self.m, []
        for i in range(n):
            ts = to_sec(int(sec[i]), int(nsec[i]))
            c = m_start
            while True:
                e = self.boundary(c)
                if not to_sec(*e) <= ts:
                    break
                c += 1
                if c - m_start > MAX_WINDOWS or e[0] >= 1 << 32:
                    if saved is None:
                        self.origin, self.E = None, []
                    raise ValueError("event %d lies at or beyond the last boundary of the call's range" % i)
            if c > m:
                cuts += [i] * (c - m)
                m = c
        self.seen = True
        self.open = n - cuts[-1] if cuts else self.open + n
        self.m = m
        return cuts, self._info(m - m_start, m_start)

    def flush(self):
        if not self.seen:
            return self._info(0, self.m)
        self.m, self.open = self.m + 1, 0
        return self._info(1, self.m - 1)


def slice_windows(sec, nsec, frequency, origin=None):
    """the rule over a whole stream: (cuts, windows, E, tail) — windows[k] = the event indices of window k for every
    closed window, E[k] its end stamp (sec, nsec), tail = the events of the window left open"""
    s = Slicer(frequency, origin)
    cuts, info = s.push(sec, nsec)
    edges = [0] + cuts
    windows = [list(range(edges[k], edges[k + 1])) for k in range(len(cuts))]
    return cuts, windows, [s.boundary(k) for k in range(len(cuts))], list(range(edges[-1], len(sec)))
