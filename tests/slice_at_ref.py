"""The rule of esvio_fe_slice_events_at (include/esvio_fe.h), read sequentially: windows that end at stamps the caller
gives.  Stamps are (sec, nsec) pairs of integers; toSec is two roundings and no FMA (plain Python floats)."""

MAX_BOUNDS = 4096  # ESVIO_FE_SLICE_MAX_WINDOWS


def to_sec(sec, nsec):
    return float(sec) + 1e-9 * float(nsec)


class SlicerAt:
    """one camera's slicer state in explicit mode: push() is one esvio_fe_slice_events_at call, flush()
    esvio_fe_slice_flush"""

    def __init__(self):
        self.seen, self.m, self.open = False, 0, 0  # seen: a call with events has succeeded

    def push(self, sec, nsec, bounds):
        """bounds: (sec, nsec) pairs, the ends of windows m, m + 1, ...  -> (cuts, info); raises ValueError — the state
        as it was — for more than MAX_BOUNDS boundaries or a decreasing list"""
        bounds = [(int(b[0]), int(b[1])) for b in bounds]
        if len(bounds) > MAX_BOUNDS:
            raise ValueError("too many boundaries")
        b = [to_sec(*k) for k in bounds]
        for k in range(1, len(b)):
            if b[k] < b[k - 1]:
                raise ValueError("boundary %d lies in front of boundary %d" % (k, k - 1))
        n = len(sec)
        m_start, m, cuts = self.m, self.m, []
        if n == 0:
            return [], dict(closed=0, first_window=m_start, count=self.m, open_events=self.open)
        for i in range(n):
            ts = to_sec(int(sec[i]), int(nsec[i]))
            c = m_start
            for bk in b:  # c_i = m_start + #{k : b_k <= ts_i}
                if bk <= ts:
                    c += 1
            if c > m:
                cuts += [i] * (c - m)
                m = c
        self.seen = True
        self.open = n - cuts[-1] if cuts else self.open + n
        self.m = m
        info = dict(closed=m - m_start, first_window=m_start, count=self.m, open_events=self.open)
        if cuts:
            info["first"], info["last"] = bounds[0], bounds[len(cuts) - 1]
        return cuts, info

    def flush(self):
        """closes the open window; it has no boundary: no stamps"""
        if not self.seen:
            return dict(closed=0, first_window=self.m, count=self.m, open_events=self.open)
        self.m, self.open = self.m + 1, 0
        return dict(closed=1, first_window=self.m - 1, count=self.m, open_events=0)


def slice_at(sec, nsec, bounds):
    """the rule over a whole stream from a fresh state: (cuts, windows, tail) — windows[k] the event indices of window k
    for every closed window, tail the events of the window left open"""
    cuts, _ = SlicerAt().push(sec, nsec, bounds)
    edges = [0] + cuts
    return cuts, [list(range(edges[k], edges[k + 1])) for k in range(len(cuts))], list(range(edges[-1], len(sec)))
