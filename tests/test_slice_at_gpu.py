"""GPU: esvio_fe_slice_events_at (windows that end at given stamps) against the sequential reading of its rule,
tests/slice_at_ref.py (SlicerAt.push).  Integers only: every cut entry and every esvio_fe_slice_info field is compared for
equality.  T is the slice chain's tile in events (esvio_fe_slice_tile_events).  Last, one end-to-end case: an EVT3 stream
with trigger words -> triggers -> events -> windows at the triggers' stamps -> each window tracked."""
import ctypes as C

import numpy as np
import pytest

import evt21_ref as E
import slice_at_ref as SA
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5A5A5A5A5
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


def tile():
    return FE.load_library().esvio_fe_slice_tile_events()


def records(ns):
    """stamps in integer nanoseconds -> EVENT_DTYPE records (x, y count the events)"""
    ns = np.asarray(ns, np.int64)
    ev = np.zeros(len(ns), EVENT_DTYPE)
    ev["x"], ev["y"] = np.arange(len(ns)) & 0xffff, np.arange(len(ns)) >> 16
    ev["sec"], ev["nsec"], ev["polarity"] = ns // 10**9, ns % 10**9, np.arange(len(ns)) & 1
    return ev


def pairs(ns):
    return [(int(v) // 10**9, int(v) % 10**9) for v in ns]


class SlAt:
    """a handle and the restatement's explicit-mode slicers of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.fresh()

    def fresh(self, how="slice_reset"):
        getattr(self.ft, how)()
        self.ref = [SA.SlicerAt(), SA.SlicerAt()]

    def close(self):
        self.ft.close()

    def call(self, cam, ev, bounds, space=FE.HOST, cuts_cap=FE.SLICE_MAX_WINDOWS, extra=3):
        """one esvio_fe_slice_events_at call -> (rc, cuts array of cuts_cap + extra entries, SliceInfo)"""
        ev = np.ascontiguousarray(ev)
        b = np.zeros(len(bounds), EVENT_DTYPE)
        if len(bounds):
            b["sec"], b["nsec"] = [p[0] for p in bounds], [p[1] for p in bounds]
            b["x"], b["y"], b["polarity"] = 0xFFFF, 0xFFFF, 0xFF  # (only sec / nsec are read)
        info = FE.SliceInfo(first_sec=71, first_nsec=72, last_sec=73, last_nsec=74)
        cuts = np.full(cuts_cap + extra, GUARD, np.uint64)
        dsrc = None
        src = C.c_void_p(ev.ctypes.data if len(ev) else 0)
        if space == FE.DEVICE:
            dsrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, max(ev.nbytes, 16), C.byref(dsrc)) == 0
            if ev.nbytes:
                assert self.L.esvio_fe_mem_upload(dsrc, C.c_void_p(ev.ctypes.data), ev.nbytes) == 0
            src = dsrc
        rc = self.L.esvio_fe_slice_events_at(self.h, cam, src, len(ev), space, C.c_void_p(b.ctypes.data if len(b) else 0), len(b),
                                             C.c_void_p(cuts.ctypes.data), cuts_cap, C.byref(info))
        if dsrc is not None:
            self.L.esvio_fe_mem_free(FE.DEVICE, dsrc)
        return rc, cuts, info

    def check(self, cam, ev, bounds, space=FE.HOST, tag=None, exact_cap=False):
        """a call that succeeds equals the restatement, which advances with it -> (cuts, info of the restatement)"""
        want, wi = self.ref[cam].push(ev["sec"], ev["nsec"], bounds)
        cap = len(want) if exact_cap else FE.SLICE_MAX_WINDOWS
        rc, cuts, info = self.call(cam, ev, bounds, space, cap)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        assert cuts[:len(want)].tolist() == want, (tag, cuts[:len(want)].tolist()[:8], want[:8])
        assert (cuts[len(want):] == GUARD).all(), (tag, "entries behind the closed windows or behind cuts_cap touched")
        self.same_info(info, wi, tag)
        return want, wi

    @staticmethod
    def same_info(info, wi, tag=None):
        got = (info.closed, info.first_window, info.count, info.open_events)
        assert got == (wi["closed"], wi["first_window"], wi["count"], wi["open_events"]), (tag, got, wi)
        stamps = (info.first_sec, info.first_nsec, info.last_sec, info.last_nsec)
        assert stamps == (wi["first"] + wi["last"] if wi["closed"] else (71, 72, 73, 74)), (tag, stamps, wi)


@pytest.fixture(scope="module")
def sl():
    s = SlAt()
    yield s
    s.close()


BASE = 10 * 10**9 + 500


def stepped(n, T):
    """steps of 100 ns, and a millisecond more at the middle and the last event of tile 0, the first of tile 1 and
    inside tile 2 — the ones that exist at this length"""
    ns = BASE + 100 * np.arange(n, dtype=np.int64)
    for at in (T // 2, T - 1, T, 2 * T + 2):
        if at < n:
            ns[at:] += 1000000
    return ns


@pytest.mark.parametrize("space", [FE.HOST, FE.DEVICE])
def test_lengths_around_the_tile_edges(sl, space):
    T = tile()
    assert T == 1024
    for n in (1, T - 1, T, T + 1, 3 * T):
        ns = stepped(n, T)
        # a boundary at each step's first event (the event ON it closes the window), one inside tile 2 twice, one never reached
        at = [a for a in (T // 2, T - 1, T, 2 * T + 2) if a < n]
        b = sorted([int(ns[a]) for a in at] + ([int(ns[2 * T + 2])] if 2 * T + 2 < n else []) + [int(ns[-1]) + 1])
        sl.fresh()
        want, wi = sl.check(0, records(ns), pairs(b), space=space, tag=("n", n), exact_cap=n != T)
        assert want == sorted(at + ([2 * T + 2] if 2 * T + 2 < n else []))
        assert wi["open_events"] == n - (want[-1] if want else 0)


def test_no_boundaries_duplicates_an_event_on_a_boundary_and_back_steps(sl):
    T = tile()
    ns = BASE + 1000 * np.arange(T + 40, dtype=np.int64)
    ev = records(ns)
    sl.fresh()
    want, wi = sl.check(0, ev, [], tag="no boundaries at all")
    assert want == [] and wi["open_events"] == T + 40
    want, wi = sl.check(0, ev[:5], [], tag="... twice: the open window keeps counting")
    assert wi["open_events"] == T + 45
    # duplicates give empty windows; an event exactly on a boundary closes the window, one 1 ns in front of it does not
    sl.fresh()
    b = [int(ns[3]), int(ns[3]), int(ns[3]), int(ns[T - 1]) + 1, int(ns[T]), int(ns[T]) + 1, int(ns[T + 1])]
    want, wi = sl.check(1, ev, pairs(b), tag="duplicates, on and beside a boundary")
    assert want == [3, 3, 3, T, T, T + 1, T + 1]
    # back-steps stay in the open window: m is a prefix maximum
    back = ns.copy()
    back[T - 2:T + 3] = [ns[T + 20], ns[2], ns[T + 20] + 1, ns[1], ns[0]]
    sl.fresh()
    want, wi = sl.check(0, records(back), pairs([int(ns[5]), int(ns[T + 20]), int(ns[T + 20]) + 1, int(ns[T + 39]) + 7]), space=FE.DEVICE,
                        tag="back-steps")
    assert want == [5, T - 2, T] and wi["open_events"] == 40
    # stamps whose double is the same as the boundary's although the integers differ by less than an ulp are equal: toSec
    sl.fresh()
    big = 4_000_000_000 * 10**9
    want, wi = sl.check(0, records([big + 100, big + 101, big + 900]), pairs([big + 101, big + 600]), tag="toSec")
    assert want == SA.slice_at([4_000_000_000] * 3, [100, 101, 900], pairs([big + 101, big + 600]))[0]


def test_4096_boundaries_and_the_refusals(sl):
    T = tile()
    n = T + 9
    ns = BASE + 10_000 * np.arange(n, dtype=np.int64)
    ev = records(ns)
    b = pairs(BASE + 2_000 * np.arange(4096, dtype=np.int64) + 1)  # five boundaries between two events: all 4096 inside the first 820
    sl.fresh()
    want, wi = sl.check(0, ev, b, tag="4096 boundaries", exact_cap=True)
    assert wi["closed"] == 4096 and wi["open_events"] == n - want[-1]
    # one event that jumps all 4096 of them
    sl.fresh()
    want, wi = sl.check(1, records([BASE, BASE + 10**9]), b, tag="one jump over 4096")
    assert want == [1] * 4096
    # refusals leave the state as it was
    sl.fresh()
    sl.check(0, ev[:10], b[:2], tag="before")
    before = (sl.ref[0].m, sl.ref[0].open)
    rc, cuts, info = sl.call(0, ev[10:], b + [b[-1]])
    assert rc == -1 and b"4096" in sl.L.esvio_fe_last_error(sl.h) and (cuts == GUARD).all()
    rc, cuts, info = sl.call(0, ev[10:], [b[9], b[8]])
    assert rc == -1 and b"decrease" in sl.L.esvio_fe_last_error(sl.h)
    rc, cuts, info = sl.call(0, ev[10:], b[2:], cuts_cap=7)
    assert rc == -1 and info.closed == 4094 and (cuts == GUARD).all()
    assert sl.L.esvio_fe_slice_events_at(sl.h, 2, None, 0, FE.HOST, None, 0, None, 0, None) == -1
    assert sl.L.esvio_fe_slice_events_at(sl.h, 0, None, 5, FE.HOST, None, 0, None, 0, None) == -1
    assert sl.L.esvio_fe_slice_events_at(sl.h, 0, FE._p(ev), 5, 7, None, 0, None, 0, None) == -1
    assert sl.L.esvio_fe_slice_events_at(sl.h, 0, FE._p(ev), 5, FE.HOST, None, 3, None, 0, None) == -1
    rc, _, info = sl.call(0, ev[:0], b[2:])
    assert rc == 0 and (info.closed, info.count, info.open_events) == (0,) + before
    assert (sl.ref[0].m, sl.ref[0].open) == before
    sl.check(0, ev[10:], b[2:], tag="after the refusals: the same events with room")


def test_two_calls_with_the_rest_of_the_boundaries_equal_one_call(sl):
    T = tile()
    rng = np.random.default_rng(3)
    n = 2 * T + 77
    t = BASE + np.sort(rng.integers(0, 50_000_000, n))
    t[rng.integers(1, n, 12)] -= 400_000  # back-steps
    bnd = np.sort(rng.integers(-1_000_000, 52_000_000, 60)) + BASE
    bnd[20] = bnd[19]
    bnd[30] = t[T]
    bnd = np.sort(bnd)
    ev, b = records(t), pairs(bnd)
    whole, wi = SA.SlicerAt().push(ev["sec"], ev["nsec"], b)
    assert 30 < wi["closed"] <= 60
    cuts = [1, T - 1, T, T + 1, 2 * T, n - 1] + [int(c) for c in rng.integers(2, n - 1, 14)]
    for i, cut in enumerate(cuts):
        sl.fresh()
        space = (FE.HOST, FE.DEVICE)[i % 2]
        c1, i1 = sl.check(0, ev[:cut], b, space=space, tag=(cut, "first"))
        c2, i2 = sl.check(0, ev[cut:], b[i1["closed"]:], space=space, tag=(cut, "second"))
        assert c1 + [c + cut for c in c2] == whole and (i2["count"], i2["open_events"]) == (wi["count"], wi["open_events"]), cut


def test_mixing_modes_is_refused_until_reset_and_flush_in_explicit_mode(sl):
    ev = records(BASE + 1000 * np.arange(50, dtype=np.int64))
    b = pairs([BASE + 5000, BASE + 20000])
    for how in ("slice_reset", "reset"):
        sl.fresh(how)
        sl.check(0, ev, b, tag="explicit first")
        with pytest.raises(FE.FrontendError, match="given stamps"):
            sl.ft.slice_events(0, ev, 1000.0)
        cuts, info = sl.ft.slice_events(1, ev, 100000.0)  # the other camera is free to be fixed-rate
        assert info.closed > 0
        rc, cuts, _ = sl.call(1, ev, b)
        assert rc == -1 and b"fixed-rate" in sl.L.esvio_fe_last_error(sl.h) and (cuts == GUARD).all()
        sl.check(0, ev[:3], b[2:], tag="the explicit camera goes on")
        # flush in explicit mode: the open window closes, it has no boundary: the stamp fields stay
        info = FE.SliceInfo(first_sec=71, first_nsec=72, last_sec=73, last_nsec=74)
        assert sl.L.esvio_fe_slice_flush(sl.h, 0, C.byref(info)) == 0
        wi = sl.ref[0].flush()
        assert (info.closed, info.first_window, info.count, info.open_events) == (wi["closed"], wi["first_window"], wi["count"], wi["open_events"]) == (1, 2, 3, 0)
        assert (info.first_sec, info.first_nsec, info.last_sec, info.last_nsec) == (71, 72, 73, 74)
        sl.check(0, ev, pairs([BASE + 7000]), tag="behind the flush: window 3 ends at the next boundary given")
    sl.fresh()
    cuts, info = sl.ft.slice_events(0, ev, 1000.0)  # after the reset either mode may come first
    sl.fresh()
    # while a feed is open the slicer is the feed's
    sl.ft.feed_open(30.0)
    rc, _, _ = sl.call(0, ev, b)
    assert rc == -1 and b"feed" in sl.L.esvio_fe_last_error(sl.h)
    sl.ft.feed_close()
    # the Python layer takes trigger records, event records or pairs as boundaries
    sl.fresh()
    trg = np.zeros(2, FE.TRIGGER_DTYPE)
    trg["sec"], trg["nsec"] = [p[0] for p in b], [p[1] for p in b]
    cuts, info = sl.ft.slice_events_at(0, ev, trg)
    assert cuts.tolist() == [5, 20] and (info.last_sec, info.last_nsec) == b[1]
    cuts, info = sl.ft.slice_events_at(0, ev[:0], [])
    assert info.count == 2
    with pytest.raises(FE.FrontendError) as e:
        sl.ft.slice_events_at(1, ev, [b[1], b[0]])
    assert e.value.info.closed == 0


# ---- end to end --------------------------------------------------------------------------------------------------------
W, H = 346, 260


def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def test_evt3_words_with_triggers_to_windows_at_the_triggers_tracked(sl):
    """both cameras' EVT3 streams carry one trigger word per `frame` (the left camera's stream both edges: only the
    rising ones are boundaries); triggers -> events (device records) -> slice_events_at at the triggers' stamps -> every
    window tracked with track_event from the device records, against tracking the sub-arrays the numpy loop cuts"""
    st = SceneStream(W=W, H=H, rate=4e5, seed=11, n_rect=8, size=(12.0, 30.0))
    base = st.t_us - 1000
    cams = [[], []]
    for _ in range(3):
        left, right, _ = st.next_batch()
        for cam, ev in enumerate((left, right)):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10**6 + ev["nsec"].astype(np.int64) // 1000
            o = E.R.readout_order(x, y, p, t)
            cams[cam].append((x[o], y[o], p[o], t[o] - base))
    words, recs = [], []
    frame_us = 6000
    flat = [[np.concatenate([q[k] for q in cams[cam]]) for k in range(4)] for cam in range(2)]
    frames = int(max(flat[0][3][-1], flat[1][3][-1])) // frame_us + 1  # (the last frame's stamp lies behind every event)
    for cam in range(2):
        x, y, p, t = flat[cam]
        out, lo = [], 0
        for k in range(1, frames + 1):  # the events in front of each frame's stamp, then the frame's trigger word(s) at that stamp
            hi = int(np.searchsorted(t, k * frame_us, side="left"))
            out.append(E.R.encode_evt3(x[lo:hi], y[lo:hi], p[lo:hi], t[lo:hi]))
            tt = k * frame_us
            stamp = [0x8000 | (tt >> 12), 0x6000 | (tt & 0xFFF)]
            out.append(np.array(stamp + [0xA001 | (cam << 8)] + ([0x8000 | ((tt + 4096) >> 12), 0xA000] if cam == 0 else []), "<u2"))
            lo = hi
        assert lo == len(t)
        words.append(np.concatenate(out))
        rec, info = E.decode(E.EVT3, words[cam], E.fresh_state(), base)
        assert info["other"] == frames * (2 - cam) and len(rec) == len(t)
        recs.append(rec)
    a, b = (FE.FeatureTracker(FE.make_config(W, H, max_cnt=60)) for _ in range(2))
    dev = []
    try:
        cut, bounds = [], None
        for cam in range(2):
            trg, ti = a.decode_triggers(cam, E.EVT3, words[cam], base)
            want_trg, _ = E.decode_triggers(E.EVT3, words[cam], E.fresh_state(), base)
            assert trg.tobytes() == want_trg.tobytes() and (trg["id"] == cam).all()
            rising = trg[trg["value"] == 1]
            if cam == 0:
                bounds = rising
                assert len(rising) * 2 == len(trg) >= 8
            else:
                assert (rising["sec"].tolist(), rising["nsec"].tolist()) == (bounds["sec"].tolist(), bounds["nsec"].tolist()), \
                    "both cameras' triggers lie on one time base"
            d, ri = a.decode_raw(cam, E.EVT3, words[cam], base, device=True)
            dev.append(d)
            assert ri.events == len(recs[cam]) and ri.other == ti.triggers + ti.untimed
            cuts, si = a.slice_events_at(cam, d.arg, bounds)
            want_cuts, _, _ = SA.slice_at(recs[cam]["sec"], recs[cam]["nsec"], [(int(s), int(n)) for s, n in zip(bounds["sec"], bounds["nsec"])])
            # (the last frame's stamp lies behind every event: its window stays open)
            assert cuts.tolist() == want_cuts and 8 <= si.closed == len(want_cuts) < len(bounds)
            assert (si.last_sec, si.last_nsec) == (int(bounds["sec"][si.closed - 1]), int(bounds["nsec"][si.closed - 1]))
            cut.append([0] + want_cuts)
        tracked = 0
        for k in range(min(len(cut[0]), len(cut[1])) - 1):
            (l0, l1), (r0, r1) = ((c[k], c[k + 1]) for c in cut)
            if l1 == l0:
                continue
            cur = float(event_times(recs[0][l1 - 1:l1])[0])
            assert cur < float(bounds["sec"][k]) + 1e-9 * float(bounds["nsec"][k])  # the window ends in front of its frame
            a.trackEvent(cur, (dev[0].arg[0] + 16 * l0, l1 - l0), (dev[1].arg[0] + 16 * r0, r1 - r0), k % 2 == 0)
            b.trackEvent(cur, recs[0][l0:l1], recs[1][r0:r1], k % 2 == 0)
            assert results(a) == results(b), k
            tracked += 1
        assert tracked >= 8 and len(a.ids) > 0
    finally:
        for d in dev:
            d.free()
        a.close()
        b.close()
