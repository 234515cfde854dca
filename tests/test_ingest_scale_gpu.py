"""GPU: the ingest chains at recording-sized calls — more tiles than the top scan has lanes, where a lane folds two or
three summaries, lanes own none and the last lane must still hold the whole call — against the restatements, every
output bit: records and flags, counts, the state behind the call (through a small second call made on it).  The inputs
are tests/ingest_scale_cases.py's; tests/test_ingest_scale_cases.py shows on the CPU what they contain.  Every length
comes from the library's taps (the tile sizes and esvio_fe_scan_lanes), which must be the values the CPU module is about."""
import ctypes as C

import numpy as np
import pytest

import ba_filter_ref as F
import bow_create_ref as BC
import evt21_ref as R21
import ingest_scale_cases as K
import text_ref as T
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, EventFields

pytestmark = pytest.mark.gpu

KINDS = ("S", "S+1", "2S+1")
FMTS = (K.EVT3, K.EVT2, K.EVT21)
W, H = K.FILTER_W, K.FILTER_H


@pytest.fixture(scope="module")
def geo():
    """chain -> (lanes of the top scan, tile) from the library"""
    L, s, t = FE.load_library(), FE.scan_lanes(), FE.text_limits()
    g = {"raw": (s.raw, L.esvio_fe_raw_tile_bytes()), "aedat": (s.aedat, L.esvio_fe_aedat_tile_events()), "text": (s.text, t.tile_bytes),
         "slice": (s.slice, L.esvio_fe_slice_tile_events()), "filter": (s.filter, s.filter_block_events), "pick": (s.pick, s.pick_tile_values)}
    assert g == K.geometry()   # the CPU module's evidence is about these values
    return g


@pytest.fixture(scope="module")
def ft():
    t = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    yield t
    t.close()


@pytest.fixture(scope="module")
def memo():
    """each case and its expectation are computed once per module"""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]
    return get


def tiles_of(geo, chain, kind):
    return K.tile_counts(geo[chain][0])[kind]


def same_records(got, want, tag):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert len(got) == len(want), (tag, len(got), len(want))
    if got.tobytes() != want.tobytes():
        size = want.shape[1] if want.ndim == 2 else want.dtype.itemsize
        i = int(np.flatnonzero((got.view(np.uint8).reshape(-1, size) != want.view(np.uint8).reshape(-1, size)).any(axis=1))[0])
        raise AssertionError((tag, "first differing record", i, got[i], want[i], len(want)))


# ---- raw -------------------------------------------------------------------------------------------------------------------
def check_raw(ft, cam, fmt, words, want, tag):
    """one decode_raw and one decode_triggers call over `words` against the restatement's (records, info) pairs"""
    (rec, wi), (trig, ti) = want["events"], want["triggers"]
    got, info = ft.decode_raw(cam, fmt, words, dst_cap=len(rec))    # room for the restatement's count, not for the bound
    for k in ("events", "untimed", "other", "bad", "wraps"):
        assert getattr(info, k) == wi[k], (tag, k, getattr(info, k), wi[k])
    assert (info.first_t_us, info.last_t_us) == (wi["first_t_us"], wi["last_t_us"]), tag
    same_records(got, rec, (tag, "events"))
    got, info = ft.decode_triggers(cam, fmt, words, dst_cap=len(trig))
    assert (info.triggers, info.untimed, info.bad, info.wraps) == (ti["triggers"], ti["untimed"], ti["bad"], ti["wraps"]), (tag, "triggers")
    assert (info.first_t_us, info.last_t_us) == (ti["first_t_us"], ti["last_t_us"]), tag
    same_records(got.view(R21.TRIGGER_DTYPE), trig, (tag, "triggers"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_raw_events_and_triggers(ft, geo, memo, fmt, kind):
    c = memo(("raw", fmt, kind), lambda: K.raw_case(fmt, tiles_of(geo, "raw", kind), *geo["raw"]))
    e = memo(("raw expect", fmt, kind), lambda: K.raw_expect(c))
    ft.decode_reset()
    check_raw(ft, 0, fmt, c["words"], e["words"], (fmt, kind, "the big call from the fresh state"))
    check_raw(ft, 0, fmt, c["follow"], e["follow"], (fmt, kind, "the small call on the state it left"))


def test_raw_second_emit_into_grown_buffers(geo):
    """S + 1 tiles of EVT2.1 words that hold more records than words: the first emit launch finds the one-record-per-word
    buffers of a new handle too small, the second one runs from the prefixes the scan left"""
    c = K.raw_case(K.EVT21, tiles_of(geo, "raw", "S+1"), *geo["raw"], dense=True)
    e = K.raw_expect(c)
    rec, wi = e["words"]["events"]
    assert len(rec) > len(c["words"])
    t = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    try:
        t.set_profiling(True)
        got, info = t.decode_raw(0, K.EVT21, c["words"], dst_cap=len(rec))
        assert t.kernel_stats(stages=True)["k_raw_emit"]["launches"] == 2 and t.kernel_stats(stages=True)["k_raw_scan"]["launches"] == 1
        assert (info.events, info.untimed, info.other, info.bad, info.wraps) == (wi["events"], wi["untimed"], wi["other"], 0, wi["wraps"])
        assert (info.first_t_us, info.last_t_us) == (wi["first_t_us"], wi["last_t_us"])
        same_records(got, rec, "second emit")
        got, info = t.decode_raw(0, K.EVT21, c["follow"], dst_cap=len(e["follow"]["events"][0]))
        same_records(got, e["follow"]["events"][0], "behind the second emit")
    finally:
        t.close()


def test_raw_two_cameras_in_one_call(geo, memo):
    """esvio_fe_track_raw: S + 1 tiles in the left camera, 3 in the right — the scan's two workgroups at different widths;
    the counts of both, and each camera's carried state through a small decode call"""
    fmt = K.EVT2
    left = memo(("raw", fmt, "S+1"), lambda: K.raw_case(fmt, tiles_of(geo, "raw", "S+1"), *geo["raw"]))
    right = K.raw_plain(fmt, 3, geo["raw"][1])
    st = [R21.fresh_state(), R21.fresh_state()]
    want = [R21.decode(fmt, c["words"], s) for c, s in zip((left, right), st)]
    t = FE.FeatureTracker(FE.make_config(346, 260, max_cnt=150))   # (every event lies inside its 64 x 48 corner)
    try:
        info, raw = t.track_raw(fmt, left["words"], right["words"], 0, True)
        for cam in (0, 1):
            wi = want[cam][1]
            assert (raw[cam].events, raw[cam].untimed, raw[cam].other, raw[cam].bad, raw[cam].wraps) == \
                (wi["events"], wi["untimed"], wi["other"], 0, wi["wraps"]), cam
            assert (raw[cam].first_t_us, raw[cam].last_t_us) == (wi["first_t_us"], wi["last_t_us"]), cam
            assert info.kept[cam] == wi["events"]   # (every event lies on the sensor and no filter is set)
        for cam, c in ((0, left), (1, right)):
            rec, wi = R21.decode(fmt, c["follow"], st[cam])
            got, ri = t.decode_raw(cam, fmt, c["follow"], dst_cap=len(rec))
            assert (ri.events, ri.wraps) == (wi["events"], wi["wraps"]) and len(rec) >= 4
            same_records(got, rec, ("the carried state of camera", cam))
    finally:
        t.close()


# ---- AEDAT -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_aedat(ft, geo, memo, kind):
    c = memo(("aedat", kind), lambda: K.aedat_case(tiles_of(geo, "aedat", kind), *geo["aedat"]))
    e = memo(("aedat expect", kind), lambda: K.aedat_expect(c))
    ft.decode_reset()
    for name, (rec, o) in zip(("data", "follow"), e):
        got, info = ft.decode_aedat(0, c[name], dst_cap=len(rec))
        assert (info.events, info.invalid, info.bad, info.polarity_packets, info.other_packets) == \
            (len(rec), o["invalid"], 0, o["polarity_packets"], o["other_packets"]), (kind, name)
        assert (info.first_t_us, info.last_t_us) == (o["ticks"][0] // 1000, o["ticks"][-1] // 1000), (kind, name)
        same_records(got, rec, (kind, name))


# ---- text --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,late", [(k, False) for k in KINDS] + [("2S+1", True)])
def test_text(ft, geo, memo, kind, late):
    c = memo(("text", kind, late), lambda: K.text_case(tiles_of(geo, "text", kind), *geo["text"], late=late))
    e = memo(("text expect", kind, late), lambda: K.text_expect(c))
    ft.decode_reset()
    for name, (rec, wi, _) in zip(("data", "follow"), e):
        got, info = ft.decode_text(0, T.TXYP, T.SEC_DECIMAL, c[name], flags=T.SKIP_MALFORMED, dst_cap=len(rec))
        for k in ("events", "lines", "comments", "blank", "malformed", "bad", "carried"):
            assert getattr(info, k) == wi[k], (kind, late, name, k, getattr(info, k), wi[k])
        if wi["first_malformed"] is not None:
            assert info.first_malformed == wi["first_malformed"], (kind, late, name)
        assert (info.first_t_ns, info.last_t_ns) == (wi["first_t_ns"], wi["last_t_ns"]), (kind, late, name)
        same_records(got, rec, (kind, late, name))


# ---- slicing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [False, True], ids=["fixed rate", "given stamps"])
@pytest.mark.parametrize("kind", KINDS)
def test_slice(ft, geo, memo, kind, at):
    c = memo(("slice", kind), lambda: K.slice_case(tiles_of(geo, "slice", kind), *geo["slice"]))
    e = memo(("slice expect", kind, at), lambda: K.slice_expect(c, at))
    ft.slice_reset()
    for name, (cuts, wi, bounds) in zip(("ev", "follow"), e):
        if at:
            got, info = ft.slice_events_at(0, c[name], bounds)
        else:
            got, info = ft.slice_events(0, c[name], K.SLICE_FREQ, K.SLICE_ORIGIN)
        assert got.tolist() == cuts, (kind, at, name)
        assert (info.closed, info.first_window, info.count, info.open_events) == \
            (wi["closed"], wi["first_window"], wi["count"], wi["open_events"]), (kind, at, name)
        assert (info.first_sec, info.first_nsec) == wi["first"] and (info.last_sec, info.last_nsec) == wi["last"], (kind, at, name)


# ---- the filter ------------------------------------------------------------------------------------------------------------------
def filter_call(ft, ev, prm, fields):
    """esvio_fe_filter_batch into host memory -> (kept records, flags, the last kept record, rejected)"""
    L, n = ft._hd.L, len(ev)
    keep = None
    if fields:
        t = ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"].astype(np.int64)
        keep = EventFields.from_arrays(ev["x"].copy(), ev["y"].copy(), t, ev["polarity"].astype(np.int8), t_unit_ns=1)
        desc = FE.fields_desc(keep)
        ptr, fptr = None, C.byref(desc)
    else:
        ptr, fptr = FE._p(ev), None
    out, flags, last = np.zeros(n, EVENT_DTYPE), np.zeros(n, np.uint8), np.zeros(1, EVENT_DTYPE)
    nk, rej, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.esvio_fe_filter_batch(ft._hd.h, 0, ptr, fptr, n, FE.HOST, C.byref(prm), FE._p(out), FE.HOST, C.byref(nk), FE._p(flags),
                                 FE._p(last), C.byref(rej), C.byref(bad))
    assert rc == 0 and bad.value == 0, (rc, L.esvio_fe_last_error(ft._hd.h))
    return out[:int(nk.value)], flags, last, int(rej.value)


@pytest.mark.parametrize("kind,fields,refractory", [("S", False, False), ("S+1", False, True), ("S", True, True), ("S+1", True, False)],
                         ids=["S records", "S+1 records refractory", "S fields refractory", "S+1 fields"])
def test_filter(ft, geo, memo, kind, fields, refractory):
    c = memo(("filter", kind), lambda: K.filter_case(tiles_of(geo, "filter", kind), *geo["filter"]))
    flags, rej, B = memo(("filter expect", kind, refractory), lambda: K.filter_expect(c, refractory))
    prm = FE.FilterParams(K.FILTER_WINDOW_NS, 1, K.FILTER_REFRACTORY_NS if refractory else 0)
    ev = c["ev"]
    ft.filter_reset()
    kept, got, last, n_rej = filter_call(ft, ev, prm, fields)
    assert n_rej == rej and np.array_equal(got, flags), (kind, np.flatnonzero(got != flags)[:5])
    want = F.raw_records(ev)[flags != 0]   # (rows of 16 bytes: numpy's own copies of the records drop the padding)
    same_records(F.raw_records(kept), want, kind)
    assert F.raw_records(last).tobytes() == want[-1:].tobytes()
    # the plane behind the call: the last events again, stamped behind it — the first of them has support from the carried plane alone
    more = F.raw_records(ev)[-1500:].copy().view(EVENT_DTYPE).reshape(-1)
    t = (ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"])[-1500:]
    t = t - t[0] + t[-1] + 2000
    more["sec"], more["nsec"] = t // 10 ** 9, t % 10 ** 9
    B2 = B.copy()
    flags2, rej2 = K.filter_fast(B2, W, H, more, prm.window_ns, 1, prm.refractory_ns)
    assert flags2[0] == 1
    kept, got, last, n_rej = filter_call(ft, more, prm, fields)
    assert n_rej == rej2 and np.array_equal(got, flags2)
    same_records(F.raw_records(kept), F.raw_records(more)[flags2 != 0], (kind, "second call"))


# ---- the seeding pick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_pick(ft, geo, memo, kind):
    c = memo(("pick", kind), lambda: K.pick_case(tiles_of(geo, "pick", kind), *geo["pick"]))
    for cuts in K.PICK_KINDS:
        cut = K.pick_cuts(c, cuts)
        want = BC.pick_ref(c["md"], c["seg_off"], cut)
        got = ft.bow_create_pick(c["md"], c["seg_off"], cut)
        assert np.array_equal(got, want), (kind, cuts, got, want)
