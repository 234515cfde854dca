"""GPU: esvio_fe_convert_events (k_events_from_fields) against the numpy restatement tests/event_fields_ref.py, byte
for byte, over the layouts recordings and SDKs deliver, every memory space of source and destination, the sizes at
which a kernel that handles four events per lane with wide loads can go wrong, and shifted bases; bad stamps, bad
descriptors; and esvio_fe_track_event_fields / converted device batches in the replay schedule against trackEvent on
make_events records, bit for bit.  Integers only: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import event_fields_ref as R
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, EventFields, event_times, make_events
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
BIG = 100_003
GUARD = 0xA5
ARENA = R.raw_bytes("", BIG) + 64


class Arenas:
    """one buffer per memory space, reused by every case: pageable, pinned (esvio_fe_mem_alloc), registered
    (esvio_fe_register_host_buffer) and device memory for the sources; device memory for a destination"""

    def __init__(self):
        L = self.L = FE.load_library()
        self.hip = C.CDLL("libamdhip64.so")
        self.pageable = self._aligned(ARENA)
        self.pin_ptr = C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.HOST, ARENA, C.byref(self.pin_ptr)) == 0
        self.pinned = np.ctypeslib.as_array(C.cast(self.pin_ptr, C.POINTER(C.c_uint8)), shape=(ARENA,))
        self.registered = self._aligned(ARENA)
        assert L.esvio_fe_register_host_buffer(C.c_void_p(self.registered.ctypes.data), ARENA) == 0
        self.dev_src, self.dev_dst = C.c_void_p(), C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.DEVICE, ARENA, C.byref(self.dev_src)) == 0
        assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * (BIG + 16), C.byref(self.dev_dst)) == 0
        self.back = self._aligned(16 * (BIG + 16))  # read-back of the device destination

    @staticmethod
    def _aligned(n):
        buf = np.zeros(n + 16, np.uint8)
        o = (-buf.ctypes.data) % 16
        return buf[o:o + n]

    def close(self):
        L = self.L
        L.esvio_fe_unregister_host_buffer(C.c_void_p(self.registered.ctypes.data))
        L.esvio_fe_mem_free(FE.HOST, self.pin_ptr)
        L.esvio_fe_mem_free(FE.DEVICE, self.dev_src)
        L.esvio_fe_mem_free(FE.DEVICE, self.dev_dst)

    def source(self, case, space):
        """the case's bytes in `space` -> (EventFields, src_space)"""
        n = len(case.raw)
        if space == "device":
            assert self.L.esvio_fe_mem_upload(self.dev_src, C.c_void_p(case.raw.ctypes.data), n) == 0
            f = case.fields
            ptrs = [self.dev_src.value + (p - case.raw.ctypes.data) for p in f.ptrs]
            return EventFields.at_pointers(ptrs, f.strides, f.n, f.t_bits, f.p_bits, f.t_unit_ns, f.t_offset), FE.DEVICE
        arena = getattr(self, space)
        arena[:n] = case.raw
        return case.relocate(arena[:n]), FE.HOST

    def read_dst(self, nbytes):
        """the first nbytes of the device destination (hipMemcpy of the runtime the library is linked to)"""
        assert self.hip.hipMemcpy(C.c_void_p(self.back.ctypes.data), self.dev_dst, C.c_size_t(nbytes), 2) == 0
        return self.back[:nbytes]

    def fill_dst(self, nbytes):
        self.back[:nbytes] = GUARD
        assert self.L.esvio_fe_mem_upload(self.dev_dst, C.c_void_p(self.back.ctypes.data), nbytes) == 0


@pytest.fixture(scope="module")
def arenas():
    a = Arenas()
    yield a
    a.close()


@pytest.fixture(scope="module")
def ft():
    t = FE.FeatureTracker(FE.make_config(192, 144, max_cnt=60))
    yield t
    t.close()


_expected = {}


def _case(layout, n, shift):
    """the case and its restatement, computed once per (layout, n, shift)"""
    key = (layout, n, shift)
    if key not in _expected:
        c = R.make_case(layout, n, seed=1000 * len(layout) + n, shift=shift, polarity="pm1" if n % 2 else "mixed")
        ev, bad = R.expected(c)
        assert not bad.any()
        _expected[key] = (c, ev.tobytes())
    return _expected[key]


def _convert(ft, fields, n, src_space, dst, dst_space):
    bad = C.c_uint64(99)
    desc = FE.fields_desc(fields)
    rc = ft._hd.L.esvio_fe_convert_events(ft._hd.h, C.byref(desc), n, src_space, dst, dst_space, C.byref(bad))
    return rc, bad.value


def _check_case(ft, arenas, case, want, space, dst_space, tag):
    n = case.n
    fields, src_space = arenas.source(case, space)
    if dst_space == FE.DEVICE:
        arenas.fill_dst(16 * (n + 2))
        rc, bad = _convert(ft, fields, n, src_space, arenas.dev_dst, FE.DEVICE)
        got = arenas.read_dst(16 * (n + 2))
    else:
        got = arenas.back[:16 * (n + 2)]
        got[:] = GUARD
        rc, bad = _convert(ft, fields, n, src_space, C.c_void_p(got.ctypes.data), FE.HOST)
    assert rc == 0 and bad == 0, (tag, rc, bad, ft._hd.L.esvio_fe_last_error(ft._hd.h))
    rec = got[:16 * n]
    if rec.tobytes() != want:
        g, w = rec.view(EVENT_DTYPE), np.frombuffer(want, EVENT_DTYPE)
        k = int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != w.view(np.uint8).reshape(-1, 16))[0]) // 16
        raise AssertionError((tag, "first differing event", k, g[k], w[k]))
    assert (rec.reshape(-1, 16)[:, 13:] == 0).all(), tag            # _pad
    assert (got[16 * n:] == GUARD).all(), (tag, "bytes beyond n records touched")


def _check(ft, arenas, layout, n, shift, space, dst_space):
    case, want = _case(layout, n, shift)
    _check_case(ft, arenas, case, want, space, dst_space, (layout, n, shift, space, dst_space))


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_convert_equals_restatement(ft, arenas, layout):
    """every size x every shift from device memory into device memory; every size in every source space at shift 0
    and at an odd shift, into both destinations; the large size in every space at two shifts"""
    shifts = R.SHIFTS[layout]
    for n in SIZES:
        for shift in shifts:
            _check(ft, arenas, layout, n, shift, "device", FE.DEVICE)
        for space in ("pageable", "pinned", "registered", "device"):
            for shift in (shifts[0], shifts[3]):
                for dst_space in (FE.DEVICE, FE.HOST):
                    _check(ft, arenas, layout, n, shift, space, dst_space)
    for space in ("pageable", "pinned", "registered", "device"):
        for shift in (shifts[0], shifts[-1]):
            _check(ft, arenas, layout, BIG, shift, space, FE.DEVICE if shift else FE.HOST)


def test_pinned_sources_both_forms(arenas):
    """page-locked sources are read in place by default; ESVIO_FE_CONVERT_PINNED_COPY=1 (the A/B of KERNELS.md) copies
    them first like pageable memory: the same records"""
    import os
    os.environ["ESVIO_FE_CONVERT_PINNED_COPY"] = "1"
    try:
        t = FE.FeatureTracker(FE.make_config(192, 144, max_cnt=60))
    finally:
        del os.environ["ESVIO_FE_CONVERT_PINNED_COPY"]
    for layout in R.LAYOUTS:
        for n in (9, 2049):
            for space in ("pinned", "registered"):
                _check(t, arenas, layout, n, R.SHIFTS[layout][1], space, FE.DEVICE)
    t.close()


def _poke_t(case, idx, vals):
    """write stamps into the case's bytes and into its logical array"""
    f = case.fields
    w = f.t_bits // 8
    vals = np.asarray(vals, case.t.dtype)
    o = f.ptrs[2] - case.raw.ctypes.data
    at = o + f.strides[2] * np.asarray(idx)[:, None] + np.arange(w)[None, :]
    case.raw[at] = vals.view(np.uint8).reshape(len(idx), w)
    case.t[idx] = vals


@pytest.mark.parametrize("layout", ["soa_u32_us", "soa_i64_ns", "aos16_i64_us", "packed13_i64_us"])
def test_bad_stamps_are_counted_not_clamped(ft, arenas, layout):
    """exactly k bad stamps, at the first index, the last index and on both sides of a block boundary (a workgroup
    takes 1024 events per round): ESVIO_FE_EINVAL and *n_bad == k from every kind of source into both kinds of
    destination; the same batch with them repaired converts"""
    n = 2049 + 1024
    case = R.make_case(layout, n, seed=77, shift=1, polarity="pm1")
    at = np.array([0, 1023, 1024, n - 1])
    good = case.t[at].copy()
    if case.t.dtype == np.uint32:  # unsigned: only the offset can push ticks below zero
        _poke_t(case, np.arange(n), case.t // 2 + 1000)
        good = case.t[at].copy()
        case.t_offset = -500
        case.fields.t_offset = -500
        _poke_t(case, at, [0, 499, 1, 7])
    elif case.t_unit_ns == 1:
        _poke_t(case, at, [16, (1 << 62) + 5, -(1 << 62) - 5, (1 << 32) * 10 ** 9 + 17])
    else:
        _poke_t(case, at, [-(1 << 40), (1 << 62) + 5, -(1 << 62) - 5, (1 << 32) * 10 ** 6 - 999_999])
    _, bad = R.expected(case)
    k = int(bad.sum())
    assert k == len(at) and bad[at].all()
    for space in ("pageable", "pinned", "device"):
        fields, src_space = arenas.source(case, space)
        for dst, dst_space in ((arenas.dev_dst, FE.DEVICE), (C.c_void_p(arenas.back.ctypes.data), FE.HOST)):
            rc, nb = _convert(ft, fields, n, src_space, dst, dst_space)
            assert rc == -1 and nb == k, (layout, space, dst_space, rc, nb, k)
            assert b"convert_events" in ft._hd.L.esvio_fe_last_error(ft._hd.h)
    _poke_t(case, at, good)
    ev, bad = R.expected(case)
    assert not bad.any()
    for space, dst_space in (("pageable", FE.HOST), ("pinned", FE.DEVICE), ("device", FE.DEVICE)):
        _check_case(ft, arenas, case, ev.tobytes(), space, dst_space, (layout, "repaired", space, dst_space))


def test_descriptor_errors(ft, arenas):
    """ESVIO_FE_EINVAL with a message, before anything is touched: no allocation, the destination as it was"""
    L, h = ft._hd.L, ft._hd.h
    case, _ = _case("soa_u32_us", 65, 0)
    _check(ft, arenas, "soa_u32_us", 65, 0, "pageable", FE.DEVICE)  # (scratch of that size exists from here on)
    allocs = ft.latency_stats()["allocs"]
    mem = ft.device_memory()[0]
    arenas.fill_dst(16 * 70)

    def call(n=65, src_space=FE.HOST, dst=arenas.dev_dst, dst_space=FE.DEVICE, **kw):
        d = FE.fields_desc(case.fields)
        for key, v in kw.items():
            setattr(d, key, v)
        bad = C.c_uint64(0)
        return L.esvio_fe_convert_events(h, C.byref(d), n, src_space, dst, dst_space, C.byref(bad))

    assert call() == 0
    arenas.fill_dst(16 * 70)
    for kw in (dict(t_bits=16), dict(t_bits=0), dict(t_unit_ns=10), dict(t_unit_ns=0), dict(p_bits=32), dict(p_bits=1),
               dict(x_stride=1), dict(y_stride=0), dict(t_stride=3), dict(t_bits=64, t_stride=4), dict(p_bits=16, p_stride=1),
               dict(p_stride=-1), dict(x=None), dict(y=None), dict(t=None), dict(p=None), dict(t_offset=(1 << 62) + 1),
               dict(t_offset=-(1 << 62) - 1), dict(src_space=2), dict(dst_space=-1), dict(dst=None),
               dict(dst=C.c_void_p(arenas.dev_dst.value + 4))):
        assert call(**kw) == -1, kw
        assert b"convert_events" in L.esvio_fe_last_error(h), kw
    assert L.esvio_fe_convert_events(None, None, 0, 0, None, 0, None) == -1
    assert L.esvio_fe_convert_events(h, None, 5, 0, arenas.dev_dst, FE.DEVICE, None) == -1
    assert (arenas.read_dst(16 * 70) == GUARD).all()
    # n == 0 succeeds and touches nothing, whatever the pointers
    assert call(n=0) == 0 and call(n=0, x=None, dst=None) == 0
    assert L.esvio_fe_convert_events(h, None, 0, 0, None, 0, None) == 0
    assert (arenas.read_dst(16 * 70) == GUARD).all()
    assert call(t_offset=1 << 62) == -1 and b"stamp" in L.esvio_fe_last_error(h)  # (a legal offset, bad events)
    assert ft.latency_stats()["allocs"] == allocs and ft.device_memory()[0] == mem
    # the mirror
    with pytest.raises(FE.FrontendError) as e:
        ft.convert_events(EventFields.from_arrays(case.x, case.y, case.t, case.p, t_offset=-(1 << 40)))
    assert e.value.n_bad == 65
    tr = FE.Tracks()
    d = FE.fields_desc(case.fields)
    assert L.esvio_fe_track_event_fields(h, 1.0, C.byref(d), 0, C.byref(d), 0, FE.HOST, 1, C.byref(tr)) == -1
    d.t_bits = 8
    assert L.esvio_fe_track_event_fields(h, 1.0, C.byref(d), 65, C.byref(d), 65, FE.HOST, 1, C.byref(tr)) == -1
    assert b"track_event_fields" in L.esvio_fe_last_error(h)


def test_second_call_of_a_size_allocates_nothing(arenas):
    t = FE.FeatureTracker(FE.make_config(192, 144, max_cnt=60))
    case, _ = _case("soa_u32_us", 2049, 0)
    for space, dst_space in (("pageable", FE.HOST), ("pinned", FE.DEVICE), ("device", FE.DEVICE)):
        _check(t, arenas, "soa_u32_us", 2049, 0, space, dst_space)
    n0, mem0 = t._hd.L.esvio_fe_latency_stats, t.device_memory()[0]
    a0 = t.latency_stats()["allocs"]
    for space, dst_space in (("pageable", FE.HOST), ("pinned", FE.DEVICE), ("device", FE.DEVICE), ("registered", FE.HOST)):
        _check(t, arenas, "soa_u32_us", 2049, 0, space, dst_space)
        _check(t, arenas, "packed13_i64_us", 2047, 3, space, dst_space)  # (fewer bytes than the scratch holds)
    assert t.latency_stats()["allocs"] == a0 and t.device_memory()[0] == mem0
    t.close()


# ---- end to end ---------------------------------------------------------------------------------------------------
W, H, FRAMES = 192, 144, 10
PUBS = [True, True, False, True, False, False, True, True, False, True]
MEMBERS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")


@pytest.fixture(scope="module")
def scene():
    """a synth scene stream at the golden scene's size as microsecond arrays per camera (what a recording holds), the
    records make_events builds of them, and the frames' times"""
    s = SceneStream(W, H, rate=1.5e6, seed=21)
    out = []
    for _ in range(FRAMES):
        cams = []
        for ev in s.next_batch()[:2]:
            t_us = ev["sec"].astype(np.int64) * 1_000_000 + ev["nsec"].astype(np.int64) // 1000
            cams.append((ev["x"].copy(), ev["y"].copy(), t_us, ev["polarity"].copy(), make_events(ev["x"], ev["y"], t_us, ev["polarity"])))
        out.append((event_times(cams[0][4])[-1], cams))
    return out


def _fields_of(cam, kind, base_us):
    x, y, t_us, p, _ = cam
    if kind == "soa":  # uint32 microseconds behind a file-wide offset, polarity {0, 1}
        return EventFields.from_arrays(x, y, (t_us - base_us).astype(np.uint32), p.astype(np.uint8), t_offset=int(base_us))
    rec = np.zeros(len(x), R.PACKED13)  # packed records, int64 nanoseconds, polarity {-1, +1}
    rec["x"], rec["y"], rec["t"], rec["p"] = x, y, t_us * 1000, np.where(p > 0, 1, -1)
    return EventFields.from_structured(rec, t_unit_ns=1)


def _snapshot(ft):
    return [getattr(ft, k).copy() for k in MEMBERS]


_reference_runs = {}


def _reference(scene, lk_accum):
    """trackEvent on make_events records, frame by frame: computed once per LK mode"""
    if lk_accum not in _reference_runs:
        ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=60, lk_accum=lk_accum))
        out = []
        for f, (tm, cams) in enumerate(scene):
            ft.trackEvent(tm, cams[0][4], cams[1][4], PUBS[f])
            out.append(_snapshot(ft))
        out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
        ft.close()
        assert len(out[-2][0]) > 20 and len(out[-2][5]) > 5  # (tracks in both cameras: the comparison is not empty)
        _reference_runs[lk_accum] = out
    return _reference_runs[lk_accum]


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (ra, rb) in enumerate(zip(got, want)):
        for k, (va, vb) in enumerate(zip(ra, rb)):
            assert va.dtype == vb.dtype and va.shape == vb.shape, (tag, f, k, va.shape, vb.shape)
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), (tag, f, k)


@pytest.mark.parametrize("lk_accum", [2, 1])
def test_track_event_fields_equals_track_event(scene, lk_accum):
    want = _reference(scene, lk_accum)
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=60, lk_accum=lk_accum))
    base_us = int(scene[0][1][0][2][0]) - 5
    got = []
    for f, (tm, cams) in enumerate(scene):
        kind = "soa" if f % 2 else "packed"
        ft.trackEventFields(tm, _fields_of(cams[0], kind, base_us), _fields_of(cams[1], kind, base_us), PUBS[f])
        got.append(_snapshot(ft))
        if f == 2:
            a0, mem0 = ft.latency_stats()["allocs"], ft.device_memory()[0]
    # (the batches differ in size by a few per cent: inside the quarter the buffers grow by)
    assert ft.latency_stats()["allocs"] == a0 and ft.device_memory()[0] == mem0
    got.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    # a bad stamp fails the call before anything is tracked
    x, y, t_us, p, _ = scene[-1][1][0]
    t_bad = t_us.copy()
    t_bad[len(t_bad) // 2] = -1
    before = _snapshot(ft)
    with pytest.raises(FE.FrontendError):
        ft.trackEventFields(scene[-1][0] + 1.0, EventFields.from_arrays(x, y, t_bad, p.astype(np.int8)),
                            _fields_of(scene[-1][1][1], "soa", base_us), True)
    _same([_snapshot(ft), [ft.gettimesurface(0), ft.gettimesurface(1)]], [before, got[-1]], "after a refused call")
    ft.close()
    _same(got, want, ("trackEventFields", lk_accum))


@pytest.mark.parametrize("lk_accum", [2, 1])
def test_converted_batches_in_the_replay_schedule(scene, lk_accum):
    """every batch converted into device memory, then the replay schedule: announced three ahead, lazy returns (each
    completed by finish() so that every member can be compared), and a stray conversion between the track calls of the
    announced sequence"""
    want = _reference(scene, lk_accum)
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=60, lk_accum=lk_accum))
    ft.set_lazy_new_stereo(True)
    base_us = int(scene[0][1][0][2][0]) - 5
    conv = [[ft.convert_events(_fields_of(c, "packed" if f % 2 else "soa", base_us)) for c in cams]
            for f, (tm, cams) in enumerate(scene)]
    for f, (tm, cams) in enumerate(scene):  # the records themselves
        for c, cam in zip(conv[f], cams):
            host = ft.convert_events(_fields_of(cam, "soa", base_us), space=FE.HOST)
            assert c.n == len(cam[4]) and host.array.tobytes() == cam[4].tobytes()
    got, announced = [], 0
    for f, (tm, cams) in enumerate(scene):
        while announced < min(f + 3, FRAMES - 1):
            announced += 1
            ft.set_next_batch(scene[announced][0], conv[announced][0].arg, conv[announced][1].arg, PUBS[announced])
        ft.trackEvent(tm, conv[f][0].arg, conv[f][1].arg, PUBS[f])
        stray = ft.convert_events(_fields_of(cams[f % 2], "packed", base_us), space=FE.DEVICE if f % 2 else FE.HOST)
        stray.free()
        ft.finish()
        got.append(_snapshot(ft))
    got.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    ft.close()
    for pair in conv:
        for c in pair:
            c.free()
    _same(got, want, ("replay", lk_accum))
