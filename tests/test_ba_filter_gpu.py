"""GPU: esvio_fe_filter_events (k_sae_keys + k_radix_pass + k_baf_*) against the sequential restatement
tests/ba_filter_ref.py — flags, n_kept, the kept records, last_kept, n_rejected and the plane's effect on the next call
— and esvio_fe_track_event_filtered against esvio_fe_track_event on the restatement's kept records.  Integers only:
every comparison is equality.  The handle and the restatement advance their planes side by side, so every call after
a test's first also checks what the calls before it left in the plane."""
import ctypes as C

import numpy as np
import pytest

import ba_filter_cases as K
import ba_filter_ref as R
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

MS = 1_000_000
GUARD = 0xA5
CAP = 40_000  # records the arenas hold


class Arenas:
    """one buffer per memory space, reused by every case"""

    def __init__(self):
        L = self.L = FE.load_library()
        self.hip = C.CDLL("libamdhip64.so")
        self.pin_ptr, self.dev_src, self.dev_dst = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.esvio_fe_mem_alloc(FE.HOST, 16 * CAP, C.byref(self.pin_ptr)) == 0
        self.pinned = np.ctypeslib.as_array(C.cast(self.pin_ptr, C.POINTER(C.c_uint8)), shape=(16 * CAP,))
        assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * CAP, C.byref(self.dev_src)) == 0
        assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * (CAP + 2), C.byref(self.dev_dst)) == 0
        self.back = np.zeros(16 * (CAP + 2), np.uint8)

    def close(self):
        self.L.esvio_fe_mem_free(FE.HOST, self.pin_ptr)
        self.L.esvio_fe_mem_free(FE.DEVICE, self.dev_src)
        self.L.esvio_fe_mem_free(FE.DEVICE, self.dev_dst)

    def source(self, ev, space):
        """the records in `space` -> (pointer, ESVIO_FE_HOST / ESVIO_FE_DEVICE, what keeps them alive)"""
        raw = np.ascontiguousarray(ev).view(np.uint8).reshape(-1)
        if space == "pageable":
            return C.c_void_p(raw.ctypes.data), FE.HOST, raw
        if space == "pinned":
            self.pinned[:len(raw)] = raw
            return self.pin_ptr, FE.HOST, None
        assert self.L.esvio_fe_mem_upload(self.dev_src, C.c_void_p(raw.ctypes.data), len(raw)) == 0
        return self.dev_src, FE.DEVICE, None

    def fill_dst(self, nbytes):
        self.back[:nbytes] = GUARD
        assert self.L.esvio_fe_mem_upload(self.dev_dst, C.c_void_p(self.back.ctypes.data), nbytes) == 0

    def read_dst(self, nbytes):
        assert self.hip.hipMemcpy(C.c_void_p(self.back.ctypes.data), self.dev_dst, C.c_size_t(nbytes), 2) == 0
        return self.back[:nbytes]


@pytest.fixture(scope="module")
def arenas():
    a = Arenas()
    yield a
    a.close()


class Filtered:
    """a handle and the restatement's planes of its two cameras, advanced together"""

    def __init__(self, w, h, **kw):
        self.w, self.h = w, h
        self.ft = FE.FeatureTracker(FE.make_config(w, h, max_cnt=kw.pop("max_cnt", 40), **kw))
        self.fresh()

    def fresh(self):
        self.B = [R.fresh_plane(self.w, self.h), R.fresh_plane(self.w, self.h)]

    def close(self):
        self.ft.close()

    def call(self, arenas, cam, ev, window, min_support, space, dst_space):
        """one esvio_fe_filter_events call -> (rc, flags, n_kept, kept bytes, last record bytes, n_rejected)"""
        L, h = self.ft._hd.L, self.ft._hd.h
        n = len(ev)
        assert n <= CAP
        src, src_space, keep = arenas.source(ev, space)
        flags = np.full(n + 8, GUARD, np.uint8)
        last = np.full(16, GUARD, np.uint8)
        nk, rej = C.c_uint64(99), C.c_uint64(99)
        if dst_space == FE.DEVICE:
            arenas.fill_dst(16 * (n + 2))
            dst = arenas.dev_dst
        else:
            host = arenas.back[:16 * (n + 2)]
            host[:] = GUARD
            dst = C.c_void_p(host.ctypes.data)
        rc = L.esvio_fe_filter_events(h, cam, src, n, src_space, window, min_support, dst, dst_space, C.byref(nk),
                                      C.c_void_p(flags.ctypes.data), C.c_void_p(last.ctypes.data), C.byref(rej))
        got = arenas.read_dst(16 * (n + 2)) if dst_space == FE.DEVICE else host
        assert (flags[n:] == GUARD).all()
        k = int(nk.value)
        assert (got[16 * max(k, n):] == GUARD).all(), "bytes beyond n records touched"
        return rc, flags[:n], k, got[:16 * k].tobytes(), last.tobytes(), int(rej.value)

    def check(self, arenas, cam, ev, window, min_support=1, space="device", dst_space=FE.DEVICE, tag=None):
        """the call equals the restatement (which advances its plane of `cam`); returns the kept fraction"""
        ev = ev.copy()
        R.raw_records(ev)[:, 13:] = ((np.arange(3 * len(ev)) * 7 + 1) & 255).astype(np.uint8).reshape(-1, 3)  # (the padding travels too)
        want, want_rej = R.filter_events(self.B[cam], self.w, self.h, ev, window, min_support)
        kept, last = R.kept_of(ev, want)
        rc, flags, k, rec, last_got, rej = self.call(arenas, cam, ev, window, min_support, space, dst_space)
        assert rc == 0, (tag, rc, self.ft._hd.L.esvio_fe_last_error(self.ft._hd.h))
        if not np.array_equal(flags, want):
            i = int(np.flatnonzero(flags != want)[0])
            raise AssertionError((tag, "first differing flag at event", i, ev[i], int(flags[i]), int(want[i]),
                                  int((flags != want).sum()), len(ev)))
        assert k == len(kept) and rej == want_rej, (tag, k, len(kept), rej, want_rej)
        assert rec == kept.tobytes(), (tag, "kept records")
        assert last_got == (last.tobytes() if last is not None else bytes([GUARD]) * 16), (tag, "last_kept")
        return float(want.mean()) if len(ev) else 0.0


@pytest.fixture(scope="module")
def f42():
    f = Filtered(K.W, K.H)
    yield f
    f.close()


@pytest.fixture(scope="module")
def f64():
    f = Filtered(64, 48)
    yield f
    f.close()


def _fresh(f):
    f.ft.filter_reset()
    f.fresh()
    return f


def _in_range(frac, tag):
    assert 0.1 <= frac <= 0.9, ("a comparison that keeps (nearly) nothing or everything shows little", tag, frac)


# ---- the hand-made cases, the sizes, one long segment -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.HAND))
def test_hand_made_cases(f42, arenas, name):
    ev, min_support, want, rejected = K.hand_case(name)
    _fresh(f42)
    rc, flags, k, rec, last, rej = f42.call(arenas, 0, ev, K.WINDOW, min_support, "device", FE.DEVICE)
    assert rc == 0 and flags.tolist() == want.tolist() and rej == rejected and k == int(want.sum())
    assert rec == R.raw_records(ev)[want != 0].tobytes()
    _fresh(f42).check(arenas, 1, ev, K.WINDOW, min_support, "pageable", FE.HOST, name)  # ... and by the restatement


@pytest.mark.parametrize("n", K.SWEEP_SIZES)
def test_size_sweep(f42, arenas, n):
    ev = K.sweep_events(n)
    _fresh(f42)
    frac = f42.check(arenas, 0, ev, MS, 1, "device", FE.DEVICE, ("sweep", n))
    if n >= 63:
        _in_range(frac, n)
    if n == 1:
        assert frac == 0.0
    # the same events again, half a window later: the plane the first call left decides their first events
    again = ev.copy()
    t = event_times_ns(again) + MS // 2
    again["sec"], again["nsec"] = t // 10 ** 9, t % 10 ** 9
    f42.check(arenas, 0, again, MS, 1, "pageable", FE.HOST, ("sweep again", n))


def event_times_ns(ev):
    return ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"].astype(np.int64)


def test_hot_pixel(f42, arenas):
    ev = K.hot_pixel_events()
    _in_range(_fresh(f42).check(arenas, 0, ev, 2000, 1, "device", FE.DEVICE, "hot pixel"), "hot pixel")
    f42.check(arenas, 0, ev, 2000, 2, "device", FE.HOST, "hot pixel, support 2, on the plane it left")


@pytest.mark.parametrize("w,h,window", [(K.W, K.H, MS), (346, 260, 40 * MS)])
def test_call_sizes_big_small_big_on_one_handle(arenas, w, h, window):
    """the stage's sort scratch is the handle's own (baf.sort): its keys kernel clears the look-back words of THIS call's
    tile count, its heads kernel the histograms and tickets for the next.  Calls of 4 sort tiles, one tile, one event and
    the first size again on one handle, flags and records as the restatement's on the planes the
    calls before left.  The digit width follows the sensor (2 x 6 bits at 42 x 42, 3 x 6 at 346 x 260) and cannot
    change within a handle: the second sensor is a second handle."""
    f = Filtered(w, h)
    try:
        for k, n in enumerate((6500, 300, 6500, 1, 2049, 6500)):
            ev = K.uniform_events(n, w, h, 8 * n, seed=300 + k, t0_us=1_000_000_000 + k * 20_000)
            frac = f.check(arenas, 0, ev, window, 1, "device", FE.DEVICE, ("sizes", w, n, k))
            if n >= 6500:
                _in_range(frac, (w, n, k))
    finally:
        f.close()


# ---- the plane from call to call ----------------------------------------------------------------------------------
def _three_batches(w, h, n=3000, seed=40):
    return [K.uniform_events(n, w, h, 8 * n, seed + b, t0_us=1_000_000_000 + b * 8 * n) for b in range(3)]


def test_carry_over_and_both_resets(f64, arenas):
    batches = _three_batches(64, 48)
    _fresh(f64)
    for b, ev in enumerate(batches):
        _in_range(f64.check(arenas, 0, ev, MS, 1, "device", FE.DEVICE, ("carry", b)), b)
    # the third batch alone gives other flags than behind the first two: the plane mattered
    alone, _ = R.filter_events(R.fresh_plane(64, 48), 64, 48, batches[2], MS)
    plane = R.fresh_plane(64, 48)
    behind = [R.filter_events(plane, 64, 48, ev, MS)[0] for ev in batches][2]
    assert not np.array_equal(alone, behind)
    for reset in (f64.ft._hd.L.esvio_fe_filter_reset, f64.ft._hd.L.esvio_fe_reset):
        f64.check(arenas, 0, batches[1], MS, 1, "device", FE.DEVICE, "before the reset")
        f64.check(arenas, 1, batches[1], MS, 1, "device", FE.DEVICE, "before the reset")
        assert reset(f64.ft._hd.h) == 0
        f64.fresh()
        for cam in (0, 1):
            rc, flags, k, rec, last, rej = f64.call(arenas, cam, batches[2], MS, 1, "device", FE.DEVICE)
            assert rc == 0 and np.array_equal(flags, alone), (reset, cam)
            R.filter_events(f64.B[cam], 64, 48, batches[2], MS)


def test_cameras_have_planes_of_their_own(f64, arenas):
    a, x, b = _three_batches(64, 48, seed=50)
    x = x.copy()
    x["sec"], x["nsec"] = b["sec"], b["nsec"]  # (camera 1's stamps are those of camera 0's next batch: they would support, if seen)
    _fresh(f64)
    f64.check(arenas, 0, a, MS, 1, "device", FE.DEVICE, "cam 0, first")
    f64.check(arenas, 1, x, 5 * MS, 1, "device", FE.DEVICE, "cam 1")
    f64.check(arenas, 0, b, MS, 1, "device", FE.DEVICE, "cam 0, behind cam 1's call")
    f64.check(arenas, 1, b, MS, 1, "device", FE.DEVICE, "cam 1, second")
    with_x, _ = R.filter_events(R.fresh_plane(64, 48), 64, 48, np.concatenate([a, x, b]), MS)
    without, _ = R.filter_events(R.fresh_plane(64, 48), 64, 48, np.concatenate([a, b]), MS)
    assert not np.array_equal(with_x[-len(b):], without[-len(b):])  # (one shared plane would have shown)


# ---- stamps in no order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["shuffled", "second_half_a_second_earlier", "nsec_above_2_30", "sec_2_32_minus_1",
                                  "equal_stamps"])
def test_non_monotonic_stamps(f64, arenas, kind):
    n = 3000
    ev = K.uniform_events(n, 64, 48, 8 * n, seed=60, t0_us=5_000_000)
    rng = np.random.default_rng(61)
    t = event_times_ns(ev)
    if kind == "shuffled":
        t = rng.permutation(t)
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    elif kind == "second_half_a_second_earlier":
        t[n // 2:] -= 10 ** 9 - 12 * MS  # (the halves overlap in time within the window's reach)
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    elif kind == "nsec_above_2_30":
        ev["sec"], ev["nsec"] = 3, (1 << 30) + (t - t.min())  # 1.07 .. 1.1 s in the nsec word, as it is
        assert (ev["nsec"] >= 1 << 30).all()
    elif kind == "sec_2_32_minus_1":
        ev["sec"], ev["nsec"] = (1 << 32) - 1, t - t.min()
        ev["sec"][::7] -= 1
        ev["nsec"][::7] += 10 ** 9 - 3 * MS  # ... and seven in the second before, up to 3 ms earlier
    else:
        t = (t // (2 * MS)) * (2 * MS)  # a dozen distinct stamps: differences of exactly 0 and exactly 2 ms
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    _fresh(f64)
    window = 2 * MS if kind == "equal_stamps" else MS
    _in_range(f64.check(arenas, 0, ev, window, 1, "device", FE.DEVICE, kind), kind)
    f64.check(arenas, 0, ev[::-1].copy(), window, 2, "pageable", FE.HOST, (kind, "reversed, support 2"))


# ---- streams, parameters, spaces ----------------------------------------------------------------------------------
SW, SH = 128, 96


def _scene(frames=8):
    s = SceneStream(W=SW, H=SH, rate=2e5, noise_frac=0.5, n_rect=6, size=(12, 30), disparity=4, seed=7)
    return [s.next_batch() for _ in range(frames)]


@pytest.fixture(scope="module")
def scene():
    return _scene()


@pytest.fixture(scope="module")
def f128():
    f = Filtered(SW, SH)
    yield f
    f.close()


@pytest.mark.parametrize("window_ms,min_support", [(1, 1), (5, 1), (20, 1), (20, 2), (20, 8), (5, 2)])
def test_scene_stream_parameters(f128, arenas, scene, window_ms, min_support):
    """four frames of the scene stream, both cameras, per window and support.  The left camera's kept fraction is
    asserted to lie in [0.1, 0.9] for every pair but (20 ms, support 8): that one keeps 4-6 % of this stream, it is an
    equality-only case, and support 8 has its asserted case in test_min_support_8_on_a_dense_patch.  The right
    camera's calls (the same scene shifted by the disparity) are compared for equality alone."""
    _fresh(f128)
    fracs = []
    for f, (left, right, _) in enumerate(scene[:4]):
        fracs.append(f128.check(arenas, 0, left, window_ms * MS, min_support, "device", FE.DEVICE, ("scene L", f)))
        f128.check(arenas, 1, right, window_ms * MS, min_support, "device", FE.HOST, ("scene R", f))
    if min_support != 8:  # (support 8 keeps a twentieth of this stream: test_min_support_8_on_a_dense_patch)
        for fr in fracs:
            _in_range(fr, (window_ms, min_support))


def test_scene_stream_346x260(arenas):
    """a DAVIS346-sized sensor (keys of 17 bits: three sort passes): the first 30 k left and 40 k right events of a
    1 Mev/s scene batch with 30 % noise, then the left camera's next 10 k on the plane the first call left"""
    f = Filtered(346, 260)
    left, right, _ = SceneStream(W=346, H=260, rate=1e6, noise_frac=0.3).next_batch()
    _in_range(f.check(arenas, 0, left[:30000], 20 * MS, 1, "device", FE.DEVICE, "346 L"), "346 20/1")
    _in_range(f.check(arenas, 1, right[:40000], 5 * MS, 2, "pinned", FE.DEVICE, "346 R"), "346 5/2")
    f.check(arenas, 0, left[30000:40000], 20 * MS, 1, "device", FE.HOST, "346 L, second call")
    f.close()


def test_min_support_8_on_a_dense_patch(f42, arenas):
    """support 8 keeps next to nothing of a scene stream; on a 12 x 12 patch where every pixel is stamped again and
    again the interior pixels pass and the border pixels (fewer than 8 neighbours stamped, or in the sensor) do not"""
    ev = K.uniform_events(4097, K.W, K.H, 8 * 4097, seed=1, patch=12)
    _in_range(_fresh(f42).check(arenas, 0, ev, 20 * MS, 8, "device", FE.DEVICE, "support 8"), "support 8")


@pytest.mark.parametrize("space", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("dst_space", [FE.HOST, FE.DEVICE])
def test_memory_spaces(f64, arenas, space, dst_space):
    _fresh(f64)
    for b, ev in enumerate(_three_batches(64, 48, n=2500, seed=70)[:2]):
        _in_range(f64.check(arenas, b, ev, MS, 1, space, dst_space, (space, dst_space, b)), (space, dst_space))


def test_second_call_of_a_size_allocates_nothing(arenas):
    f = Filtered(64, 48)
    mem0 = f.ft.device_memory()[0]
    ev = K.uniform_events(2049, 64, 48, 8 * 2049, seed=80)
    combos = (("pageable", FE.HOST), ("pinned", FE.DEVICE), ("device", FE.DEVICE))
    for space, dst_space in combos:
        f.check(arenas, 0, ev, MS, 1, space, dst_space, "first")
    assert f.ft.device_memory()[0] < mem0  # (the planes and the scratch: allocated by the first filtering call)
    a1, mem1 = f.ft.latency_stats()["allocs"], f.ft.device_memory()[0]
    for space, dst_space in combos + (("device", FE.HOST),):
        f.check(arenas, 1, ev, MS, 1, space, dst_space, "second")
        f.check(arenas, 0, ev[:2047], MS, 2, space, dst_space, "smaller")
    assert f.ft.latency_stats()["allocs"] == a1 and f.ft.device_memory()[0] == mem1
    f.close()


def test_argument_errors(f64, arenas):
    """ESVIO_FE_EINVAL with a message, before any device work: nothing allocated, the destination and the plane as
    they were"""
    L, h = f64.ft._hd.L, f64.ft._hd.h
    ev = K.uniform_events(65, 64, 48, 520, seed=90)
    _fresh(f64).check(arenas, 0, ev, MS, 1, "device", FE.DEVICE, "scratch exists from here on")
    allocs, mem = f64.ft.latency_stats()["allocs"], f64.ft.device_memory()[0]
    src, _, _ = arenas.source(ev, "device")
    arenas.fill_dst(16 * 70)
    nk, rej = C.c_uint64(0), C.c_uint64(0)

    def call(cam=0, ev=src, n=65, space=FE.DEVICE, window=MS, min_support=1, dst=arenas.dev_dst, dst_space=FE.DEVICE):
        return L.esvio_fe_filter_events(h, cam, ev, n, space, window, min_support, dst, dst_space, C.byref(nk), None, None,
                                        C.byref(rej))

    for kw in (dict(window=0), dict(window=-5), dict(window=(1 << 62) + 1), dict(min_support=0), dict(min_support=9),
               dict(min_support=-1), dict(cam=2), dict(cam=-1), dict(space=2), dict(dst_space=-1), dict(ev=None),
               dict(dst=None), dict(dst=C.c_void_p(arenas.dev_dst.value + 8)),
               dict(dst=src), dict(dst=C.c_void_p(src.value + 16 * 64)), dict(ev=C.c_void_p(arenas.dev_dst.value + 16 * 32))):
        assert call(**kw) == -1, kw
        assert b"filter_events" in L.esvio_fe_last_error(h), kw
    assert (arenas.read_dst(16 * 70) == GUARD).all()
    assert call(n=0) == 0 and call(n=0, ev=None, dst=None) == 0 and nk.value == 0  # n == 0 touches nothing
    assert call(window=1 << 62, min_support=8) == 0 and nk.value == 0               # (the limits themselves are legal)
    R.filter_events(f64.B[0], 64, 48, ev, 1 << 62, 8)
    assert f64.ft.latency_stats()["allocs"] == allocs and f64.ft.device_memory()[0] == mem
    f64.check(arenas, 0, ev, MS, 1, "device", FE.DEVICE, "the plane behind the refused calls")
    tr, kept = FE.Tracks(), (C.c_uint64 * 2)()
    for kw in (dict(window=0), dict(min_support=9), dict(space=3)):
        a = dict(window=MS, min_support=1, space=FE.DEVICE)
        a.update(kw)
        assert L.esvio_fe_track_event_filtered(h, src, 65, src, 65, a["space"], a["window"], a["min_support"], 1,
                                               C.byref(tr), C.byref(kept), None) == -1, kw
        assert b"track_event_filtered" in L.esvio_fe_last_error(h)
    assert L.esvio_fe_track_event_filtered(h, None, 65, src, 65, FE.DEVICE, MS, 1, 1, C.byref(tr), C.byref(kept), None) == -1


def test_python_mirror(f64, arenas):
    ev = K.uniform_events(2500, 64, 48, 20000, seed=95)
    _fresh(f64)
    want, rej = R.filter_events(f64.B[0], 64, 48, ev, MS)
    kept, flags, n_rej = f64.ft.filter_events(0, ev, MS)
    assert np.array_equal(flags, want) and n_rej == rej and kept.tobytes() == R.raw_records(ev)[want != 0].tobytes()
    want, rej = R.filter_events(f64.B[0], 64, 48, ev, 5 * MS, 2)
    dev, flags, n_rej = f64.ft.filter_events(0, ev, 5 * MS, min_support=2, device=True)
    assert np.array_equal(flags, want) and dev.n == int(want.sum()) and dev.last.tobytes() == R.raw_records(ev)[want != 0][-1].tobytes()
    R.filter_events(f64.B[1], 64, 48, ev[want != 0], MS)
    f64.ft.filter_events(1, dev.arg, MS)  # (device records go back in as any device batch)
    dev.free()
    f64.check(arenas, 1, ev, MS, 1, "device", FE.DEVICE, "behind the mirror's calls")


# ---- the tracker ----------------------------------------------------------------------------------------------------
MEMBERS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
PUBS = [True, True, False, True, False, False, True, True]


def _snapshot(ft):
    return [getattr(ft, k).copy() for k in MEMBERS]


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (ra, rb) in enumerate(zip(got, want)):
        for k, (va, vb) in enumerate(zip(ra, rb)):
            assert va.dtype == vb.dtype and va.shape == vb.shape, (tag, f, k, va.shape, vb.shape)
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), (tag, f, k)


_plain_runs = {}


def _plain(scene):
    """trackEvent on the raw scene batches, frame by frame: computed once"""
    if "run" not in _plain_runs:
        ft = FE.FeatureTracker(FE.make_config(SW, SH, max_cnt=40))
        out = []
        for f, (left, right, t_us) in enumerate(scene):
            ft.trackEvent(t_us * 1e-6, left, right, PUBS[f])
            out.append(_snapshot(ft))
        out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
        ft.close()
        assert len(out[-2][0]) > 5
        _plain_runs["run"] = out
    return _plain_runs["run"]


@pytest.mark.parametrize("announced", [False, True])
def test_stage_tap_between_track_calls_changes_no_tracking_result(scene, arenas, announced):
    want = _plain(scene)
    f = Filtered(SW, SH)
    ft, got, ahead = f.ft, [], 0
    if announced:
        ft.set_lazy_new_stereo(True)
    for k, (left, right, t_us) in enumerate(scene):
        while announced and ahead < min(k + 3, len(scene) - 1):
            ahead += 1
            ft.set_next_batch(scene[ahead][2] * 1e-6, scene[ahead][0], scene[ahead][1], PUBS[ahead])
        ft.trackEvent(t_us * 1e-6, left, right, PUBS[k])
        f.check(arenas, k % 2, left if k % 2 else right, 5 * MS, 1, "device" if k % 2 else "pageable",
                FE.DEVICE if k % 3 else FE.HOST, ("tap", announced, k))
        if announced:
            ft.finish()
        got.append(_snapshot(ft))
    got.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    f.close()
    _same(got, want, ("tap", announced))


def test_track_event_filtered_equals_track_event_on_the_kept_records(scene):
    window, min_support = 5 * MS, 1
    fused = FE.FeatureTracker(FE.make_config(SW, SH, max_cnt=40))
    plain = FE.FeatureTracker(FE.make_config(SW, SH, max_cnt=40))
    B = [R.fresh_plane(SW, SH), R.fresh_plane(SW, SH)]
    got, want = [], []
    # one batch of isolated left events (no two within reach of each other) in front of frame 3, on a plane that is
    # made fresh for it: nothing is kept on the left, nothing is tracked
    lonely = K.records([(5 + 9 * (i % 12), 5 + 9 * (i // 12), 1, 1000 * i) for i in range(60)])
    for f, (left, right, _) in enumerate(scene):
        if f == 3:
            fused.filter_reset()
            B = [R.fresh_plane(SW, SH), R.fresh_plane(SW, SH)]
            before = _snapshot(fused)
            R.filter_events(B[0], SW, SH, lonely, window, min_support)
            flags_r, _ = R.filter_events(B[1], SW, SH, right, window, min_support)
            kept, t = fused.trackEventFiltered(lonely, right, window, min_support, pub=True)
            assert kept == (0, int(flags_r.sum())) and t is None
            _same([_snapshot(fused)], [before], "an empty left batch leaves `out` as it was")
        fl, _ = R.filter_events(B[0], SW, SH, left, window, min_support)
        fr, _ = R.filter_events(B[1], SW, SH, right, window, min_support)
        _in_range(float(fl.mean()), ("fused L", f))
        _in_range(float(fr.mean()), ("fused R", f))
        kl, kr = left[fl != 0], right[fr != 0]
        cur_time = float(kl[-1]["sec"]) + 1e-9 * float(kl[-1]["nsec"])
        src = (left, right) if f % 2 else (FE.EventBuffer(left, FE.DEVICE), FE.EventBuffer(right, FE.DEVICE))
        kept, t = fused.trackEventFiltered(src[0] if f % 2 else src[0].arg, src[1] if f % 2 else src[1].arg, window,
                                           min_support, pub=PUBS[f])
        assert kept == (len(kl), len(kr)) and t == cur_time, (f, kept, t, cur_time)
        got.append(_snapshot(fused))
        plain.trackEvent(cur_time, kl, kr, PUBS[f])
        want.append(_snapshot(plain))
        if not f % 2:  # (the filter has run: nothing of the call reads the caller's device batches any more)
            src[0].free(), src[1].free()
    got.append([fused.gettimesurface(0), fused.gettimesurface(1)])
    want.append([plain.gettimesurface(0), plain.gettimesurface(1)])
    assert len(want[-2][0]) > 5  # (tracks: the comparison is not empty)
    _same(got, want, "trackEventFiltered")
    # with batches announced the call is refused
    left, right, t_us = scene[-1]
    fused.set_next_batch(t_us * 1e-6 + 1.0, left, right, True)
    with pytest.raises(FE.FrontendError) as e:
        fused.trackEventFiltered(left, right, window, min_support)
    assert "rc=-1" in str(e.value) and "announced" in str(e.value)
    fused.close()
    plain.close()
