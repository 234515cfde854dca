"""GPU: esvio_fe_filter_batch — the filter rule with esvio_fe_filter_params (support test, refractory period), on
records and on caller-layout field arrays read where they lie — against the sequential restatement
tests/ba_filter2_ref.py, and esvio_fe_track_batch against the calls it gathers.  Integers only: flags, kept bytes,
n_kept, last_kept and n_rejected are compared for equality, tracking results bit for bit.  A handle and the
restatement advance their planes side by side, so every call after a test's first also checks what the calls before it
left in the plane."""
import ctypes as C

import numpy as np
import pytest

import ba_filter2_ref as R2
import ba_filter_cases as K
import ba_filter_ref as R
import event_fields_ref as RF
import test_ba_filter2_ref as H2
import test_ba_filter_gpu as T
import test_event_fields_gpu as TF
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, EventFields, event_times

pytestmark = pytest.mark.gpu

MS = T.MS
GUARD = T.GUARD
P = FE.FilterParams


def event_ns(ev):
    return ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"].astype(np.int64)


def shifted(ev, ns):
    """the same events `ns` nanoseconds later"""
    out = ev.copy()
    t = event_ns(ev) + ns
    out["sec"], out["nsec"] = t // 10 ** 9, t % 10 ** 9
    return out


@pytest.fixture(scope="module")
def arenas():
    a = T.Arenas()
    yield a
    a.close()


@pytest.fixture(scope="module")
def farenas():
    a = TF.Arenas()
    yield a
    a.close()


def batch_call(ft, arenas, cam, n, prm, dst_space, ev=None, fields=None, space=FE.DEVICE):
    """one esvio_fe_filter_batch call (ev: a pointer; fields: an EventFields) into the arena's destination ->
    (rc, flags, n_kept, kept bytes, last record bytes, n_rejected, n_bad)"""
    L, h = ft._hd.L, ft._hd.h
    flags = np.full(n + 8, GUARD, np.uint8)
    last = np.full(16, GUARD, np.uint8)
    nk, rej, bad = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    if dst_space == FE.DEVICE:
        arenas.fill_dst(16 * (n + 2))
        dst = arenas.dev_dst
    else:
        host = arenas.back[:16 * (n + 2)]
        host[:] = GUARD
        dst = C.c_void_p(host.ctypes.data)
    desc = FE.fields_desc(fields) if fields is not None else None
    rc = L.esvio_fe_filter_batch(h, cam, ev, C.byref(desc) if desc is not None else None, n, space, C.byref(prm), dst,
                                 dst_space, C.byref(nk), C.c_void_p(flags.ctypes.data), C.c_void_p(last.ctypes.data),
                                 C.byref(rej), C.byref(bad))
    got = arenas.read_dst(16 * (n + 2)) if dst_space == FE.DEVICE else host
    assert (flags[n:] == GUARD).all()
    k = int(nk.value)
    if rc == 0:
        assert (got[16 * max(k, n):] == GUARD).all(), "bytes beyond n records touched"
    return rc, flags[:n].copy(), k, got[:16 * k].tobytes(), last.tobytes(), int(rej.value), int(bad.value)


class Filtered2(T.Filtered):
    """T.Filtered (esvio_fe_filter_events against ba_filter_ref) plus esvio_fe_filter_batch against ba_filter2_ref,
    on the same handle and the same restated planes"""

    def check2(self, arenas, cam, ev, prm, space="device", dst_space=FE.DEVICE, tag=None):
        """the call on records equals the restatement -> (kept fraction, share of the supported events the refractory
        test drops)"""
        ev = ev.copy()
        R.raw_records(ev)[:, 13:] = ((np.arange(3 * len(ev)) * 5 + 3) & 255).astype(np.uint8).reshape(-1, 3)  # (the padding travels too)
        want, want_rej, sup, refr = R2.filter_events(self.B[cam], self.w, self.h, ev, prm.window_ns, prm.min_support,
                                                     prm.refractory_ns, want_parts=True)
        kept, last = R.kept_of(ev, want)
        src, src_space, keep = arenas.source(ev, space)
        rc, flags, k, rec, last_got, rej, bad = batch_call(self.ft, arenas, cam, len(ev), prm, dst_space, ev=src, space=src_space)
        assert rc == 0 and bad == 0, (tag, rc, self.ft._hd.L.esvio_fe_last_error(self.ft._hd.h))
        if not np.array_equal(flags, want):
            i = int(np.flatnonzero(flags != want)[0])
            raise AssertionError((tag, "first differing flag at event", i, ev[i], int(flags[i]), int(want[i]),
                                  int((flags != want).sum()), len(ev)))
        assert k == len(kept) and rej == want_rej, (tag, k, len(kept), rej, want_rej)
        assert rec == kept.tobytes(), (tag, "kept records")
        assert last_got == (last.tobytes() if last is not None else bytes([GUARD]) * 16), (tag, "last_kept")
        n = max(len(ev), 1)
        return float(want.sum()) / n, float((sup & refr).sum()) / max(int(sup.sum()), 1)


@pytest.fixture(scope="module")
def f42():
    f = Filtered2(K.W, K.H)
    yield f
    f.close()


@pytest.fixture(scope="module")
def f64():
    f = Filtered2(64, 48)
    yield f
    f.close()


def _fresh(f):
    f.ft.filter_reset()
    f.fresh()
    return f


def _not_vacuous(fr, tag, refractory=True):
    kept, dropped = fr
    print(tag, "kept %.3f, supported events the refractory test drops %.3f" % (kept, dropped))
    assert 0.1 <= kept <= 0.9, ("a comparison that keeps (nearly) nothing or everything shows little", tag, kept)
    if refractory:
        assert dropped >= 0.1, ("the refractory test drops too little of what the support test keeps", tag, dropped)


# ---- against the restatement: records ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.HAND))
def test_first_rules_hand_cases_through_the_new_entry(f42, arenas, name):
    ev, min_support, want, rejected = K.hand_case(name)
    _fresh(f42).check2(arenas, 0, ev, P(K.WINDOW, min_support, 0), "pageable", FE.HOST, name)
    assert R2.filter_events(R2.fresh_plane(K.W, K.H), K.W, K.H, ev, K.WINDOW, min_support, 0)[0].tolist() == want.tolist()


@pytest.mark.parametrize("name", sorted(H2.HAND2))
def test_refractory_hand_cases(f42, arenas, name):
    rows, window, min_support, refractory, want, rejected = H2.HAND2[name]
    ev = K.records(rows)
    got = R2.filter_events(R2.fresh_plane(K.W, K.H), K.W, K.H, ev, window, min_support, refractory)
    assert got[0].tolist() == want and got[1] == rejected  # (the restatement gives the hand-derived answer ...)
    _fresh(f42).check2(arenas, 0, ev, P(window, min_support, refractory), "device", FE.DEVICE, name)  # ... and the kernels its


@pytest.mark.parametrize("n", K.SWEEP_SIZES)
def test_size_sweep(f42, arenas, n):
    """each size twice on one plane — the second time half a window later, on what the first call left — with the
    support and the refractory test together, then with the refractory test alone"""
    ev = K.sweep_events(n)
    for prm in (P(MS, 1, 4 * MS), P(0, 0, 4 * MS)):
        _fresh(f42)
        fr = f42.check2(arenas, 0, ev, prm, "device", FE.DEVICE, ("sweep", n, prm.min_support))
        if n >= 63:
            _not_vacuous(fr, ("sweep", n, prm.min_support), refractory=prm.min_support > 0)
        f42.check2(arenas, 0, shifted(ev, MS // 2), prm, "pinned", FE.HOST, ("sweep, carried over", n, prm.min_support))


def test_hot_pixel(f42, arenas):
    """a 5000-long segment: the own-pixel predecessor sits inside a long run"""
    ev = K.hot_pixel_events()
    _not_vacuous(_fresh(f42).check2(arenas, 0, ev, P(2000, 1, 4000), "device", FE.DEVICE, "hot pixel"), "hot pixel")
    f42.check2(arenas, 0, shifted(ev, 1000), P(0, 0, 4000), "device", FE.HOST, "hot pixel, refractory alone, carried over")


def test_cameras_have_planes_of_their_own(f64, arenas):
    _fresh(f64)
    a = K.uniform_events(3000, 64, 48, 24000, seed=40)
    b = K.uniform_events(2500, 64, 48, 20000, seed=41)
    prm = P(MS, 1, 8 * MS)
    _not_vacuous(f64.check2(arenas, 0, a, prm, "device", FE.DEVICE, "cam 0"), "uniform 3000")
    f64.check2(arenas, 1, b, prm, "pageable", FE.DEVICE, "cam 1: nothing of cam 0's plane")
    f64.check2(arenas, 0, shifted(b, 2 * MS), prm, "device", FE.HOST, "cam 0 behind cam 1's call")
    f64.check2(arenas, 1, shifted(a, 2 * MS), P(0, 0, 8 * MS), "device", FE.DEVICE, "cam 1 again")


@pytest.mark.parametrize("kind", ["shuffled", "second_half_a_second_earlier", "nsec_above_2_30", "sec_2_32_minus_1",
                                  "equal_stamps"])
def test_non_monotonic_stamps(f64, arenas, kind):
    """the five kinds of test_ba_filter_gpu.test_non_monotonic_stamps with the refractory rule on"""
    n = 3000
    ev = K.uniform_events(n, 64, 48, 8 * n, seed=60, t0_us=5_000_000)
    rng = np.random.default_rng(61)
    t = event_ns(ev)
    if kind == "shuffled":
        t = rng.permutation(t)
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    elif kind == "second_half_a_second_earlier":
        t[n // 2:] -= 10 ** 9 - 12 * MS
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    elif kind == "nsec_above_2_30":
        ev["sec"], ev["nsec"] = 3, (1 << 30) + (t - t.min())
        assert (ev["nsec"] >= 1 << 30).all()
    elif kind == "sec_2_32_minus_1":
        ev["sec"], ev["nsec"] = (1 << 32) - 1, t - t.min()
        ev["sec"][::7] -= 1
        ev["nsec"][::7] += 10 ** 9 - 3 * MS
    else:
        t = (t // (2 * MS)) * (2 * MS)
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    _fresh(f64)
    window = 2 * MS if kind == "equal_stamps" else MS
    fr = f64.check2(arenas, 0, ev, P(window, 1, 8 * MS), "device", FE.DEVICE, kind)
    _not_vacuous(fr, kind)
    f64.check2(arenas, 0, ev[::-1].copy(), P(window, 2, 3 * MS), "pageable", FE.HOST, (kind, "reversed, support 2"))
    f64.check2(arenas, 0, ev, P(0, 0, 8 * MS), "device", FE.DEVICE, (kind, "refractory alone"))


def test_old_and_new_entry_points_alternate_on_one_plane(f64, arenas):
    _fresh(f64)
    batches = [K.uniform_events(2049, 64, 48, 16000, seed=50 + k, t0_us=1_000_000_000 + 14_000 * k) for k in range(4)]
    f64.check(arenas, 0, batches[0], MS, 1, "device", FE.DEVICE, "old")
    f64.check2(arenas, 0, batches[1], P(MS, 1, 8 * MS), "device", FE.DEVICE, "new behind old")
    f64.check(arenas, 0, batches[2], 2 * MS, 2, "pageable", FE.HOST, "old behind new")
    f64.check2(arenas, 0, batches[3], P(0, 0, 8 * MS), "pinned", FE.HOST, "new, refractory alone")
    f64.check2(arenas, 0, shifted(batches[3], MS), P(MS, 1, 0), "device", FE.DEVICE, "new with the old rule")


# ---- the fields form --------------------------------------------------------------------------------------------------
FW, FH = 64, 48
FIELD_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4097)
FPRM = P(MS, 1, 4 * MS)
_field_cases = {}


def _field_case(layout, n):
    """a case of event_fields_ref in `layout` whose events lie on a 12 x 12 patch of the 64 x 48 sensor (a few outside
    the sensor), stamps stepping 0..59 us — and its records by the numpy restatement of the conversion"""
    key = (layout, n)
    if key not in _field_cases:
        c = RF.make_case(layout, n, seed=7000 + 13 * len(layout) + n, shift=0, polarity="pm1" if n % 2 else "mixed")
        rng = np.random.default_rng(n)
        x, y, t, p = c.fields.keep  # (views into c.raw: the case is rewritten in place)
        x[:] = np.where(rng.random(n) < 0.05, FW + rng.integers(0, 9, n), rng.integers(0, 12, n))
        y[:] = np.where(rng.random(n) < 0.05, FH + rng.integers(0, 9, n), rng.integers(0, 12, n))
        steps = np.cumsum(rng.integers(0, 60, n)) * (1000 if c.t_unit_ns == 1 else 1)
        t[:] = (int(t[0]) + steps).astype(t.dtype)
        c.x, c.y, c.t = x.copy(), y.copy(), t.copy()
        ev, bad = RF.expected(c)
        assert not bad.any()
        _field_cases[key] = (c, ev)
    return _field_cases[key]


@pytest.fixture(scope="module")
def pair():
    """two handles advanced side by side: `a` filters fields, `b` converts and filters the records"""
    a, b = Filtered2(FW, FH), Filtered2(FW, FH)
    yield a, b
    a.close(), b.close()


@pytest.mark.parametrize("layout", RF.LAYOUTS)
def test_fields_form_equals_convert_then_filter(pair, arenas, farenas, layout):
    fa, fb = pair
    _fresh(fa), _fresh(fb)
    combos = [("device", FE.DEVICE), ("pinned", FE.HOST), ("pageable", FE.DEVICE), ("device", FE.HOST),
              ("pageable", FE.HOST), ("pinned", FE.DEVICE)]
    L = fa.ft._hd.L
    for k, n in enumerate(FIELD_SIZES):
        case, ev = _field_case(layout, n)
        space, dst_space = combos[k % len(combos)]
        cam = k & 1
        tag = (layout, n, space, dst_space)
        # the two-call form on handle b: convert into device memory, filter the records
        fields, src_space = farenas.source(case, space)
        bad = C.c_uint64(9)
        desc = FE.fields_desc(fields)
        assert L.esvio_fe_convert_events(fb.ft._hd.h, C.byref(desc), n, src_space, arenas.dev_src, FE.DEVICE, C.byref(bad)) == 0, tag
        two = batch_call(fb.ft, arenas, cam, n, FPRM, dst_space, ev=arenas.dev_src, space=FE.DEVICE)
        one = batch_call(fa.ft, arenas, cam, n, FPRM, dst_space, fields=fields, space=src_space)
        assert one[0] == 0 and two[0] == 0, (tag, L.esvio_fe_last_error(fa.ft._hd.h))
        assert np.array_equal(one[1], two[1]), (tag, "flags", int((one[1] != two[1]).sum()))
        assert one[2:] == two[2:], (tag, one[2], two[2], one[5:], two[5:])
        # ... and both equal the restatement on the restated conversion's records
        want, want_rej, sup, refr = R2.filter_events(fa.B[cam], FW, FH, ev, FPRM.window_ns, FPRM.min_support,
                                                     FPRM.refractory_ns, want_parts=True)
        kept, last = R.kept_of(ev, want)
        assert np.array_equal(one[1], want) and one[2] == len(kept) and one[3] == kept.tobytes() and one[5] == want_rej, tag
        assert one[4] == (last.tobytes() if last is not None else bytes([GUARD]) * 16), tag
        if n >= 1023:
            _not_vacuous((float(want.sum()) / n, float((sup & refr).sum()) / max(int(sup.sum()), 1)), tag)


@pytest.mark.parametrize("kind", ["t_beyond_2_62", "negative_ticks"])
def test_bad_event_fails_the_call_and_leaves_the_plane(arenas, farenas, kind):
    f = Filtered2(FW, FH)
    L, h = f.ft._hd.L, f.ft._hd.h
    n = 1025
    good, ev_good = _field_case("soa_i64_ns", n)
    f.check2(arenas, 0, ev_good, FPRM, "device", FE.DEVICE, "a plane that is not fresh")
    for pos in (0, n // 2, n - 1):
        c = RF.make_case("soa_i64_ns", n, seed=1, shift=0)
        x, y, t, p = c.fields.keep
        x[:], y[:], t[:], p[:] = good.x, good.y, good.t + 2 * MS, good.p
        t[pos] = (1 << 62) + 1 if kind == "t_beyond_2_62" else -5  # (ticks = t + t_offset = -22)
        if pos == n // 2:
            t[pos + 1] = t[pos]
        n_bad = 2 if pos == n // 2 else 1
        for space in ("device", "pageable"):
            fields, src_space = farenas.source(c, space)
            rc, _, _, _, _, _, bad = batch_call(f.ft, arenas, 0, n, FPRM, FE.DEVICE, fields=fields, space=src_space)
            assert rc == -1 and bad == n_bad, (kind, pos, space, rc, bad)
            assert b"filter_batch" in L.esvio_fe_last_error(h) and b"stamp" in L.esvio_fe_last_error(h)
        # the next call equals the restatement advanced from the plane before the bad calls
        nxt = shifted(ev_good, (3 + pos % 3) * MS)
        f.check2(arenas, 0, nxt, FPRM, "device", FE.DEVICE, (kind, pos, "the call behind the bad one"))
    f.close()


def test_second_call_of_a_size_allocates_nothing(arenas, farenas):
    f = Filtered2(FW, FH)
    case, ev = _field_case("soa_u32_us", 4097)
    small, _ = _field_case("packed13_i64_us", 1025)
    combos = (("pageable", FE.HOST), ("pinned", FE.DEVICE), ("device", FE.DEVICE))
    for space, dst_space in combos:
        fields, src_space = farenas.source(case, space)
        assert batch_call(f.ft, arenas, 0, case.n, FPRM, dst_space, fields=fields, space=src_space)[0] == 0
    a1, mem1 = f.ft.latency_stats()["allocs"], f.ft.device_memory()[0]
    for space, dst_space in combos + (("device", FE.HOST),):
        for c in (case, small):
            fields, src_space = farenas.source(c, space)
            assert batch_call(f.ft, arenas, 1, c.n, FPRM, dst_space, fields=fields, space=src_space)[0] == 0
    _fresh(f).check2(arenas, 0, ev[:2047], P(0, 0, MS), "device", FE.DEVICE)  # (the restated planes did not follow the calls above)
    assert f.ft.latency_stats()["allocs"] == a1 and f.ft.device_memory()[0] == mem1
    f.close()


def test_python_mirror(f64, arenas):
    ev = K.uniform_events(2500, 64, 48, 20000, seed=95)
    _fresh(f64)
    prm = P(MS, 1, 4 * MS)
    want, rej = R2.filter_events(f64.B[0], 64, 48, ev, MS, 1, 4 * MS)
    kept, flags, n_rej = f64.ft.filter_batch(0, ev, prm)
    assert np.array_equal(flags, want) and n_rej == rej and kept.tobytes() == R.raw_records(ev)[want != 0].tobytes()
    fields = EventFields.from_arrays(ev["x"].copy(), ev["y"].copy(), event_ns(ev), ev["polarity"].astype(np.int8), t_unit_ns=1)
    want, rej = R2.filter_events(f64.B[1], 64, 48, ev, MS, 1, 4 * MS)
    dev, flags, n_rej = f64.ft.filter_batch(1, fields, prm, device=True)
    assert np.array_equal(flags, want) and dev.n == int(want.sum()) and n_rej == rej
    assert dev.last.tobytes() == R.raw_records(ev)[want != 0][-1].tobytes()
    dev.free()
    fields.keep[2][7] = -1
    with pytest.raises(FE.FrontendError) as e:
        f64.ft.filter_batch(1, fields, prm)
    assert e.value.n_bad == 1
    f64.check2(arenas, 1, shifted(ev, MS), prm, "device", FE.DEVICE, "behind the mirror's calls")


# ---- esvio_fe_track_batch ---------------------------------------------------------------------------------------------
SW, SH, PUBS = T.SW, T.SH, T.PUBS
TPRM = P(5 * MS, 1, 2 * MS)


@pytest.fixture(scope="module")
def scene():
    return T._scene()


def _tracker():
    return FE.FeatureTracker(FE.make_config(SW, SH, max_cnt=40))


def _fields_of(ev):
    """the records as separate arrays: x, y, int64 nanoseconds, polarity {-1, +1}"""
    return EventFields.from_arrays(ev["x"].copy(), ev["y"].copy(), event_ns(ev), np.where(ev["polarity"] > 0, 1, -1).astype(np.int8),
                                   t_unit_ns=1)


def _motion(left, f):
    t = event_times(left)
    return FE.make_motion(t[0] + 0.8 * (t[-1] - t[0]), v=(0.8, -0.3, 0.2), v_pre=(0.7, -0.25, 0.15),
                          accel=(4.0, 5.0, 3.0) if f % 2 else (0.5, 0.2, 0.1), omega=(0.3, -0.4, 0.6),
                          fx=0.9 * SW, fy=0.9 * SW, cx=SW / 2.0 + 3.5, cy=SH / 2.0 - 2.25)


def _finish(ft, out):
    out.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    ft.close()
    return out


def test_records_without_a_filter_are_the_track_call(scene):
    want = T._plain(scene)
    ft, got = _tracker(), []
    for f, (left, right, t_us) in enumerate(scene):
        info = ft.track_batch(left, right, cur_time=t_us * 1e-6, pub=PUBS[f])
        assert info.tracked == 1 and tuple(info.kept) == (len(left), len(right)) and info.cur_time == t_us * 1e-6
        got.append(T._snapshot(ft))
    T._same(_finish(ft, got), want, "track_batch, records")
    # ... with three batches announced
    ft, got, ahead = _tracker(), [], 0
    ft.set_lazy_new_stereo(True)
    ref = _tracker()
    ref.set_lazy_new_stereo(True)
    want = []
    for k, (left, right, t_us) in enumerate(scene):
        while ahead < min(k + 3, len(scene) - 1):
            ahead += 1
            for t in (ft, ref):
                t.set_next_batch(scene[ahead][2] * 1e-6, scene[ahead][0], scene[ahead][1], PUBS[ahead])
        ft.track_batch(left, right, cur_time=t_us * 1e-6, pub=PUBS[k])
        ref.trackEvent(t_us * 1e-6, left, right, PUBS[k])
        ft.finish(), ref.finish()
        got.append(T._snapshot(ft)), want.append(T._snapshot(ref))
    T._same(_finish(ft, got), _finish(ref, want), "track_batch, records, announced")
    T._same(got[:-1], T._plain(scene)[:-1], "announced equals plain")


def test_fields_without_a_filter_equal_track_event_fields(scene):
    a, b, got, want = _tracker(), _tracker(), [], []
    for f, (left, right, t_us) in enumerate(scene):
        fl, fr = _fields_of(left), _fields_of(right)
        if f % 2:  # (every other frame takes its stamp from the batch: the last left record's)
            info = a.track_batch(fl, fr, cur_time=None, pub=PUBS[f])
            cur = float(left[-1]["sec"]) + 1e-9 * float(left[-1]["nsec"])
            assert info.cur_time == cur
        else:
            cur = t_us * 1e-6
            a.track_batch(fl, right, cur_time=cur, pub=PUBS[f])  # (and a camera given as records beside the other's fields)
        b.trackEventFields(cur, fl, fr, PUBS[f])
        got.append(T._snapshot(a)), want.append(T._snapshot(b))
    assert len(want[-1][0]) > 5
    T._same(_finish(a, got), _finish(b, want), "track_batch, fields")


def test_records_with_the_first_rule_equal_track_event_filtered(scene):
    a, b, got, want = _tracker(), _tracker(), [], []
    prm = P(5 * MS, 1, 0)
    for f, (left, right, _) in enumerate(scene):
        info = a.track_batch(left, right, cur_time=None, pub=PUBS[f], params=prm)
        kept, t = b.trackEventFiltered(left, right, 5 * MS, 1, pub=PUBS[f])
        assert tuple(info.kept) == kept and info.cur_time == t and info.tracked == 1 and tuple(info.bad) == (0, 0)
        got.append(T._snapshot(a)), want.append(T._snapshot(b))
    assert len(want[-1][0]) > 5
    T._same(_finish(a, got), _finish(b, want), "track_batch, records, filter")


@pytest.mark.parametrize("mc", [False, True])
def test_filtered_fields_equal_the_two_step_form(scene, mc):
    """fields, support and refractory test, the stamp from the batch (and the motion-compensated overload) against
    convert_events, filter_batch per camera into device memory with last_kept, then the track call on the kept records.
    In front of frame 3: a left batch the filter empties — nothing is tracked, `out` is untouched, and the frames
    behind it equal a sequence that skipped it."""
    a, b, got, want, hold = _tracker(), _tracker(), [], [], []
    plane = R2.fresh_plane(SW, SH)  # (the left camera's, restated: for the fractions this comparison is made at)
    lonely = K.records([(5 + 9 * (i % 12), 5 + 9 * (i // 12), 1, 1000 * i) for i in range(60)])
    for f, (left, right, _) in enumerate(scene):
        if f == 3:
            a.filter_reset(), b.filter_reset()
            before = T._snapshot(a)
            info = a.track_batch(_fields_of(lonely), _fields_of(right), pub=True, params=TPRM,
                                 measurements=_motion(lonely, f) if mc else None)
            assert info.tracked == 0 and info.kept[0] == 0 and info.kept[1] > 0
            T._same([T._snapshot(a)], [before], "an emptied left batch leaves `out` as it was")
            for cam, ev in ((0, lonely), (1, right)):  # (the planes have advanced: the two-step form's advance too)
                b.filter_batch(cam, ev, TPRM)
            plane = R2.fresh_plane(SW, SH)
            R2.filter_events(plane, SW, SH, lonely, TPRM.window_ns, TPRM.min_support, TPRM.refractory_ns)
        m = _motion(left, f) if mc else None
        info = a.track_batch(_fields_of(left), _fields_of(right), cur_time=None, pub=PUBS[f], params=TPRM, measurements=m)
        conv = [b.convert_events(_fields_of(left)), b.convert_events(_fields_of(right))]
        kept = [b.filter_batch(cam, conv[cam].arg, TPRM, device=True)[0] for cam in (0, 1)]
        cur = float(kept[0].last["sec"]) + 1e-9 * float(kept[0].last["nsec"])
        b.trackEvent(cur, kept[0].arg, kept[1].arg, PUBS[f], measurements=m)
        hold += conv + kept
        assert info.tracked == 1 and tuple(info.kept) == (kept[0].n, kept[1].n) and info.cur_time == cur
        fl, _, sup, refr = R2.filter_events(plane, SW, SH, left, TPRM.window_ns, TPRM.min_support, TPRM.refractory_ns, want_parts=True)
        assert info.kept[0] == int(fl.sum())
        _not_vacuous((float(fl.mean()), float((sup & refr).sum()) / max(int(sup.sum()), 1)), ("scene L", f, mc))
        got.append(T._snapshot(a)), want.append(T._snapshot(b))
    assert len(want[-1][0]) > 5
    T._same(_finish(a, got), _finish(b, want), ("track_batch, fields, filter", mc))
    for h in hold:
        h.free()


@pytest.mark.parametrize("filtered", [True, False])
def test_a_bad_event_in_a_batch_tracks_nothing(scene, filtered):
    """a BAD event in either camera: ESVIO_FE_EINVAL, info.bad exact per camera, nothing tracked; with a filter the plane
    of the camera that held it is as it was (the next call on that camera equals the restatement advanced from the
    plane before the bad call)"""
    ft = _tracker()
    prm = TPRM if filtered else None
    plane = R2.fresh_plane(SW, SH)
    left, right, _ = scene[0]
    info = ft.track_batch(_fields_of(left), _fields_of(right), pub=True, params=prm)
    assert info.tracked == 1 and tuple(info.bad) == (0, 0)
    if filtered:
        R2.filter_events(plane, SW, SH, left, TPRM.window_ns, TPRM.min_support, TPRM.refractory_ns)
    before = T._snapshot(ft)
    left, right, _ = scene[1]
    def refused(bad_cam, where):
        fields = [_fields_of(left), _fields_of(right)]
        for i in where:
            fields[bad_cam].keep[2][i] = -1 - i  # (ticks < 0)
        with pytest.raises(FE.FrontendError) as e:
            ft.track_batch(fields[0], fields[1], pub=True, params=prm)
        want_bad = [0, 0]
        want_bad[bad_cam] = len(where)
        assert "rc=-1" in str(e.value) and "stamp" in str(e.value) and "track_batch" in str(e.value)
        assert list(e.value.info.bad) == want_bad and e.value.info.tracked == 0, (bad_cam, list(e.value.info.bad))
        T._same([T._snapshot(ft)], [before], ("nothing tracked", bad_cam))

    refused(0, [5])
    refused(0, [len(left) - 1])
    if filtered:  # the left plane behind two bad left batches is the plane frame 0 left
        want, rej = R2.filter_events(plane, SW, SH, left, TPRM.window_ns, TPRM.min_support, TPRM.refractory_ns)
        _, flags, n_rej = ft.filter_batch(0, _fields_of(left), TPRM)
        assert np.array_equal(flags, want) and n_rej == rej
    refused(1, [0, len(right) - 1])  # (whether the left plane advances here is unspecified)
    ft.filter_reset()
    info = ft.track_batch(_fields_of(left), _fields_of(right), pub=True, params=prm)  # (the next call works normally)
    assert info.tracked == 1 and tuple(info.bad) == (0, 0)
    ft.close()


@pytest.mark.parametrize("announced", [False, True])
def test_filter_batch_between_track_calls_changes_no_tracking_result(scene, arenas, announced):
    want = T._plain(scene)
    f = Filtered2(SW, SH)
    ft, got, ahead = f.ft, [], 0
    if announced:
        ft.set_lazy_new_stereo(True)
    for k, (left, right, t_us) in enumerate(scene):
        while announced and ahead < min(k + 3, len(scene) - 1):
            ahead += 1
            ft.set_next_batch(scene[ahead][2] * 1e-6, scene[ahead][0], scene[ahead][1], PUBS[ahead])
        ft.trackEvent(t_us * 1e-6, left, right, PUBS[k])
        if k % 2:
            f.check2(arenas, k % 2, left, TPRM, "device", FE.DEVICE if k % 3 else FE.HOST, ("tap", announced, k))
        else:
            want_f, _ = R2.filter_events(f.B[0], SW, SH, right, TPRM.window_ns, TPRM.min_support, TPRM.refractory_ns)
            _, flags, _ = ft.filter_batch(0, _fields_of(right), TPRM)
            assert np.array_equal(flags, want_f), ("tap, fields", announced, k)
        if announced:
            ft.finish()
        got.append(T._snapshot(ft))
    got.append([ft.gettimesurface(0), ft.gettimesurface(1)])
    f.close()
    T._same(got, want, ("tap", announced))


def test_argument_errors(f64, arenas, scene):
    L, h = f64.ft._hd.L, f64.ft._hd.h
    ev = K.uniform_events(65, 64, 48, 520, seed=90)
    _fresh(f64).check2(arenas, 0, ev, P(MS, 1, MS), "device", FE.DEVICE, "scratch exists from here on")
    allocs, mem = f64.ft.latency_stats()["allocs"], f64.ft.device_memory()[0]
    src, _, _ = arenas.source(ev, "device")
    arenas.fill_dst(16 * 70)
    fields = _fields_of(ev)
    desc = FE.fields_desc(fields)
    nk = C.c_uint64(0)

    def call(ev=src, fields=None, prm=P(MS, 1, MS), space=FE.DEVICE, n=65):
        return L.esvio_fe_filter_batch(h, 0, ev, fields, n, space, C.byref(prm) if prm is not None else None, arenas.dev_dst,
                                       FE.DEVICE, C.byref(nk), None, None, None, None)

    reserved = P(MS, 1, MS)
    reserved.reserved = 1
    bad_desc = FE.fields_desc(fields)
    bad_desc.t_bits = 48
    for kw in (dict(ev=None), dict(fields=C.byref(desc), space=FE.HOST), dict(prm=None), dict(prm=reserved),
               dict(prm=P(0, 1, 0)), dict(prm=P((1 << 62) + 1, 1, 0)), dict(prm=P(MS, -1, 0)), dict(prm=P(MS, 9, 0)),
               dict(prm=P(MS, 1, -1)), dict(prm=P(MS, 1, (1 << 62) + 1)), dict(ev=None, fields=C.byref(bad_desc), space=FE.HOST)):
        assert call(**kw) == -1, kw
        assert b"filter_batch" in L.esvio_fe_last_error(h), kw
    assert (arenas.read_dst(16 * 70) == GUARD).all()
    assert call(n=0) == 0 and call(n=0, ev=None) == 0 and nk.value == 0                # n == 0 touches nothing
    assert call(prm=P(-7, 0, 0)) == 0 and nk.value == 65                               # (support 0: the window is not read)
    R2.filter_events(f64.B[0], 64, 48, ev, 0, 0, 0)
    assert call(prm=P(1 << 62, 8, 1 << 62)) == 0 and nk.value == 0                      # (the limits themselves are legal)
    R2.filter_events(f64.B[0], 64, 48, ev, 1 << 62, 8, 1 << 62)
    assert f64.ft.latency_stats()["allocs"] == allocs and f64.ft.device_memory()[0] == mem
    f64.check2(arenas, 0, ev, P(MS, 1, MS), "device", FE.DEVICE, "the plane behind the refused calls")
    # the batch call
    tr, info = FE.Tracks(), FE.BatchInfo()

    def batch(**kw):
        b = FE.Batch()
        b.left, b.right, b.nL, b.nR, b.space, b.pub_this_frame = src.value, src.value, 65, 65, FE.DEVICE, 1
        for k, v in kw.items():
            setattr(b, k, v)
        return L.esvio_fe_track_batch(h, C.byref(b), C.byref(tr), C.byref(info))

    for kw in (dict(left_fields=C.pointer(desc)), dict(left=None), dict(right=None), dict(reserved=3), dict(space=2),
               dict(filter=C.pointer(reserved)), dict(filter=C.pointer(P(MS, 9, 0))), dict(filter=C.pointer(P(0, 1, 0))),
               dict(filter=C.pointer(P(MS, 1, -1))), dict(left=None, left_fields=C.pointer(bad_desc))):
        assert batch(**kw) == -1, kw
        assert b"track_batch" in L.esvio_fe_last_error(h), kw
    # a fields batch or a filter while batches are announced
    ft = _tracker()
    left, right, t_us = scene[0]
    ft.set_next_batch(t_us * 1e-6 + 1.0, left, right, True)
    for kw in (dict(params=TPRM), dict()):
        with pytest.raises(FE.FrontendError) as e:
            if kw:
                ft.track_batch(left, right, cur_time=t_us * 1e-6, **kw)
            else:
                ft.track_batch(_fields_of(left), _fields_of(right), cur_time=t_us * 1e-6)
        assert "rc=-1" in str(e.value) and "announced" in str(e.value)
    ft.close()
