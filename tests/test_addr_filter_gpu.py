"""GPU: the address stage of the filter rule (esvio_fe_set_address_filter, esvio_fe_set_pixel_mask: step 1a) and
hot-pixel learning (esvio_fe_hot_learn, esvio_fe_hot_select) against the sequential restatement
tests/addr_filter_ref.py.  Integers only: every comparison is equality.  A handle and the restatement advance their
planes side by side, as in tests/test_batch_gpu.py, so a test's second call also checks what its first left in the
plane.  Every filter case asserts that it is not vacuous — the stage rejects some events and not all, and something is
kept — except at the two sizes (0 and 1 events) where one batch cannot hold both a rejected and a kept event."""
import ctypes as C

import numpy as np
import pytest

import addr_filter_cases as A
import addr_filter_ref as RA
import ba_filter_cases as K
import event_fields_ref as RF
import evt_ref as RE
import test_ba_filter_gpu as T
import test_batch_gpu as TB
import test_event_fields_gpu as TF
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, EventFields, event_times, make_events
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

MS = T.MS
GUARD = T.GUARD
P = FE.FilterParams
W, H = A.W, A.H
LAYOUTS = ("soa_i64_ns", "aos16_i64_us", "packed13_i64_us")  # separate arrays, an aligned AoS record, a packed one
OFFSETS = {"soa_i64_ns": -17, "aos16_i64_us": 999_999, "packed13_i64_us": 999_999}


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


def address_filter(stage):
    return FE.AddressFilter(stage.roi, stage.polarity, stage.flatten, stage.use_mask)


def mask_xy(stage, w):
    return np.array([(p % w, p // w) for p in sorted(stage.mask or ())], np.uint16).reshape(-1, 2)


def fields_case(ev, layout):
    """the records' fields in `layout` (stamps are whole microseconds) -> (case, the records conversion makes of them)"""
    n = len(ev)
    c = RF.make_case(layout, n, seed=1, shift=0)
    c.t_offset = OFFSETS[layout]
    c.fields = c.relocate(c.raw)
    x, y, t, p = c.fields.keep
    ns = TB.event_ns(ev)
    assert (ns % 1000 == 0).all()
    x[:], y[:] = ev["x"], ev["y"]
    t[:] = (ns if c.t_unit_ns == 1 else ns // 1000) - c.t_offset
    p[:] = np.where(ev["polarity"] != 0, 1, -1)
    c.x, c.y, c.t, c.p = x.copy(), y.copy(), t.copy(), p.copy()
    rec, bad = RF.expected(c)
    assert not bad.any()
    return c, rec


class Staged:
    """a handle, the restatement's planes of its two cameras and each camera's stage, advanced together"""

    def __init__(self, w, h, **kw):
        self.w, self.h = w, h
        self.ft = FE.FeatureTracker(FE.make_config(w, h, max_cnt=kw.pop("max_cnt", 40), **kw))
        self.stage = [None, None]
        self.fresh()

    def fresh(self):
        self.B = [RA.fresh_plane(self.w, self.h), RA.fresh_plane(self.w, self.h)]

    def close(self):
        self.ft.close()

    def set_stage(self, cam, stage):
        self.stage[cam] = stage
        self.ft.set_address_filter(cam, address_filter(stage) if stage is not None else None)
        if stage is not None and stage.mask is not None:
            self.ft.set_pixel_mask(cam, mask_xy(stage, self.w))

    def check(self, arenas, farenas, cam, ev, prm, how, tag):
        """one call equals the restatement.  how: ("records", space, dst_space), ("fields", layout, space, dst_space) or
        ("filter_events", space, dst_space).  -> (n rejected by the stage, n kept)"""
        stage = self.stage[cam]
        ev = ev.copy()
        n = len(ev)
        if how[0] == "fields":
            case, ev = fields_case(ev, how[1])
        else:
            RA.raw_records(ev)[:, 13:] = ((np.arange(3 * n) * 5 + 3) & 255).astype(np.uint8).reshape(-1, 3)  # (the padding travels)
        want, want_rej, by_stage = RA.filter_events(self.B[cam], self.w, self.h, ev, prm.window_ns, prm.min_support,
                                                    prm.refractory_ns, stage)
        kept, last = RA.kept_of(ev, want, stage)
        if how[0] == "fields":
            fields, src_space = farenas.source(case, how[2])
            got = TB.batch_call(self.ft, arenas, cam, n, prm, how[3], fields=fields, space=src_space)
        elif how[0] == "records":
            src, src_space, keep = arenas.source(ev, how[1])
            got = TB.batch_call(self.ft, arenas, cam, n, prm, how[2], ev=src, space=src_space)
        else:
            assert prm.refractory_ns == 0 and prm.min_support >= 1
            got = T.Filtered.call(self, arenas, cam, ev, prm.window_ns, prm.min_support, how[1], how[2]) + (0,)
        rc, flags, k, rec, last_got, rej, bad = got
        assert rc == 0 and bad == 0, (tag, rc, self.ft._hd.L.esvio_fe_last_error(self.ft._hd.h))
        if not np.array_equal(flags, want):
            i = int(np.flatnonzero(flags != want)[0])
            raise AssertionError((tag, "first differing flag at event", i, ev[i], int(flags[i]), int(want[i]),
                                  int((flags != want).sum()), n))
        assert k == len(kept) and rej == want_rej, (tag, k, len(kept), rej, want_rej)
        assert rec == kept.tobytes(), (tag, "kept records")
        assert last_got == (last.tobytes() if last is not None else bytes([GUARD]) * 16), (tag, "last_kept")
        return by_stage, k


def not_vacuous(res, n, tag):
    by_stage, kept = res
    print(tag, "n %d: %d rejected by the stage, %d kept" % (n, by_stage, kept))
    if n >= 2:
        assert 0 < by_stage < n and 0 < kept, ("a comparison in which the stage rejects nothing or everything shows little", tag, by_stage, kept, n)


@pytest.fixture(scope="module")
def s42():
    f = Staged(W, H)
    yield f
    f.close()


@pytest.fixture(scope="module")
def s64():
    f = Staged(64, 48)
    yield f
    f.close()


def _fresh(f, stage, cams=(0, 1)):
    f.ft.filter_reset()
    f.fresh()
    for cam in cams:
        f.set_stage(cam, stage)
    return f


# ---- 1. the filter against the restatement ----------------------------------------------------------------------------
HOT_STAGE = dict(roi=A.FULL, use_mask=1, mask=[A.pix(A.HOT)])
RECORD_WAYS = [("records", "device", FE.DEVICE), ("records", "pageable", FE.HOST), ("records", "pinned", FE.DEVICE),
               ("records", "device", FE.HOST)]


@pytest.mark.parametrize("prm", [P(2000, 1, 0), P(0, 0, 0)], ids=["support1", "address_alone"])
def test_hot_pixel_stream_with_its_pixel_masked(s42, arenas, farenas, prm):
    ev = K.hot_pixel_events()
    ways = RECORD_WAYS + [("fields", "soa_i64_ns", "device", FE.DEVICE), ("fields", "aos16_i64_us", "pageable", FE.HOST),
                          ("fields", "packed13_i64_us", "pinned", FE.DEVICE), ("filter_events", "device", FE.DEVICE)]
    for how in ways:
        if how[0] == "filter_events" and prm.min_support == 0:
            continue  # (esvio_fe_filter_events has no support 0)
        _fresh(s42, RA.Stage(**HOT_STAGE))
        res = s42.check(arenas, farenas, 0, ev, prm, how, ("hot", how))
        assert res[0] == 5000
        not_vacuous(res, len(ev), ("hot", how))
        # a second call on the plane the first left, through another way in
        again = TB.shifted(ev, 1000)
        not_vacuous(s42.check(arenas, farenas, 0, again, prm, RECORD_WAYS[1] if how[0] == "fields" else ways[4], ("hot again", how)),
                    len(ev), ("hot again", how))


UNIFORM_STAGES = [dict(roi=A.ROI, polarity=1, flatten=2), dict(roi=A.ROI, polarity=2, flatten=1),
                  dict(roi=A.ROI, polarity=1, flatten=1), dict(roi=A.ROI, polarity=2, flatten=2)]


@pytest.mark.parametrize("n", K.SWEEP_SIZES)
def test_size_sweep_with_roi_polarity_and_flatten(s42, arenas, farenas, n):
    """the wave, the four-event group and the sort tile: each size with the ROI and both polarity modes, each behind
    both flatten values, as records and (n > 0) as fields, twice on one plane"""
    ev = K.sweep_events(n)
    for k, kw in enumerate(UNIFORM_STAGES):
        stage = RA.Stage(**kw)
        prm = P(MS, 1, 0) if k % 2 == 0 else P(0, 0, MS // 10)
        how = RECORD_WAYS[k % 4]
        _fresh(s42, stage)
        not_vacuous(s42.check(arenas, farenas, 0, ev, prm, how, ("sweep", n, k)), n, ("sweep", n, k))
        if n == 0:
            continue
        how2 = ("fields", LAYOUTS[k % 3], ("device", "pageable", "pinned")[k % 3], FE.HOST if k % 2 else FE.DEVICE)
        not_vacuous(s42.check(arenas, farenas, 0, TB.shifted(ev, MS // 2), prm, how2, ("sweep, carried over", n, k)), n,
                    ("sweep, carried over", n, k))
    if n >= 63:  # the entry point of the first rule, with a stage
        _fresh(s42, RA.Stage(**UNIFORM_STAGES[0]))
        not_vacuous(s42.check(arenas, farenas, 0, ev, P(MS, 1, 0), ("filter_events", "pageable", FE.HOST), ("sweep, old entry", n)), n, n)


def test_counts_of_the_uniform_stream(s42, arenas, farenas):
    u = A.uniform4097()
    _fresh(s42, RA.Stage(A.FULL, polarity=1))
    assert s42.check(arenas, farenas, 0, u, P(0, 0, 0), RECORD_WAYS[0], "ON only") == (4097 - 2098, 2098)
    _fresh(s42, RA.Stage(A.ROI))
    assert s42.check(arenas, farenas, 0, u, P(0, 0, 0), ("fields", "soa_i64_ns", "device", FE.DEVICE), "ROI") == (4097 - 824, 824)


def test_mask_word_edges_on_the_wider_sensor(s64, arenas, farenas):
    """64 x 48: a row is two whole mask words; pixels at both ends of words of both cameras, each camera its own mask"""
    ev = A.with_outsiders(A.uniform_wide(4097, seed=77), 64, 48)
    masks = [[0, 31, 32, 63, 64, 64 * 47 + 63] + list(range(64 * 10, 64 * 10 + 40)),
             [1, 30, 33, 95, 96] + list(range(64 * 20 + 31, 64 * 20 + 34))]
    for cam in (0, 1):
        _fresh(s64, None)
        s64.set_stage(cam, RA.Stage((0, 0, 63, 47), use_mask=1, mask=masks[cam]))
        res = s64.check(arenas, farenas, cam, ev, P(MS, 1, 4 * MS), RECORD_WAYS[cam], ("wide", cam))
        not_vacuous(res, len(ev), ("wide", cam))
        other = s64.check(arenas, farenas, 1 - cam, ev, P(MS, 1, 4 * MS), RECORD_WAYS[2], ("wide, the camera without a stage", cam))
        assert other[0] == 0
        not_vacuous(s64.check(arenas, farenas, cam, TB.shifted(ev, MS), P(0, 0, 0), ("fields", "packed13_i64_us", "device", FE.HOST),
                              ("wide again", cam)), len(ev), ("wide again", cam))
    _fresh(s64, None)


# ---- 2. the GPU against itself ------------------------------------------------------------------------------------------
def test_a_stage_equals_the_stream_without_its_rejected_events(arenas):
    a, b = Staged(W, H), Staged(W, H)
    try:
        for ev, kw in ((A.with_outsiders(K.hot_pixel_events(), W, H), HOT_STAGE),
                       (A.with_outsiders(A.uniform4097(), W, H), dict(roi=A.ROI, polarity=2, flatten=1, use_mask=1,
                                                                      mask=[A.pix((10, 10)), A.pix((20, 15))]))):
            stage = RA.Stage(**kw)
            prm = P(2000, 1, 4000) if kw is HOT_STAGE else P(MS, 1, 2 * MS)
            _fresh(a, stage), _fresh(b, None)
            prime = RA.without_stage(ev, stage, W, H)
            assert 0 < len(prime) < len(ev)
            src, sp, keep = arenas.source(ev, "device")
            ga = TB.batch_call(a.ft, arenas, 0, len(ev), prm, FE.DEVICE, ev=src, space=sp)
            src, sp, keep = arenas.source(prime, "device")
            gb = TB.batch_call(b.ft, arenas, 0, len(prime), prm, FE.DEVICE, ev=src, space=sp)
            assert ga[0] == 0 and gb[0] == 0
            assert ga[2] == gb[2] > 0 and ga[3] == gb[3] and ga[4] == gb[4], "kept records, last_kept"
            assert ga[5] == gb[5] + (len(ev) - len(prime))
            # the next call, without a stage on either, on each plane
            a.set_stage(0, None)
            nxt = TB.shifted(ev, 3000 if kw is HOT_STAGE else MS)
            src, sp, keep = arenas.source(nxt, "device")
            na = TB.batch_call(a.ft, arenas, 0, len(nxt), prm, FE.HOST, ev=src, space=sp)
            nb = TB.batch_call(b.ft, arenas, 0, len(nxt), prm, FE.HOST, ev=src, space=sp)
            assert na[0] == 0 and np.array_equal(na[1], nb[1]) and na[2:] == nb[2:] and 0 < na[2] < len(nxt)
    finally:
        a.close(), b.close()


# ---- 3. settings --------------------------------------------------------------------------------------------------------
def test_without_a_stage_the_chain_is_the_one_it_was(arenas, farenas):
    f = Staged(W, H)
    try:
        ev = K.sweep_events(2049)
        f.ft.set_profiling(True)
        f.check(arenas, farenas, 0, ev, P(MS, 1, 0), RECORD_WAYS[0], "no stage")
        st = f.ft.kernel_stats(stages=True)
        assert st["k_sae_keys"]["launches"] == 1 and st["k_baf_keys_addr"]["launches"] == 0 and st["k_baf_emit"]["launches"] == 1
        f.set_stage(0, RA.Stage(**UNIFORM_STAGES[0]))
        f.ft.reset_kernel_stats()
        f.check(arenas, farenas, 0, TB.shifted(ev, MS), P(MS, 1, 0), RECORD_WAYS[0], "a stage")
        st = f.ft.kernel_stats(stages=True)
        assert st["k_sae_keys"]["launches"] == 0 and st["k_baf_keys_addr"]["launches"] == 1 and st["k_radix_pass"]["launches"] == 2
        f.set_stage(0, None)
        f.ft.reset_kernel_stats()
        f.check(arenas, farenas, 0, TB.shifted(ev, 2 * MS), P(MS, 1, 0), RECORD_WAYS[0], "no stage again")
        st = f.ft.kernel_stats(stages=True)
        assert st["k_sae_keys"]["launches"] == 1 and st["k_baf_keys_addr"]["launches"] == 0
    finally:
        f.close()


def test_settings_survive_resets_and_argument_errors_change_nothing(arenas, farenas):
    f = Staged(W, H)
    L, h = f.ft._hd.L, f.ft._hd.h
    try:
        assert len(f.ft.pixel_mask(0)) == 0
        ev = A.uniform4097()
        # use_mask with no mask set rejects nothing
        f.set_stage(0, RA.Stage(A.FULL, use_mask=1))
        assert f.check(arenas, farenas, 0, ev, P(0, 0, 0), RECORD_WAYS[0], "no mask set")[0] == 0
        xy = [(41, 41), (31, 0), (5, 7), (32, 0), (0, 0), (21, 1), (5, 7)]  # (unordered, one pair twice)
        stage = RA.Stage(A.ROI, polarity=1, flatten=1, use_mask=1, mask=[A.pix(p) for p in xy])
        f.set_stage(0, stage)
        raster = sorted(set(xy), key=lambda p: A.pix(p))
        assert f.ft.pixel_mask(0).tolist() == [list(p) for p in raster] and len(f.ft.pixel_mask(1)) == 0
        cap, n = np.zeros((3, 2), np.uint16), C.c_size_t(0)
        assert L.esvio_fe_get_pixel_mask(h, 0, C.c_void_p(cap.ctypes.data), 3, C.byref(n)) == -1 and n.value == len(raster)
        assert cap.tolist() == [list(p) for p in raster[:3]]
        # argument errors: nothing changes
        bad_filters = [FE.AddressFilter((5, 7, 42, 20)), FE.AddressFilter((5, 7, 30, 42)), FE.AddressFilter((6, 7, 5, 20)),
                       FE.AddressFilter((5, 8, 30, 7)), FE.AddressFilter(A.FULL, polarity=3), FE.AddressFilter(A.FULL, polarity=-1),
                       FE.AddressFilter(A.FULL, flatten=3), FE.AddressFilter(A.FULL, use_mask=2)]
        r = FE.AddressFilter(A.FULL)
        r.reserved = 1
        for a in bad_filters + [r]:
            assert L.esvio_fe_set_address_filter(h, 0, C.byref(a)) == -1 and b"set_address_filter" in L.esvio_fe_last_error(h)
        assert L.esvio_fe_set_address_filter(h, 2, C.byref(FE.AddressFilter(A.FULL))) == -1
        out = np.array([[3, 3], [42, 3]], np.uint16)
        assert L.esvio_fe_set_pixel_mask(h, 0, C.c_void_p(out.ctypes.data), 2) == -1 and b"set_pixel_mask" in L.esvio_fe_last_error(h)
        out[1] = (3, 42)
        assert L.esvio_fe_set_pixel_mask(h, 0, C.c_void_p(out.ctypes.data), 2) == -1
        assert L.esvio_fe_set_pixel_mask(h, 0, None, 2) == -1 and L.esvio_fe_set_pixel_mask(h, -1, None, 0) == -1
        assert f.ft.pixel_mask(0).tolist() == [list(p) for p in raster]
        not_vacuous(f.check(arenas, farenas, 0, ev, P(MS, 1, 0), RECORD_WAYS[0], "behind the refused calls"), len(ev), "refused")
        # the settings survive esvio_fe_reset and esvio_fe_filter_reset; the planes do not
        f.ft.reset()
        f.fresh()
        assert f.ft.pixel_mask(0).tolist() == [list(p) for p in raster]
        not_vacuous(f.check(arenas, farenas, 0, ev, P(MS, 1, 0), RECORD_WAYS[3], "behind reset"), len(ev), "reset")
        f.ft.filter_reset()
        f.fresh()
        not_vacuous(f.check(arenas, farenas, 0, ev, P(MS, 1, 0), ("fields", "aos16_i64_us", "device", FE.DEVICE), "behind filter_reset"),
                    len(ev), "filter_reset")
        # n == 0 clears the mask; NULL takes the stage away
        f.ft.set_pixel_mask(0, [])
        stage.mask = set()
        assert len(f.ft.pixel_mask(0)) == 0
        f.check(arenas, farenas, 0, TB.shifted(ev, MS), P(MS, 1, 0), RECORD_WAYS[0], "an empty mask")
        f.set_stage(0, None)
        assert f.check(arenas, farenas, 0, TB.shifted(ev, 2 * MS), P(MS, 1, 0), RECORD_WAYS[0], "no stage")[0] == 0
    finally:
        f.close()


# ---- 4. learning and selection against the restatement ----------------------------------------------------------------
def info_dict(info):
    return dict(events=info.events, span_ns=info.span_ns, threshold=info.threshold, above=info.above, selected=info.selected)


def same_selection(ft, cam, hot, tag, **kw):
    want_xy, want_cnt, want_info = hot.select(kw["max_pixels"], kw.get("min_count", 1), kw.get("min_rate_hz", 0), kw.get("mean_factor", 0))
    xy, cnt, info = ft.hot_select(cam, FE.HotParams(**kw))
    assert info_dict(info) == want_info, (tag, info_dict(info), want_info)
    assert [tuple(p) for p in xy.tolist()] == want_xy and cnt.tolist() == want_cnt, (tag, xy.tolist(), want_xy)
    return xy, cnt, info


SELECTIONS = [dict(max_pixels=8, min_rate_hz=100_000), dict(max_pixels=4, min_rate_hz=10_000), dict(max_pixels=8, mean_factor=100),
              dict(max_pixels=4096, min_rate_hz=10_000), dict(max_pixels=8, min_count=320), dict(max_pixels=5, min_count=1)]


def fields_of(ev):
    return EventFields.from_arrays(ev["x"].copy(), ev["y"].copy(), TB.event_ns(ev), np.where(ev["polarity"] > 0, 1, -1).astype(np.int8),
                                   t_unit_ns=1)


@pytest.mark.parametrize("way", ["records_two_calls", "records_one_call_device", "fields_two_calls", "fields_one_call_device"])
def test_learning_and_the_four_selections(farenas, way):
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    try:
        ev = K.hot_pixel_events()
        hot = RA.Hot(W, H)
        same_selection(ft, 0, hot, "nothing learned", max_pixels=8)
        hot.learn(ev)
        parts = [ev[:3001], ev[3001:]] if "two" in way else [ev]
        bufs = []
        for part in parts:
            if way.startswith("records"):
                if "device" in way:
                    bufs.append(FE.EventBuffer(part, FE.DEVICE))
                    ft.hot_learn(0, bufs[-1].arg)
                else:
                    ft.hot_learn(0, part)
            elif "device" in way:
                case, _ = fields_case(part, "packed13_i64_us")
                fields, space = farenas.source(case, "device")
                ft.hot_learn(0, fields, src_space=space)
            else:
                ft.hot_learn(0, fields_of(part))
        for kw in SELECTIONS:
            xy, cnt, info = same_selection(ft, 0, hot, (way, kw), **kw)
        xy, cnt, info = same_selection(ft, 0, hot, way, **SELECTIONS[1])
        assert [tuple(p) for p in xy.tolist()] == [(20, 20), (20, 21), (19, 19), (21, 19)] and info.threshold == 151 and info.above == 9
        assert same_selection(ft, 0, hot, way, **SELECTIONS[0])[2].threshold == 1507
        assert same_selection(ft, 0, hot, way, **SELECTIONS[2])[2].threshold == 567
        same_selection(ft, 1, RA.Hot(W, H), "the other camera learned nothing", max_pixels=8)
        # the filter's reset leaves the state, the handle's and the stage's own clear it
        ft.filter_reset()
        same_selection(ft, 0, hot, "behind filter_reset", **SELECTIONS[1])
        ft.hot_reset() if "two" in way else ft.reset()
        same_selection(ft, 0, RA.Hot(W, H), "behind the reset", max_pixels=8)
        for b in bufs:
            b.free()
    finally:
        ft.close()


def test_selections_in_turn_on_a_sensor_of_several_sort_tiles():
    """the selection sorts one key per PIXEL, 4 x 8 bits, in scratch of the stage's own that a memset clears whole before
    every call: the sort's size and digit width are the sensor's and cannot change within a handle.  What changes from
    call to call is the keys — at 96 x 72 (6912 keys: three full sort tiles and a partial one) a selection over many
    counted pixels, one over five (every other key is 0xffffffff, next to the last tile's padding lanes), one over none,
    and the first again, each as the restatement's: equal counts in pixel order."""
    w, h = 96, 72
    ft = FE.FeatureTracker(FE.make_config(w, h, max_cnt=40))
    try:
        hot = RA.Hot(w, h)
        big = K.uniform_events(20000, w, h, 50_000, seed=71)
        few = K.uniform_events(5, w, h, 50, seed=72, t0_us=1_000_100_000)

        def learn(ev):
            hot.learn(ev)
            ft.hot_learn(0, ev)

        def selections(tag):
            for kw in (dict(max_pixels=4096, min_count=1), dict(max_pixels=4096, min_count=4), dict(max_pixels=7, min_count=1)):
                same_selection(ft, 0, hot, (tag, kw), **kw)

        learn(big)
        assert same_selection(ft, 0, hot, "many", max_pixels=4096, min_count=1)[2].above > 4096
        selections("many")
        ft.hot_reset()
        hot = RA.Hot(w, h)
        learn(few)
        assert same_selection(ft, 0, hot, "five", max_pixels=4096, min_count=1)[2].selected in (4, 5)
        selections("five")
        ft.hot_reset()
        hot = RA.Hot(w, h)
        selections("none")
        learn(big)
        selections("many again")
    finally:
        ft.close()


def test_out_of_sensor_events_and_a_bad_stamp():
    ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=40))
    try:
        ev = A.with_outsiders(A.uniform4097(), W, H)
        hot = RA.Hot(W, H)
        ft.hot_learn(1, ev)
        hot.learn(ev)
        assert hot.N < len(ev)
        same_selection(ft, 1, hot, "out-of-sensor events", max_pixels=4096, min_count=1)
        more = TB.shifted(A.with_outsiders(K.hot_pixel_events(), W, H, every=89), 5 * MS)
        fields = fields_of(more)
        bad = [7, 4000, len(more) - 1]
        for i in bad:
            fields.keep[2][i] = -3 - i  # (ticks < 0)
        with pytest.raises(FE.FrontendError) as e:
            ft.hot_learn(1, fields)
        assert e.value.n_bad == 3 and "hot_learn" in str(e.value) and "rc=-1" in str(e.value)
        hot.learn(more, bad=bad)  # the others are counted
        same_selection(ft, 1, hot, "behind a BAD call", max_pixels=4096, min_count=1)
        same_selection(ft, 1, hot, "behind a BAD call", max_pixels=16, min_rate_hz=5000, mean_factor=20)
    finally:
        ft.close()


def test_every_pixel_ties_and_install(arenas, farenas):
    """every pixel holds the same count: the order is the index alone, the cut falls inside the tie; install makes the
    selection the camera's mask, and the filter then rejects exactly those pixels' events"""
    f = Staged(W, H)
    L, h = f.ft._hd.L, f.ft._hd.h
    try:
        yy, xx = np.divmod(np.arange(W * H), W)
        t_us = 1_000_000_000 + np.arange(W * H)
        ev = make_events(np.tile(xx, 3), np.tile(yy, 3), np.concatenate([t_us + k * 5000 for k in range(3)]), np.tile(xx & 1, 3))
        hot = RA.Hot(W, H)
        f.ft.hot_learn(0, ev)
        hot.learn(ev)
        xy, cnt, info = same_selection(f.ft, 0, hot, "ties", max_pixels=100, min_count=3)
        assert info.above == W * H and cnt.tolist() == [3] * 100 and [A.pix(p) for p in xy.tolist()] == list(range(100))
        same_selection(f.ft, 0, hot, "ties, nothing reaches 4", max_pixels=100, min_count=4)
        # selected > cap with a list: EINVAL, info filled, nothing installed
        f.ft.set_pixel_mask(0, [(9, 9)])
        with pytest.raises(FE.FrontendError) as e:
            f.ft.hot_select(0, FE.HotParams(max_pixels=100, min_count=3, install=True), cap=40)
        assert e.value.info.selected == 100 and e.value.info.above == W * H and f.ft.pixel_mask(0).tolist() == [[9, 9]]
        # parameter errors
        for kw in (dict(max_pixels=0), dict(max_pixels=4097), dict(min_count=0), dict(min_rate_hz=(1 << 20) + 1), dict(mean_factor=(1 << 20) + 1)):
            prm = FE.HotParams(**kw)
            assert L.esvio_fe_hot_select(h, 0, C.byref(prm), None, None, 0, None) == -1 and b"hot_select" in L.esvio_fe_last_error(h), kw
        prm = FE.HotParams()
        prm.reserved = 1
        assert L.esvio_fe_hot_select(h, 0, C.byref(prm), None, None, 0, None) == -1 and L.esvio_fe_hot_select(h, 2, C.byref(FE.HotParams()), None, None, 0, None) == -1
        assert f.ft.pixel_mask(0).tolist() == [[9, 9]]
        # install: the mask is the list, sorted; on the hot stream learned on top, by rate
        f.ft.hot_reset()
        hot.reset()
        hp = K.hot_pixel_events()
        f.ft.hot_learn(0, hp)
        hot.learn(hp)
        xy, cnt, info = f.ft.hot_select(0, FE.HotParams(max_pixels=4, min_rate_hz=10_000, install=True))
        assert [tuple(p) for p in xy.tolist()] == hot.select(4, min_rate_hz=10_000)[0]
        assert f.ft.pixel_mask(0).tolist() == sorted(xy.tolist(), key=lambda p: A.pix(p)) and len(f.ft.pixel_mask(1)) == 0
        stage = RA.Stage(A.FULL, use_mask=1, mask=[A.pix(p) for p in xy.tolist()])
        f.stage[0] = stage
        f.ft.set_address_filter(0, address_filter(stage))
        res = f.check(arenas, farenas, 0, hp, P(2000, 1, 0), RECORD_WAYS[0], "the installed mask")
        assert res[0] == int(cnt.sum())
        not_vacuous(res, len(hp), "the installed mask")
        # nothing learned, install: the empty mask
        f.ft.hot_reset()
        xy, cnt, info = f.ft.hot_select(0, FE.HotParams(max_pixels=8, install=True))
        assert info_dict(info) == dict(events=0, span_ns=0, threshold=1, above=0, selected=0) and len(f.ft.pixel_mask(0)) == 0
    finally:
        f.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------
EW, EH, FRAMES = 192, 144, 5
HOT_PIXELS = [[(50, 40), (100, 70), (150, 120)], [(43, 40), (93, 70), (191, 143)]]
EPRM = P(5 * MS, 1, 0)


def _inject(ev, pixels, period_us=50):
    """the batch with every pixel of `pixels` firing on the period's grid, merged in stamp order"""
    t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
    grid = np.arange(-(-int(t[0]) // period_us) * period_us, int(t[-1]) + 1, period_us)
    parts = [ev] + [make_events(np.full(len(grid), x), np.full(len(grid), y), grid, (grid // period_us + k) & 1)
                    for k, (x, y) in enumerate(pixels)]
    allev = np.concatenate([RA.raw_records(p) for p in parts])  # (whole records: numpy's own concatenation packs them)
    ta = np.concatenate([t] + [grid] * len(pixels))
    return allev[np.argsort(ta, kind="stable")].copy().view(EVENT_DTYPE).reshape(-1)


def _without(ev, pixels):
    hit = np.zeros(len(ev), bool)
    for x, y in pixels:
        hit |= (ev["x"] == x) & (ev["y"] == y)
    return RA.raw_records(ev)[~hit].copy().view(EVENT_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def hot_scene():
    """the golden scene's generator (tests/golden/make_golden.py), three hot pixels per camera injected"""
    s = SceneStream(EW, EH, rate=1.5e5, n_rect=6, seed=2024, size=(25.0, 60.0), speed=(120.0, 260.0), disparity=7,
                    t0_us=1_700_000_000_000_000)
    frames = []
    for _ in range(FRAMES):
        left, right, _ = s.next_batch()
        assert not any(((ev["x"] == x) & (ev["y"] == y)).sum() > 40 for cam, ev in enumerate((left, right)) for x, y in HOT_PIXELS[cam])
        frames.append((_inject(left, HOT_PIXELS[0]), _inject(right, HOT_PIXELS[1])))
    return frames


def test_learn_install_and_track_equals_tracking_the_cleaned_streams(hot_scene):
    a, b = (FE.FeatureTracker(FE.make_config(EW, EH, max_cnt=60, min_dist=6)) for _ in range(2))
    try:
        ref = [RA.Hot(EW, EH), RA.Hot(EW, EH)]
        for left, right in hot_scene:
            for cam, ev in enumerate((left, right)):
                a.hot_learn(cam, ev)
                ref[cam].learn(ev)
        for cam in (0, 1):
            xy, cnt, info = a.hot_select(cam, FE.HotParams(max_pixels=8, min_rate_hz=10_000, install=True))
            want = ref[cam].select(8, min_rate_hz=10_000)
            assert [tuple(p) for p in xy.tolist()] == want[0] and cnt.tolist() == want[1] and info_dict(info) == want[2]
            assert sorted(tuple(p) for p in xy.tolist()) == sorted(HOT_PIXELS[cam]), (cam, xy.tolist(), cnt.tolist())
            a.set_address_filter(cam, FE.AddressFilter((0, 0, EW - 1, EH - 1), use_mask=1))
        planes = [RA.fresh_plane(EW, EH), RA.fresh_plane(EW, EH)]
        for f, (left, right) in enumerate(hot_scene):
            pub = f != 2
            ia = a.track_batch(left, right, pub=pub, params=EPRM)
            ib = b.track_batch(_without(left, HOT_PIXELS[0]), _without(right, HOT_PIXELS[1]), pub=pub, params=EPRM)
            for cam, ev in enumerate((left, right)):
                stage = RA.Stage((0, 0, EW - 1, EH - 1), use_mask=1, mask=[A.pix(p, EW) for p in HOT_PIXELS[cam]])
                flags, rej, by = RA.filter_events(planes[cam], EW, EH, ev, EPRM.window_ns, EPRM.min_support, 0, stage)
                assert (ia.kept[cam], ia.rejected[cam]) == (int(flags.sum()), rej) and by > 1000 and ia.kept[cam] == ib.kept[cam] > 0
                assert ib.rejected[cam] == rej - by
            assert ia.tracked == ib.tracked == 1 and ia.cur_time == ib.cur_time
            T._same([T._snapshot(a)], [T._snapshot(b)], ("frame", f))
        T._same([[a.gettimesurface(0), a.gettimesurface(1)]], [[b.gettimesurface(0), b.gettimesurface(1)]], "time surfaces")
        assert len(a.ids) > 5 and len(a.ids_right) > 0
    finally:
        a.close(), b.close()


def test_the_stage_runs_behind_the_decoder_and_in_the_feed(hot_scene):
    left, right = hot_scene[0]
    stages = [RA.Stage((0, 0, EW - 1, EH - 1), use_mask=1, mask=[A.pix(p, EW) for p in HOT_PIXELS[cam]]) for cam in (0, 1)]
    # esvio_fe_track_raw with a filter: the records in read-out order inside equal stamps, as EVT3 words
    ft = FE.FeatureTracker(FE.make_config(EW, EH, max_cnt=60))
    try:
        base = int(left["sec"][0]) * 10 ** 6 - 1000
        recs, words = [], []
        for cam, ev in enumerate((left, right)):
            x, y, p = (ev[k].astype(np.int64) for k in ("x", "y", "polarity"))
            t = ev["sec"].astype(np.int64) * 10 ** 6 + ev["nsec"].astype(np.int64) // 1000
            o = RE.readout_order(x, y, p, t)
            recs.append(make_events(x[o], y[o], t[o], p[o]))
            words.append(RE.encode(RE.EVT3, x[o], y[o], p[o], t[o] - base))
            ft.set_pixel_mask(cam, HOT_PIXELS[cam])
            ft.set_address_filter(cam, address_filter(stages[cam]))
        info, raw = ft.track_raw(RE.EVT3, words[0], words[1], base, True, params=EPRM)
        for cam in (0, 1):
            flags, rej, by = RA.filter_events(RA.fresh_plane(EW, EH), EW, EH, recs[cam], EPRM.window_ns, EPRM.min_support, 0, stages[cam])
            assert raw[cam].events == len(recs[cam]) and by > 1000
            assert (info.kept[cam], info.rejected[cam]) == (int(flags.sum()), rej), (cam, info.kept[cam], info.rejected[cam])
        assert info.tracked == 1
        # the feed with a filter, on the same handle behind a reset: the settings are still there
        ft.reset()
        ft.feed_open(30.0, params=EPRM)
        for cam, ev in enumerate((left, right)):
            flags, rej, by = RA.filter_events(RA.fresh_plane(EW, EH), EW, EH, ev, EPRM.window_ns, EPRM.min_support, 0, stages[cam])
            pushed = ft.feed_push_events(cam, ev)
            assert (pushed.appended, pushed.rejected) == (int(flags.sum()), rej) and by > 1000, (cam, pushed.appended, pushed.rejected)
        ft.feed_close()
    finally:
        ft.close()
