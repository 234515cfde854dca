"""CPU: the numpy restatement of esvio_fe_convert_events (tests/event_fields_ref.py) against make_events and against
hand-written known answers, and events.EventFields' view of sliced, offset and structured arrays.  The GPU tests
(tests/test_event_fields_gpu.py) hold the kernel against this restatement byte for byte."""
import numpy as np
import pytest

import event_fields_ref as R
from esvio_amd.events import EVENT_DTYPE, EventFields, make_events


def _one(t, unit=1000, off=0, dtype=np.int64, p=1):
    ev, bad = R.convert(np.array([7], np.uint16), np.array([9], np.uint16), np.array([t], dtype), np.array([p], np.int8), unit, off)
    return int(ev["sec"][0]), int(ev["nsec"][0]), int(ev["polarity"][0]), bool(bad[0])


def test_restatement_equals_make_events_on_microseconds():
    rng = np.random.default_rng(3)
    n = 20000
    x, y = rng.integers(0, 1280, n).astype(np.uint16), rng.integers(0, 720, n).astype(np.uint16)
    t = np.sort(rng.integers(0, 4_000_000_000, n)).astype(np.int64) + 1_700_000_000_000_000
    p = rng.integers(0, 2, n).astype(np.uint8)
    want = make_events(x, y, t, p)
    got, bad = R.convert(x, y, t, p, 1000, 0)
    assert not bad.any() and got.tobytes() == want.tobytes()
    # the same stamps as uint32 + a file-wide offset
    got, bad = R.convert(x, y, (t - t[0]).astype(np.uint32), p, 1000, int(t[0]))
    assert not bad.any() and got.tobytes() == want.tobytes()
    # ... and as nanoseconds
    got, bad = R.convert(x, y, t * 1000, p, 1, 0)
    assert not bad.any() and got.tobytes() == want.tobytes()
    assert (got.view(np.uint8).reshape(-1, 16)[:, 13:] == 0).all()


def test_known_answers():
    assert _one(999_999) == (0, 999_999_000, 1, False)
    assert _one(1_000_000) == (1, 0, 1, False)
    assert _one(999_999_999, unit=1) == (0, 999_999_999, 1, False)
    # the last representable tick, and one more
    assert _one((1 << 32) * 10 ** 6 - 1) == ((1 << 32) - 1, 999_999_000, 1, False)
    assert _one((1 << 32) * 10 ** 6)[3]
    assert _one((1 << 32) * 10 ** 9 - 1, unit=1) == ((1 << 32) - 1, 999_999_999, 1, False)
    assert _one((1 << 32) * 10 ** 9, unit=1)[3]
    # t_offset carries a stamp across a second boundary, in both directions
    assert _one(999_999, off=1) == (1, 0, 1, False)
    assert _one(1_000_000, off=-1) == (0, 999_999_000, 1, False)
    assert _one(5, off=1_700_000_000 * 10 ** 6, dtype=np.uint32) == (1_700_000_000, 5000, 1, False)
    assert _one((1 << 32) - 1, off=0, dtype=np.uint32) == (4294, 967_295_000, 1, False)  # unsigned, not -1
    # negative ticks
    assert _one(-1)[3] and _one(0, off=-1)[3] and _one(10, off=-11, dtype=np.uint32)[3]
    assert not _one(0)[3] and not _one(10, off=-10, dtype=np.uint32)[3]
    # 64-bit stamps outside +-2^62 are bad whatever the offset makes of them
    assert _one((1 << 62) + 1, off=-(1 << 62))[3] and not _one(1 << 62, off=-(1 << 62))[3]
    assert _one(-(1 << 62) - 1, off=1 << 62)[3] and _one(1 << 62, off=1 << 62)[3]
    # polarity: signed, > 0
    for p, want in ((-1, 0), (0, 0), (1, 1), (2, 1), (127, 1), (-128, 0)):
        assert _one(5, p=p)[2] == want, p
    ev, _ = R.convert(np.zeros(1, np.uint16), np.zeros(1, np.uint16), np.zeros(1, np.int64), np.array([255], np.uint8))
    assert ev["polarity"][0] == 0  # 255 read as int8 is -1
    ev, _ = R.convert(np.zeros(2, np.uint16), np.zeros(2, np.uint16), np.zeros(2, np.int64), np.array([-1, 1], np.int16))
    assert ev["polarity"].tolist() == [0, 1]
    # x, y are bit patterns
    ev, _ = R.convert(np.array([-2], np.int16), np.array([65535], np.uint16), np.zeros(1, np.int64), np.ones(1, np.int8))
    assert ev["x"][0] == 65534 and ev["y"][0] == 65535


def test_event_fields_strides_of_views():
    n = 40
    x = np.arange(n, dtype=np.uint16)
    y = np.arange(2 * n, dtype=np.uint16)[::2]         # strided
    t = np.arange(n + 3, dtype=np.int64)[3:]           # offset
    p = np.ones((n, 4), np.int8)[:, 1]                 # a column
    f = EventFields.from_arrays(x, y, t, p, t_unit_ns=1, t_offset=-5)
    assert f.n == n and f.strides == (2, 4, 8, 4) and (f.t_bits, f.p_bits, f.t_unit_ns, f.t_offset) == (64, 8, 1, -5)
    assert f.ptrs == (x.ctypes.data, y.ctypes.data, t.ctypes.data, p.ctypes.data)
    assert f.ptrs[2] == t.base.ctypes.data + 24
    assert [s for _, s in f.spans()] == [2 * n, 4 * (n - 1) + 2, 8 * n, 4 * (n - 1) + 1]
    for dt, size in ((R.AOS16, 16), (R.PACKED13, 13)):
        rec = np.zeros(n + 2, dt)[2:]
        f = EventFields.from_structured(rec)
        base = rec.ctypes.data
        assert f.strides == (size,) * 4 and f.t_bits == 64 and f.p_bits == 8 and f.t_unit_ns == 1000
        assert f.ptrs == tuple(base + dt.fields[k][1] for k in ("x", "y", "t", "p"))
        g = EventFields.from_structured(rec[::3])
        assert g.strides == (3 * size,) * 4 and g.n == len(rec[::3]) and g.ptrs == f.ptrs
    named = np.zeros(5, np.dtype([("ts", "<u4"), ("col", "<u2"), ("row", "<u2"), ("pol", "<i2")]))
    f = EventFields.from_structured(named, x="col", y="row", t="ts", p="pol")
    assert f.strides == (10,) * 4 and (f.t_bits, f.p_bits) == (32, 16)
    assert EventFields.from_arrays(x[:1], x[:1], t[:1], p[:1]).strides == (2, 2, 8, 1)
    assert EventFields.from_arrays(x[:0], x[:0], t[:0], p[:0]).n == 0
    for bad in (dict(t=np.zeros(n, np.int32)), dict(t=np.zeros(n, np.uint64)), dict(x=np.zeros(n, np.uint8)),
                dict(p=np.zeros(n, np.int32)), dict(y=np.zeros(n - 1, np.uint16)), dict(x=x[::-1]), dict(t=np.zeros(n, np.float64))):
        kw = dict(x=x, y=x, t=t, p=p)
        kw.update(bad)
        with pytest.raises(ValueError):
            EventFields.from_arrays(**kw)
    with pytest.raises(ValueError):
        EventFields.from_arrays(x, x, t, p, t_unit_ns=10)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_case_generators_describe_what_they_wrote(layout):
    """the generators' fields, read back through their pointers' views, are the logical arrays; the restatement of a
    case does not depend on where the bytes lie"""
    for shift in R.SHIFTS[layout]:
        for n in (0, 1, 9, 257):
            c = R.make_case(layout, n, seed=n + 1, shift=shift, polarity="mixed")
            f = c.fields
            assert f.n == n
            if n == 0:
                continue
            for k, (a, w) in enumerate(zip((c.x, c.y, c.t, c.p), (2, 2, f.t_bits // 8, f.p_bits // 8))):
                o = f.ptrs[k] - c.raw.ctypes.data
                idx = o + f.strides[k] * np.arange(n)[:, None] + np.arange(w)[None, :]
                assert np.array_equal(c.raw[idx].reshape(-1), a.view(np.uint8).reshape(-1)), (layout, shift, n, k)
            if layout == "packed13_i64_us":
                assert {(f.ptrs[2] + 13 * i) % 8 for i in range(min(n, 8))} == (set(range(8)) if n >= 8 else {(f.ptrs[2] + 13 * i) % 8 for i in range(n)})
            ev, bad = R.expected(c)
            assert not bad.any() and ev.dtype == EVENT_DTYPE
            other = np.zeros(len(c.raw) + 16, np.uint8)
            o = (-other.ctypes.data) % 16
            other[o:o + len(c.raw)] = c.raw
            g = c.relocate(other[o:o + len(c.raw)])
            assert g.strides == f.strides and tuple(q - other.ctypes.data - o for q in g.ptrs) == tuple(q - c.raw.ctypes.data for q in f.ptrs)
