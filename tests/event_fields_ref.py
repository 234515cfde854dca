"""numpy restatement of esvio_fe_convert_events' arithmetic (include/esvio_fe.h), independent of the kernel: plain
integer // and % on int64 / Python ints, no multiplies-for-divisions, no vector paths.  Also the case generators the
CPU and GPU tests share: the layouts a recording or an SDK delivers, laid into one raw byte buffer so that a test can
put that buffer into pageable, page-locked, registered or device memory and keep every offset.

    ticks = t + t_offset            t: uint32 (unsigned) or int64 (signed), tps = 10^9 / t_unit_ns
    bad   = ticks < 0, or ticks // tps >= 2^32, or a 64-bit t outside +-2^62
    sec   = ticks // tps,  nsec = (ticks % tps) * t_unit_ns,  polarity = (signed p > 0),  x, y: bit patterns
"""
import numpy as np

from esvio_amd.events import EVENT_DTYPE, EventFields

LIM = 1 << 62


def convert(x, y, t, p, t_unit_ns=1000, t_offset=0):
    """-> (records EVENT_DTYPE, bad bool[n]); the record of a bad event is unspecified (zeros here)"""
    x, y, t, p = (np.asarray(a) for a in (x, y, t, p))
    assert t_unit_ns in (1, 1000) and abs(int(t_offset)) <= LIM
    assert (t.dtype.kind, t.dtype.itemsize) in (("u", 4), ("i", 8)) and p.dtype.itemsize in (1, 2)
    tps = 10 ** 9 // t_unit_ns
    n = len(x)
    ticks = [int(v) + int(t_offset) for v in t.tolist()]  # Python ints: no overflow to reason about
    bad = np.array([tk < 0 or tk // tps >= 1 << 32 for tk in ticks], bool).reshape(n)
    if t.dtype.itemsize == 8:
        bad |= np.array([abs(v) > LIM for v in t.tolist()], bool).reshape(n)
    ev = np.zeros(n, EVENT_DTYPE)
    good = np.flatnonzero(~bad)
    tk = np.array([ticks[i] for i in good], np.uint64).reshape(len(good))
    ev["x"][good] = x.view(np.uint16)[good] if x.dtype.itemsize == 2 else x[good]
    ev["y"][good] = y.view(np.uint16)[good] if y.dtype.itemsize == 2 else y[good]
    ev["sec"][good] = tk // np.uint64(tps)
    ev["nsec"][good] = (tk % np.uint64(tps)) * np.uint64(t_unit_ns)
    signed = p.view(np.int8 if p.dtype.itemsize == 1 else np.int16)
    ev["polarity"][good] = (signed[good] > 0)
    return ev, bad


# ---- layouts -------------------------------------------------------------------------------------------------------
AOS16 = np.dtype({"names": ["t", "x", "y", "p"], "formats": ["<i8", "<u2", "<u2", "i1"], "offsets": [0, 8, 10, 12], "itemsize": 16})
PACKED13 = np.dtype({"names": ["x", "y", "p", "t"], "formats": ["<u2", "<u2", "i1", "<i8"], "offsets": [0, 2, 4, 5], "itemsize": 13})
LAYOUTS = ("soa_u32_us", "soa_i64_ns", "aos16_i64_us", "packed13_i64_us", "soa_p16_us")
# shifts that mean something per layout: separate arrays: every base moved by that many ELEMENTS; the aligned AoS
# record: the base moved by 4 * shift bytes (shift 0: the aligned-record path, else unaligned stamps); the packed
# record: the base residue modulo 8 (the stamp then lies at every residue as i runs)
SHIFTS = {"soa_u32_us": (0, 1, 2, 3), "soa_i64_ns": (0, 1, 2, 3), "aos16_i64_us": (0, 1, 2, 3),
          "packed13_i64_us": (0, 1, 2, 3, 4, 5, 6, 7), "soa_p16_us": (0, 1, 2, 3)}


class Case:
    """one batch in one layout: `raw` (uint8, the only storage), `fields` (EventFields of views into raw), the logical
    arrays x / y / t / p (copies) and the unit / offset — and `spec`, from which relocate() rebuilds the fields over
    another copy of the same bytes"""

    def relocate(self, raw):
        """the same layout over `raw` (same bytes at the same offsets from a base of the same alignment mod 16)"""
        return _fields_over(raw, self.spec, self.n, self.t_unit_ns, self.t_offset)


def raw_bytes(layout, n):
    """upper bound of the buffer a case needs (for arenas)"""
    return 16 * (n + 8) * 2 + 256


def _fields_over(raw, spec, n, unit, off):
    kind = spec[0]
    if kind == "soa":
        _, offs, dts = spec
        arrs = [raw[o:o + n * np.dtype(d).itemsize].view(d) for o, d in zip(offs, dts)]
        return EventFields.from_arrays(*arrs, t_unit_ns=unit, t_offset=off)
    _, o, dt = spec
    rec = raw[o:o + n * dt.itemsize].view(dt)
    return EventFields.from_structured(rec, t_unit_ns=unit, t_offset=off)


def make_case(layout, n, seed, shift=0, alloc=None, polarity="01"):
    """alloc(nbytes) -> a uint8 array whose address is a multiple of 16 (default: pageable numpy memory)"""
    rng = np.random.default_rng(seed)
    c = Case()
    c.layout, c.n, c.shift = layout, n, shift
    x = rng.integers(0, 1 << 16, n).astype(np.uint16)  # (bit patterns: out-of-sensor values included)
    y = rng.integers(0, 1 << 16, n).astype(np.uint16)
    steps = np.cumsum(rng.integers(0, 700_000 if n < 4096 else 60, n)).astype(np.int64)  # crosses second boundaries
    pol = {"01": [0, 1], "pm1": [-1, 1], "mixed": [-1, 0, 1, 2, 127, -128]}[polarity]
    if layout in ("soa_u32_us", "soa_p16_us"):
        t = (steps % (1 << 32)).astype(np.uint32)
        c.t_unit_ns, c.t_offset = 1000, 1_700_000_000_000_000 - 123_456  # a file-wide offset: the recording's epoch
    elif layout == "soa_i64_ns":
        t = steps * 1000 + 1_650_000_000 * 10 ** 9 + rng.integers(0, 1000, n)
        c.t_unit_ns, c.t_offset = 1, -17
    else:
        t = steps + 1_650_000_000 * 10 ** 6
        c.t_unit_ns, c.t_offset = 1000, 999_999
    p = rng.choice(np.array(pol, np.int16 if layout == "soa_p16_us" else np.int8), n)
    if layout == "soa_p16_us":  # (16-bit polarity as SDKs deliver it: -1 / +1)
        p = rng.choice(np.array([-1, 1], np.int16), n)
    if alloc is None:
        def alloc(nbytes):
            buf = np.zeros(nbytes + 16, np.uint8)
            o = (-buf.ctypes.data) % 16
            return buf[o:o + nbytes]
    raw = alloc(raw_bytes(layout, n))
    assert raw.ctypes.data % 16 == 0 or n == 0
    raw[:] = 0xEE
    if layout.startswith("soa"):
        dts = [np.dtype("<u2"), np.dtype("<u2"), t.dtype, p.dtype]
        offs, o = [], 0
        for d in dts:
            o = (o + 15) & ~15
            offs.append(o + shift * d.itemsize)
            o = offs[-1] + n * d.itemsize
        c.spec = ("soa", tuple(offs), tuple(dts))
        for o, d, a in zip(offs, dts, (x, y, t, p)):
            raw[o:o + n * d.itemsize].view(d)[:] = a
    else:
        dt = AOS16 if layout == "aos16_i64_us" else PACKED13
        o = 4 * shift if layout == "aos16_i64_us" else shift
        c.spec = ("aos", o, dt)
        rec = raw[o:o + n * dt.itemsize].view(dt)
        rec["x"], rec["y"], rec["t"], rec["p"] = x, y, t, p
    c.raw = raw
    c.x, c.y, c.t, c.p = x, y, t, p
    c.fields = c.relocate(raw)
    return c


def expected(c):
    return convert(c.x, c.y, c.t, c.p, c.t_unit_ns, c.t_offset)
