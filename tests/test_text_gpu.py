"""GPU: text event files on the device (esvio_fe_decode_text, esvio_fe_track_text, esvio_fe_feed_push_text) against
tests/text_ref.py, the sequential reading of include/esvio_fe.h "text event files": the records byte for byte, every
field of the info struct, the state behind every call — after a refusal too."""
import ctypes as C
import os

import numpy as np
import pytest

import text_ref as T
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE, event_times
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu

GUARD = 0xA5
FORMATS = [(o, t) for o in (T.TXYP, T.XYPT) for t in (T.SEC_DECIMAL, T.INT_US, T.INT_NS)]
DAVIS, DVS = (T.TXYP, T.SEC_DECIMAL), (T.XYPT, T.INT_US)
COUNTS = ("events", "lines", "comments", "blank", "malformed", "bad")
RESULTS = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
           "right_pts_velocity")
LIM = FE.text_limits()
TILE = LIM.tile_bytes


class Dec:
    """a handle and the reading's states of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.hip = C.CDLL("libamdhip64.so")
        self.fresh()

    def fresh(self):
        self.ft.decode_reset()
        self.st = [T.fresh(), T.fresh()]

    def close(self):
        self.ft.close()

    def call(self, fmt, data, flags=0, cam=0, off=0, space="host", dst_cap=None, dst_space=FE.HOST, skew=0):
        """one esvio_fe_decode_text call -> (rc, the dst_cap records as bytes, TextInfo); nothing of the reading moves.
        skew: a device or page-locked source that many bytes behind a 16-byte boundary"""
        data = np.frombuffer(bytes(data), np.uint8)
        nbytes = data.nbytes
        if dst_cap is None:
            dst_cap = FE.text_bound(nbytes)
        info = FE.TextInfo(first_malformed=-99, first_t_ns=-77, last_t_ns=-78)
        back = np.full(16 * (dst_cap + 2), GUARD, np.uint8)
        dsrc = ddst = psrc = None
        if space == "device":
            dsrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, nbytes + 32, C.byref(dsrc)) == 0
            src, sp = C.c_void_p(dsrc.value + skew), FE.DEVICE
            assert self.L.esvio_fe_mem_upload(src, C.c_void_p(data.ctypes.data if nbytes else 0), nbytes) == 0
        elif space == "pinned":
            psrc = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.HOST, nbytes + 32, C.byref(psrc)) == 0
            np.ctypeslib.as_array(C.cast(psrc, C.POINTER(C.c_uint8)), shape=(nbytes + 32,))[skew:skew + nbytes] = data
            src, sp = C.c_void_p(psrc.value + skew), FE.HOST
        else:
            src, sp = C.c_void_p(data.ctypes.data if nbytes else 0), FE.HOST
        if dst_space == FE.DEVICE:
            ddst = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, len(back), C.byref(ddst)) == 0
            assert self.L.esvio_fe_mem_upload(ddst, C.c_void_p(back.ctypes.data), len(back)) == 0
            dst = ddst
        else:
            dst = C.c_void_p(back.ctypes.data)
        f = FE.TextFormat(fmt[0], fmt[1], flags, 0)
        rc = self.L.esvio_fe_decode_text(self.h, cam, C.byref(f), src, nbytes, sp, off, dst, dst_cap, dst_space, C.byref(info))
        if ddst is not None:
            assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(len(back)), 2) == 0
            self.L.esvio_fe_mem_free(FE.DEVICE, ddst)
        if dsrc is not None:
            self.L.esvio_fe_mem_free(FE.DEVICE, dsrc)
        if psrc is not None:
            self.L.esvio_fe_mem_free(FE.HOST, psrc)
        assert (back[16 * dst_cap:] == GUARD).all(), "bytes beyond dst_cap records touched"
        return rc, back[:16 * dst_cap], info

    def check(self, fmt, data, flags=0, cam=0, off=0, space="host", dst_cap=None, dst_space=FE.HOST, skew=0, tag=None):
        """a call equals the reading, which advances with it when the call succeeds and stays when it is refused
        -> (records, info, ok of the reading)"""
        cap = FE.text_bound(len(data)) if dst_cap is None else dst_cap
        recs, wi, ok, st = T.read(self.st[cam], fmt[0], fmt[1], flags, data, off, cap)
        rc, got, info = self.call(fmt, data, flags, cam, off, space, cap, dst_space, skew)
        assert rc == (0 if ok else -1), (tag, rc, ok, self.L.esvio_fe_last_error(self.h), wi)
        for k in COUNTS:
            assert getattr(info, k) == wi[k], (tag, k, getattr(info, k), wi[k])
        assert info.first_malformed == (-99 if wi["first_malformed"] is None else wi["first_malformed"]), (tag, info.first_malformed, wi)
        assert info.carried == wi["carried"], (tag, info.carried, wi["carried"])
        if not ok:
            stored = 0 if wi["events"] > cap else wi["events"]
            assert (got[16 * stored:] == GUARD).all(), (tag, "records beyond the count touched by a refused call")
            return recs, wi, ok
        if wi["events"]:
            assert (info.first_t_ns, info.last_t_ns) == (wi["first_t_ns"], wi["last_t_ns"]), tag
        else:
            assert (info.first_t_ns, info.last_t_ns) == (-77, -78), (tag, "untouched if none")
        want = T.records_array(recs)
        n = len(want)
        if got[:16 * n].tobytes() != want.tobytes():
            g = got[:16 * n].view(EVENT_DTYPE)
            i = int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0]) // 16
            raise AssertionError((tag, "first differing record", i, g[i], want[i], n))
        assert (got[16 * n:] == GUARD).all(), (tag, "records beyond the count touched")
        self.st[cam] = st
        return recs, wi, ok


@pytest.fixture(scope="module")
def dec():
    d = Dec()
    yield d
    d.close()


def event_line(fmt, x, y, p, ticks, sep=b" ", minus=False):
    t = {T.SEC_DECIMAL: b"%d.%09d" % (ticks // 10 ** 9, ticks % 10 ** 9), T.INT_US: b"%d" % (ticks // 1000), T.INT_NS: b"%d" % ticks}[fmt[1]]
    pol = b"-1" if (minus and not p) else b"%d" % p
    cols = [t, b"%d" % x, b"%d" % y, pol] if fmt[0] == T.TXYP else [b"%d" % x, b"%d" % y, pol, t]
    return sep.join(cols)


def stream(fmt, n, rng, mixed=True):
    """n event lines; mixed: comments, blank lines, CRLF, comma- and tab-separated lines and "-1" among them"""
    out, ticks = [], int(rng.integers(0, 10 ** 12))
    for _ in range(n):
        ticks += int(rng.integers(0, 50_000_000))
        r = rng.random() if mixed else 1.0
        if r < 0.08:
            out.append(b"# a comment\n" if r < 0.04 else b"%\r\n")
        elif r < 0.14:
            out.append(b"\n" if r < 0.11 else b" \t\r\n")
        sep = b" " if r > 0.5 else b"," if r > 0.3 else b"\t" if r > 0.2 else b" , "
        out.append(event_line(fmt, int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), int(rng.integers(0, 2)), ticks, sep, r < 0.7) +
                   (b"\r\n" if mixed and rng.random() < 0.3 else b"\n"))
    return b"".join(out)


def fill(k):
    """exactly k bytes of comment and blank lines"""
    out = b""
    while len(out) < k:
        r = min(k - len(out), 60)
        out += b"\n" if r == 1 else b"#" + b"x" * (r - 2) + b"\n"
    return out


def exact(fmt, nbytes, rng):
    """a mixed stream of exactly nbytes bytes that ends with a terminator"""
    out = b""
    while nbytes - len(out) >= 200:
        out += stream(fmt, 1, rng)
    return out + fill(nbytes - len(out))


# ---- 1. line counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_line_counts_around_the_wave_and_the_tile(dec, fmt):
    rng = np.random.default_rng(10 * fmt[0] + fmt[1])
    for n in (0, 1, 63, 64, 65):
        dec.fresh()
        recs, wi, ok = dec.check(fmt, stream(fmt, n, rng), T.END, tag=(fmt, n))
        assert ok and wi["events"] == n
    for nbytes in (TILE - 1, TILE, TILE + 1):
        dec.fresh()
        recs, wi, ok = dec.check(fmt, exact(fmt, nbytes, rng), tag=(fmt, "bytes", nbytes))
        assert ok and wi["events"] > 50 and wi["comments"] and wi["blank"] and wi["carried"] == 0
    dec.fresh()
    recs, wi, ok = dec.check(fmt, exact(fmt, 3 * TILE, rng) + stream(fmt, 1, rng, mixed=False), tag=(fmt, "3 tiles + a line"))
    assert ok and wi["events"] > 200


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------
def test_every_line_slides_across_the_first_tile_edge(dec):
    rng = np.random.default_rng(2)
    body = exact(DAVIS, TILE - 200, rng) + stream(DAVIS, 12, rng)  # lines on both sides of byte TILE
    for k in range(0, 71):
        dec.fresh()
        recs, wi, ok = dec.check(DAVIS, fill(k) + body, tag=("slide", k))
        assert ok


def test_terminators_and_long_bodies_at_the_tile_edge(dec):
    rng = np.random.default_rng(3)
    more = stream(DAVIS, 5, rng)
    body64 = event_line(DAVIS, 1, 2, 1, 3 * 10 ** 9).ljust(64, b" ")
    cases = {
        "newline last byte of the tile": exact(DAVIS, TILE, rng) + more,
        "newline first byte of the next tile": exact(DAVIS, TILE + 1, rng) + more,
        "64-byte body from the tile's last byte": exact(DAVIS, TILE - 1, rng) + body64 + b"\r\n" + more,
        "64-byte body from the next tile's first byte": exact(DAVIS, TILE, rng) + body64 + b"\n" + more,
        "65-byte body from the tile's last byte": exact(DAVIS, TILE - 1, rng) + body64 + b" \n" + more,
    }
    for tag, data in cases.items():
        dec.fresh()
        recs, wi, ok = dec.check(DAVIS, data, T.SKIP_MALFORMED, tag=tag)
        assert ok and wi["malformed"] == (1 if tag.startswith("65") else 0), tag
    # a tile that holds no line start: overlong lines, 2.5 tiles each
    data = more + b"x" * (5 * TILE // 2) + b"\n" + more + b"y" * (5 * TILE // 2) + b"\r\n" + more
    for flags, good in ((T.SKIP_MALFORMED, True), (0, False)):
        dec.fresh()
        recs, wi, ok = dec.check(DAVIS, data, flags, tag=("no line start", flags))
        assert ok == good and wi["malformed"] == 2 and wi["events"] == 15 and wi["first_malformed"] == len(more)
    # ... and one no '\n' follows: it is no line of this call, the call after it ends it
    dec.fresh()
    recs, wi, ok = dec.check(DAVIS, more + b"x" * (5 * TILE // 2), tag="overlong, unterminated")
    assert ok and wi["malformed"] == 0 and wi["carried"] == 0 and dec.st[0]["skip"]
    recs, wi, ok = dec.check(DAVIS, b"x" * TILE, tag="overlong, goes on")
    assert ok and wi["lines"] == 0
    recs, wi, ok = dec.check(DAVIS, b"xx\n" + more, T.SKIP_MALFORMED, tag="overlong, ends")
    assert ok and wi["malformed"] == 1 and wi["first_malformed"] == -(5 * TILE // 2 + TILE) and wi["events"] == 5


# ---- 3. chunking ---------------------------------------------------------------------------------------------------------
CHUNKED = (b"# t x y p\r\n1.5 3 4 1\n\n , \r\n2.25,5,6,0\r\n" + b"7" * 97 + b"\n3.000000001\t65535\t0\t-1\nbad line\n4294967295.999999999 1 1 1\n" +
           b"5 1 1 1" + b" " * 57 + b"\r\n" + b"9" * 64 + b"\n6 2 2 0")


def whole_stream(dec):
    dec.fresh()
    recs, wi, ok = dec.check(DAVIS, CHUNKED, T.END | T.SKIP_MALFORMED, tag="whole")
    assert ok and (wi["events"], wi["comments"], wi["blank"], wi["malformed"]) == (6, 1, 2, 3)
    return recs, wi


@pytest.mark.parametrize("space", ["host", "device"])
def test_a_stream_cut_in_two_at_every_byte(dec, space):
    recs, wi = whole_stream(dec)
    for cut in range(len(CHUNKED) + 1):
        dec.fresh()
        a = dec.check(DAVIS, CHUNKED[:cut], T.SKIP_MALFORMED, space=space, tag=("cut", cut, "first"))
        b = dec.check(DAVIS, CHUNKED[cut:], T.END | T.SKIP_MALFORMED, space=space, tag=("cut", cut, "second"))
        assert a[2] and b[2] and a[0] + b[0] == recs, cut
        assert all(a[1][k] + b[1][k] == wi[k] for k in COUNTS), cut


def test_a_stream_one_byte_per_call_and_a_reset_in_the_middle(dec):
    recs, wi = whole_stream(dec)
    dec.fresh()
    got, sums = [], dict.fromkeys(COUNTS, 0)
    for i in range(len(CHUNKED) + 1):
        r, w, ok = dec.check(DAVIS, CHUNKED[i:i + 1], T.SKIP_MALFORMED | (T.END if i == len(CHUNKED) else 0), tag=("byte", i))
        assert ok
        got += r
        for k in COUNTS:
            sums[k] += w[k]
    assert got == recs and all(sums[k] == wi[k] for k in COUNTS)
    # esvio_fe_decode_reset drops the tail
    dec.fresh()
    r, w, ok = dec.check(DAVIS, b"1.5 3 4 1\n2.5 3 4", tag="a tail")
    assert ok and w["carried"] == 7
    dec.fresh()
    r, w, ok = dec.check(DAVIS, b" 1\n", T.SKIP_MALFORMED, tag="behind the reset")
    assert ok and w["events"] == 0 and w["malformed"] == 1


# ---- 4. malformed causes ---------------------------------------------------------------------------------------------------
MALFORMED = {
    "65-byte body": (DAVIS, b"2.5 1 1 1" + b" " * 56, b"2.5 1 1 1" + b" " * 55),
    "three tokens": (DAVIS, b"2.5 1 1", b"2.5 1 1 1"),
    "five tokens": (DAVIS, b"2.5 1 1 1 1", b"2.5 1 1 1"),
    "65536": (DAVIS, b"2.5 65536 1 1", b"2.5 65535 1 1"),
    "six digits": (DAVIS, b"2.5 1 000001 1", b"2.5 1 00001 1"),
    "p = 2": (DAVIS, b"2.5 1 1 2", b"2.5 1 1 1"),
    "p = +1": (DAVIS, b"2.5 1 1 +1", b"2.5 1 1 1"),
    "p = -0": (DAVIS, b"2.5 1 1 -0", b"2.5 1 1 0"),
    "1e5": (DAVIS, b"1e5 1 1 1", b"100000 1 1 1"),
    ".5": (DAVIS, b".5 1 1 1", b"0.5 1 1 1"),
    "5.": (DAVIS, b"5. 1 1 1", b"5.0 1 1 1"),
    "11-digit integer part": (DAVIS, b"12345678901.5 1 1 1", b"1234567890.5 1 1 1"),
    "20-digit integer": (DVS, b"1 1 1 00000000000000000025", b"1 1 1 0000000000000000025"),
    "a NUL byte": (DAVIS, b"2.5 1\x00 1 1", b"2.5 10 1 1"),
    "a letter": (DAVIS, b"2.5 1a 1 1", b"2.5 10 1 1"),
}


@pytest.mark.parametrize("cause", sorted(MALFORMED))
def test_a_malformed_line_in_the_second_of_three_lines(dec, cause):
    fmt, bad, good = MALFORMED[cause]
    first, third = event_line(fmt, 7, 8, 1, 10 ** 9) + b"\n", event_line(fmt, 9, 10, 0, 3 * 10 ** 9) + b"\r\n"
    dec.fresh()
    recs, wi, ok = dec.check(fmt, first + bad + b"\n" + third, tag=cause)
    assert not ok and wi["malformed"] == 1 and wi["first_malformed"] == len(first) and wi["events"] == 2
    recs, wi, ok = dec.check(fmt, first + bad + b"\n" + third, T.SKIP_MALFORMED, dst_space=FE.DEVICE, tag=(cause, "skipped"))
    assert ok and wi["malformed"] == 1 and len(recs) == 2 and wi["first_malformed"] == len(first)
    # the line begins in the tail: a negative offset; the state is as before, the repaired bytes decode normally
    dec.fresh()
    k = min(3, len(os.path.commonprefix([bad, good])))
    if k == 0:  # (a leading separator is stripped: it changes no class)
        bad, good, k = b" " + bad, b" " + good, 1
    recs, wi, ok = dec.check(fmt, first + bad[:k], tag=(cause, "head"))
    assert ok and wi["carried"] == k
    recs, wi, ok = dec.check(fmt, bad[k:] + b"\n" + third, tag=(cause, "rest"))
    assert not ok and wi["first_malformed"] == -k and wi["carried"] == k
    recs, wi, ok = dec.check(fmt, good[k:] + b"\n" + third, tag=(cause, "repaired"))
    assert ok and wi["events"] == 2 and wi["malformed"] == 0


# ---- 5. BAD causes ---------------------------------------------------------------------------------------------------------
BAD = {
    "4294967296.0": (DAVIS, b"4294967296.0 1 1 1", 0),
    "pushed below zero": (DAVIS, b"1.0 1 1 1", -2 * 10 ** 9),
    "pushed beyond 2^32 s": (DAVIS, b"1.0 1 1 1", 1 << 62),
    "19-digit INT_US": (DVS, b"1 1 1 9999999999999999999", 0),
    "19-digit INT_US pulled back": (DVS, b"1 1 1 9999999999999999999", -(1 << 62)),
    "ticks == -1": (DAVIS, b"0.000000001 1 1 1", -2),
}


@pytest.mark.parametrize("cause", sorted(BAD))
def test_a_bad_stamp_counts_exactly_and_leaves_the_state(dec, cause):
    fmt, bad, off = BAD[cause]
    # a line that is good under this offset (none is under +2^62: ticks >= 2^62 > 2^32 s)
    good = b"" if off > 0 else event_line(fmt, 3, 4, 1, ((5 * 10 ** 9 - off) // 1000 + 1) * 1000) + b"\n"
    dec.fresh()
    recs, wi, ok = dec.check(fmt, good + b"7 7", off=off, tag=(cause, "a tail first"))
    assert ok and wi["carried"] == 3 and wi["events"] == (1 if good else 0)
    recs, wi, ok = dec.check(fmt, b"\n" + good + bad + b"\n" + good, T.SKIP_MALFORMED, off=off, tag=cause)
    assert not ok and wi["bad"] == 1 and wi["events"] == (3 if good else 1) and wi["malformed"] == 1 and wi["carried"] == 3
    recs, wi, ok = dec.check(fmt, bad + b"\n", off=off, dst_space=FE.DEVICE, tag=(cause, "alone, behind the tail"))
    assert not ok and wi["malformed"] == 1 and wi["first_malformed"] == -3  # ("7 7" + the line: no event line)
    recs, wi, ok = dec.check(fmt, b"\n" + good, T.SKIP_MALFORMED, off=off, tag=(cause, "the state is as it was"))
    assert ok and wi["malformed"] == 1 and wi["first_malformed"] == -3 and wi["events"] == (1 if good else 0)


def test_the_largest_good_stamp_passes(dec):
    dec.fresh()
    recs, wi, ok = dec.check(DAVIS, b"4294967295.999999999 1 1 1\n")
    assert ok and recs == [(1, 1, 4294967295, 999999999, 1)]
    recs, wi, ok = dec.check(DVS, b"1 1 1 4294967295999999\n1 1 0 0\n")
    assert ok and recs[0] == (1, 1, 4294967295, 999999000, 1)
    recs, wi, ok = dec.check((T.XYPT, T.INT_NS), b"1 1 1 4611686018427387904\n", off=-(1 << 62))
    assert ok and recs == [(1, 1, 0, 0, 1)]


# ---- 6. edge values ----------------------------------------------------------------------------------------------------------
def test_edge_values(dec):
    dec.fresh()
    data = (b"1.5 65535 65535 1\n" b"0000000002.5 007 00007 0\n" b"3.1 1 2 -1\n" b"3.123456789 1 2 1\n" b"3.1234567891 1 2 1\n"
            b"3.999999999999 1 2 1\n" b"4\t1\t2\t1\n" b"5 1 2 1 \t ,\r\n" b",,6,1,2,0,,\n" b"7 1 2 1")
    recs, wi, ok = dec.check(DAVIS, data, tag="edge values")
    assert ok and wi["events"] == 9 and wi["carried"] == 7
    assert recs[:6] == [(65535, 65535, 1, 500000000, 1), (7, 7, 2, 500000000, 0), (1, 2, 3, 100000000, 0), (1, 2, 3, 123456789, 1),
                        (1, 2, 3, 123456789, 1), (1, 2, 3, 999999999, 1)]
    # an END call with no bytes and a carried tail
    recs, wi, ok = dec.check(DAVIS, b"", T.END, tag="END, no bytes, a tail")
    assert ok and recs == [(1, 2, 7, 0, 1)] and wi["lines"] == 1 and wi["carried"] == 0
    recs, wi, ok = dec.check(DAVIS, b"", T.END, tag="END, no bytes, no tail")
    assert ok and wi["lines"] == 0
    recs, wi, ok = dec.check(DAVIS, b"", 0, tag="no bytes")
    assert ok and wi["lines"] == 0


# ---- 7. dst_cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_space", [FE.HOST, FE.DEVICE])
def test_dst_cap_exactly_enough_and_one_short(dec, dst_space):
    rng = np.random.default_rng(7)
    data = exact(DVS, TILE + 300, rng)
    dec.fresh()
    recs, wi, ok = dec.check(DVS, b"# ", tag="a tail")  # (it makes a comment of the chunk's first line)
    n = T.read(dec.st[0], DVS[0], DVS[1], 0, data)[1]["events"]
    assert n > 100
    recs, wi, ok = dec.check(DVS, data, dst_cap=n - 1, dst_space=dst_space, tag="one short")
    assert not ok and wi["events"] == n and wi["carried"] == 2
    recs, wi, ok = dec.check(DVS, data, dst_cap=n, dst_space=dst_space, tag="exactly enough")
    assert ok and wi["events"] == n and wi["malformed"] == 0 and wi["carried"] == 0


# ---- 8. source spaces ------------------------------------------------------------------------------------------------------------
def test_device_sources_at_every_alignment(dec):
    rng = np.random.default_rng(8)
    data = exact(DAVIS, TILE + 300, rng) + b"9.5 1 2"
    for skew in range(16):
        dec.fresh()
        dec.check(DAVIS, b"# a tail of %2d\r" % skew + b"x" * (skew * 3), space="device", skew=(skew * 7) % 16, tag=("tail", skew))
        recs, wi, ok = dec.check(DAVIS, b"\n" + data, space="device", skew=skew, dst_space=FE.DEVICE if skew % 2 else FE.HOST, tag=("skew", skew))
        assert ok and wi["carried"] == 7 and wi["comments"] >= 1


def test_page_locked_sources_below_and_above_the_in_place_limit_and_pageable_ones(dec):
    rng = np.random.default_rng(9)
    small = exact(DVS, 3 * TILE + 17, rng)
    big = stream(DVS, 12000, rng)
    assert len(big) > (256 << 10) + 4096
    for space, data, skew in (("pinned", small, 0), ("pinned", small, 3), ("pinned", big, 0), ("pinned", big, 5), ("host", big, 0)):
        dec.fresh()
        recs, wi, ok = dec.check(DVS, data, space=space, skew=skew, tag=(space, len(data), skew))
        assert ok and wi["events"] > 100


# ---- 9. round trip -----------------------------------------------------------------------------------------------------------------
W, H = 64, 48


@pytest.fixture(scope="module")
def frames():
    """4 frames of the bench scene stream at a small sensor size: per frame and camera the records as an array and as tuples"""
    st = SceneStream(W=W, H=H, rate=2e5, seed=7, n_rect=8, size=(12.0, 30.0), speed=(40.0, 110.0), disparity=4)
    out = []
    for _ in range(4):
        left, right, _ = st.next_batch()
        out.append([(ev, [(int(e["x"]), int(e["y"]), int(e["sec"]), int(e["nsec"]), int(e["polarity"] != 0)) for e in ev]) for ev in (left, right)])
    assert 2000 < len(out[0][0][0]) < 25000
    return out


def test_round_trip_through_the_cited_writers(dec, frames):
    ev, tup = frames[0][0]
    floored = [(x, y, s, ns // 1000 * 1000, p) for x, y, s, ns, p in tup]
    for write, fmt, want in ((T.write_davis, DAVIS, tup), (T.write_dvs, DVS, floored), (T.write_cpp, DVS, floored), (T.write_csv, DVS, floored)):
        dec.fresh()
        recs, wi, ok = dec.check(fmt, write(tup), tag=write.__name__)
        assert ok and recs == want and wi["events"] == wi["lines"] == len(tup)
    rec, info = dec.ft.decode_text(0, T.TXYP, T.SEC_DECIMAL, T.write_davis(tup))
    assert rec.tobytes() == T.records_array(tup).tobytes()
    assert all(np.array_equal(rec[k], ev[k]) for k in ("x", "y", "sec", "nsec")) and np.array_equal(rec["polarity"], ev["polarity"] != 0)


# ---- 10. esvio_fe_track_text ---------------------------------------------------------------------------------------------------------
def results(ft):
    return {k: np.array(getattr(ft, k)).tobytes() for k in RESULTS}


def make_tracker(max_cnt=40):
    return FE.FeatureTracker(FE.make_config(W, H, max_cnt=max_cnt))


@pytest.mark.parametrize("filtered", [False, True])
def test_track_text_equals_track_event_on_the_readings_records(frames, filtered):
    a, b = make_tracker(), make_tracker()
    prm = FE.FilterParams(5_000_000, 1, 200_000) if filtered else None
    try:
        for i, fr in enumerate(frames[:3]):
            texts = [b"# frame %d\n" % i + T.write_davis(fr[c][1]) for c in range(2)]
            recs = [T.records_array(T.read(T.fresh(), T.TXYP, T.SEC_DECIMAL, 0, t)[0]) for t in texts]
            pub = i != 1
            if filtered:
                ia = a.track_batch(recs[0], recs[1], pub=pub, params=prm)
            else:
                a.trackEvent(float(event_times(recs[0][-1:])[0]), recs[0], recs[1], pub)
            ib, text = b.track_text(T.TXYP, T.SEC_DECIMAL, texts[0], texts[1], pub=pub, params=prm)
            assert ib.tracked == 1 and ib.cur_time == float(event_times(recs[0][-1:])[0]) or filtered
            if filtered:
                assert (ia.kept[0], ia.kept[1], ia.rejected[0], ia.cur_time, ia.tracked) == (ib.kept[0], ib.kept[1], ib.rejected[0], ib.cur_time, ib.tracked)
                assert 0 < ib.kept[0] < text[0].events
            else:
                assert (ib.kept[0], ib.kept[1]) == (len(recs[0]), len(recs[1]))
            for c in range(2):
                assert (text[c].events, text[c].comments, text[c].lines, text[c].carried) == (len(recs[c]), 1, len(recs[c]) + 1, 0)
            assert results(a) == results(b), i
        assert len(a.ids) > 0 and len(a.ids_right) > 0
    finally:
        a.close()
        b.close()


def test_track_text_refusals_move_no_state(frames):
    ft = make_tracker(40)
    try:
        left, right = (T.write_dvs(frames[0][c][1][:600]) for c in range(2))
        n = 600
        # a tail in both cameras first: a state that moved would show
        ft.decode_text(0, T.XYPT, T.INT_US, b"# le")
        ft.decode_text(1, T.XYPT, T.INT_US, b"# ri")
        with pytest.raises(FE.FrontendError, match="both cameras' text states are as they were") as e:
            ft.track_text(T.XYPT, T.INT_US, b"ft\n" + left, b"ght\n" + right + b"1 1 1 9999999999999999999\n")
        assert (e.value.info.bad[0], e.value.info.bad[1], e.value.info.tracked) == (0, 1, 0) and len(ft.ids) == 0
        assert (e.value.text[0].events, e.value.text[1].events, e.value.text[1].bad, e.value.text[1].comments) == (n, n + 1, 1, 1)
        with pytest.raises(FE.FrontendError, match="malformed") as e:
            ft.track_text(T.XYPT, T.INT_US, b"ft\n" + left, b"ght\n" + right + b"oops\n")
        assert e.value.text[1].malformed == 1 and e.value.text[1].first_malformed == len(b"ght\n" + right) and e.value.info.tracked == 0
        ev = T.records_array(frames[0][0][1][:600])
        dl = FE.EventBuffer(ev, FE.DEVICE)
        ft.set_next_batch(float(event_times(ev[-1:])[0]), dl.arg, dl.arg, True)
        with pytest.raises(FE.FrontendError, match="announced"):
            ft.track_text(T.XYPT, T.INT_US, left, right)
        ft.trackEvent(float(event_times(ev[-1:])[0]), dl.arg, dl.arg, True)
        dl.free()
        info, text = ft.track_text(T.XYPT, T.INT_US, b"ft\n" + left, b"ght\n" + right + b"oops\n", flags=T.SKIP_MALFORMED)
        assert info.tracked == 1 and (info.kept[0], info.kept[1]) == (n, n)
        assert [(t.events, t.comments, t.malformed, t.carried) for t in text] == [(n, 1, 0, 0), (n, 1, 1, 0)]
    finally:
        ft.close()


# ---- 11. esvio_fe_feed_push_text -------------------------------------------------------------------------------------------------------
def test_a_feed_fed_4099_byte_chunks_equals_the_feed_fed_the_readings_records(frames):
    a, b = make_tracker(40), make_tracker(40)
    try:
        a.feed_open(200.0)
        b.feed_open(200.0)
        tracked = 0
        st = [T.fresh(), T.fresh()]
        for fr in frames[:3]:
            for cam in range(2):
                data = T.write_davis(fr[cam][1])
                for lo in range(0, len(data), 4099):
                    recs, wi, ok, st[cam] = T.read(st[cam], T.TXYP, T.SEC_DECIMAL, 0, data[lo:lo + 4099])
                    ia = a.feed_push_text(cam, T.TXYP, T.SEC_DECIMAL, data[lo:lo + 4099])
                    ib = b.feed_push_events(cam, T.records_array(recs))
                    assert ok and (ia.appended, ia.closed, ia.queued, ia.bad) == (ib.appended, ib.closed, ib.queued, 0) and ia.appended == len(recs)
                    while True:
                        wa, wb = a.feed_peek(), b.feed_peek()
                        assert (wa is None) == (wb is None)
                        if wa is None:
                            break
                        assert (wa.index, wa.end_sec, wa.end_nsec, wa.count[0], wa.count[1]) == (wb.index, wb.end_sec, wb.end_nsec, wb.count[0], wb.count[1])
                        ja, jb = a.feed_track(tracked % 3 != 1), b.feed_track(tracked % 3 != 1)
                        assert (ja.tracked, ja.cur_time, ja.kept[0], ja.kept[1]) == (jb.tracked, jb.cur_time, jb.kept[0], jb.kept[1])
                        if ja.tracked:
                            assert results(a) == results(b), tracked
                        tracked += 1
        assert tracked >= 5 and len(a.ids) > 0
    finally:
        a.close()
        b.close()


def test_feed_push_text_with_a_bad_line_appends_nothing_and_leaves_the_state(frames):
    good = T.write_dvs(frames[0][0][1][:500])
    for filtered in (False, True):
        ft = make_tracker(40)
        try:
            ft.feed_open(1000.0, params=FE.FilterParams(1_000_000, 0) if filtered else None)
            info = ft.feed_push_text(0, T.XYPT, T.INT_US, b"# a ta")
            assert (info.appended, info.bad) == (0, 0)
            with pytest.raises(FE.FrontendError, match="nothing was appended, the camera's state is as it was") as e:
                ft.feed_push_text(0, T.XYPT, T.INT_US, b"il\n" + good + b"1 1 1 9999999999999999999\n")
            assert (e.value.info.appended, e.value.info.bad, e.value.info.closed) == (0, 1, 0)
            with pytest.raises(FE.FrontendError, match="malformed"):
                ft.feed_push_text(0, T.XYPT, T.INT_US, b"il\n" + good + b"oops\n")
            # the tail still waits: a state that had moved would read "il" as a malformed line
            info = ft.feed_push_text(0, T.XYPT, T.INT_US, b"il\n" + good)
            assert (info.appended + info.rejected, info.bad) == (500, 0)
        finally:
            ft.close()
