"""What the GPU tests of EVT2.1 decoding and of the trigger stage share: a handle whose two decoders per camera — the
event decoder's and the trigger decoder's — are advanced together with the restatement's (tests/evt21_ref.py), every
call compared byte for byte, guard bytes behind every destination."""
import ctypes as C

import numpy as np

import evt21_ref as E
from esvio_amd import frontend as FE
from esvio_amd.events import EVENT_DTYPE

GUARD = 0xA5
FMTS = (E.EVT3, E.EVT2, E.EVT21)
TOP = {E.EVT3: 0xFFF, E.EVT2: 0x0FFFFFFF, E.EVT21: 0x0FFFFFFF}
EVENT = {E.EVT3: 0x2000 | 0x800 | 77, E.EVT2: (1 << 28) | (9 << 22) | (77 << 11) | 33, E.EVT21: E.event_word(1, 9, 77, 33, 0b1001)}
OTHER = {E.EVT3: 0xE000, E.EVT2: 0xE0000000, E.EVT21: 0xE << 60}


def th_word(fmt, v):
    return (0x8000 | v) if fmt == E.EVT3 else (0x80000000 | v) if fmt == E.EVT2 else E.th_word(v)


def tile_words(fmt):
    return FE.load_library().esvio_fe_raw_tile_bytes() // E.word_dtype(fmt).itemsize


def as_words(fmt, w):
    """a list or array of Python / numpy integers -> the stream's words (EVT2.1 words do not fit int64: object route)"""
    return np.array([int(v) for v in w], dtype=np.uint64).astype(E.word_dtype(fmt)) if len(w) else np.zeros(0, E.word_dtype(fmt))


def stream(fmt, n, rng, triggers=True):
    """n words with every type: a time base first, then events, vectors, time words, triggers and others"""
    if n == 0:
        return as_words(fmt, [])
    if fmt == E.EVT21:
        typ = rng.choice([0, 1, 1, 8, 0xA if triggers else 0xE, 0xE], n)
        w = [(int(t) << 60) | int(rng.integers(0, 1 << 28)) << 32 | int(rng.integers(0, 1 << 32)) for t in typ]
        sparse = rng.integers(0, 4, n)
        for k in range(n):
            if typ[k] <= 1 and sparse[k] == 0:
                w[k] &= ~0xFFFFFFFF | (1 << int(rng.integers(0, 32)))  # one bit at the most
            if typ[k] <= 1 and sparse[k] == 1:
                w[k] &= ~0xFFFFFFFF  # a zero mask
        th = np.flatnonzero(typ == 8)
        for j, k in enumerate(th):
            w[k] = E.th_word(1000 + j)
        w[0] = E.th_word(999)
        return as_words(fmt, w)
    if fmt == E.EVT2:
        typ = rng.choice([0, 1, 0, 1, 8, 0xA if triggers else 0xE], n)
        w = (typ.astype(np.int64) << 28) | rng.integers(0, 1 << 28, n)
        th = typ == 8
        w[th] = 0x80000000 | (1000 + np.cumsum(th)[th])
        w[0] = 0x80000000 | 1000
        return w.astype("<u4")
    typ = rng.choice([0x0, 0x2, 0x2, 0x3, 0x4, 0x4, 0x5, 0x6, 0x8, 0xA if triggers else 0xE], n)
    w = (typ.astype(np.int64) << 12) | rng.integers(0, 4096, n)
    th = typ == 0x8
    w[th] = 0x8000 | ((100 + np.cumsum(th)[th]) & 0xFFF)
    w[0] = 0x8000 | 100
    return w.astype("<u2")


class Dec:
    """a handle and the restatement's decoder states of its two cameras, advanced together"""

    def __init__(self):
        self.ft = FE.FeatureTracker(FE.make_config(64, 48, max_cnt=40))
        self.L, self.h = self.ft._hd.L, self.ft._hd.h
        self.hip = C.CDLL("libamdhip64.so")
        self.fresh()

    def fresh(self):
        self.ft.decode_reset()
        self.st = [E.fresh_state(), E.fresh_state()]   # the event decoders
        self.tst = [E.fresh_state(), E.fresh_state()]  # the trigger decoders

    def close(self):
        self.ft.close()

    def _source(self, words, space, skew):
        """-> (pointer, memory space, free()) for the words in host, page-locked or device memory, `skew` bytes behind
        a 16-byte boundary"""
        nbytes = words.nbytes
        if space == "device":
            d = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, nbytes + 32, C.byref(d)) == 0
            src = C.c_void_p(d.value + skew)
            if nbytes:
                assert self.L.esvio_fe_mem_upload(src, C.c_void_p(words.ctypes.data), nbytes) == 0
            return src, FE.DEVICE, lambda: self.L.esvio_fe_mem_free(FE.DEVICE, d)
        if space == "pinned":  # page-locked memory of the library's runtime: read in place by the kernels
            p = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.HOST, nbytes + 32, C.byref(p)) == 0
            np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes + 32,))[skew:skew + nbytes] = words.view(np.uint8)
            return C.c_void_p(p.value + skew), FE.HOST, lambda: self.L.esvio_fe_mem_free(FE.HOST, p)
        return C.c_void_p(words.ctypes.data if nbytes else 0), FE.HOST, lambda: None

    # ---- events ----
    def call(self, fmt, words, cam=0, off=0, space="host", dst_cap=None, dst_space=FE.HOST, skew=0):
        """one esvio_fe_decode_raw call -> (rc, the dst_cap records as bytes, RawInfo); nothing of the restatement moves"""
        words = np.ascontiguousarray(words, E.word_dtype(fmt))
        if dst_cap is None:
            dst_cap = FE.raw_bound(fmt, words.nbytes)
        info = FE.RawInfo(first_t_us=-77, last_t_us=-78)
        back = np.full(16 * (dst_cap + 2), GUARD, np.uint8)
        src, sp, free = self._source(words, space, skew)
        ddst = None
        if dst_space == FE.DEVICE:
            ddst = C.c_void_p()
            assert self.L.esvio_fe_mem_alloc(FE.DEVICE, len(back), C.byref(ddst)) == 0
            assert self.L.esvio_fe_mem_upload(ddst, C.c_void_p(back.ctypes.data), len(back)) == 0
            dst = ddst
        else:
            dst = C.c_void_p(back.ctypes.data)
        rc = self.L.esvio_fe_decode_raw(self.h, cam, fmt, src, words.nbytes, sp, off, dst, dst_cap, dst_space, C.byref(info))
        if ddst is not None:
            assert self.hip.hipMemcpy(C.c_void_p(back.ctypes.data), ddst, C.c_size_t(len(back)), 2) == 0
            self.L.esvio_fe_mem_free(FE.DEVICE, ddst)
        free()
        assert (back[16 * dst_cap:] == GUARD).all(), "bytes beyond dst_cap records touched"
        return rc, back[:16 * dst_cap], info

    def check(self, fmt, words, cam=0, off=0, space="host", dst_space=FE.HOST, tag=None, exact_cap=False, skew=0):
        """a call that succeeds equals the restatement, which advances with it -> (records, info of the restatement)"""
        want, wi = E.decode(fmt, np.asarray(words), self.st[cam], off)
        rc, got, info = self.call(fmt, words, cam, off, space, len(want) if exact_cap else None, dst_space, skew)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        for k in ("events", "untimed", "other", "bad", "wraps"):
            assert getattr(info, k) == wi[k], (tag, k, getattr(info, k), wi[k])
        if len(want):
            assert (info.first_t_us, info.last_t_us) == (wi["first_t_us"], wi["last_t_us"]), tag
        else:
            assert (info.first_t_us, info.last_t_us) == (-77, -78), (tag, "untouched if none")
        n = len(want)
        if got[:16 * n].tobytes() != want.tobytes():
            g = got[:16 * n].view(EVENT_DTYPE)
            i = int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0]) // 16
            raise AssertionError((tag, "first differing record", i, g[i], want[i], n))
        assert (got[16 * n:] == GUARD).all(), (tag, "records beyond the count touched")
        return want, wi

    # ---- triggers ----
    def tcall(self, fmt, words, cam=0, off=0, space="host", dst_cap=None, skew=0):
        """one esvio_fe_decode_triggers call -> (rc, the dst_cap records as bytes, TriggerInfo)"""
        words = np.ascontiguousarray(words, E.word_dtype(fmt))
        if dst_cap is None:
            dst_cap = len(words)
        info = FE.TriggerInfo(first_t_us=-77, last_t_us=-78)
        back = np.full(16 * (dst_cap + 2), GUARD, np.uint8)
        src, sp, free = self._source(words, space, skew)
        rc = self.L.esvio_fe_decode_triggers(self.h, cam, fmt, src, words.nbytes, sp, off, C.c_void_p(back.ctypes.data), dst_cap,
                                             C.byref(info))
        free()
        assert (back[16 * dst_cap:] == GUARD).all(), "bytes beyond dst_cap records touched"
        return rc, back[:16 * dst_cap], info

    def tcheck(self, fmt, words, cam=0, off=0, space="host", tag=None, exact_cap=False, skew=0):
        want, wi = E.decode_triggers(fmt, np.asarray(words), self.tst[cam], off)
        rc, got, info = self.tcall(fmt, words, cam, off, space, len(want) if exact_cap else None, skew)
        assert rc == 0, (tag, rc, self.L.esvio_fe_last_error(self.h))
        for k in ("triggers", "untimed", "bad", "wraps"):
            assert getattr(info, k) == wi[k], (tag, k, getattr(info, k), wi[k])
        if len(want):
            assert (info.first_t_us, info.last_t_us) == (wi["first_t_us"], wi["last_t_us"]), tag
        else:
            assert (info.first_t_us, info.last_t_us) == (-77, -78), (tag, "untouched if none")
        n = len(want)
        if got[:16 * n].tobytes() != want.tobytes():
            g = got[:16 * n].view(E.TRIGGER_DTYPE)
            i = int(np.flatnonzero(g.view(np.uint8).reshape(-1, 16) != want.view(np.uint8).reshape(-1, 16))[0]) // 16
            raise AssertionError((tag, "first differing trigger", i, g[i], want[i], n))
        assert (got[16 * n:] == GUARD).all(), (tag, "records beyond the count touched")
        return want, wi
