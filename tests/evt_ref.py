"""The raw-stream rule of include/esvio_fe.h (esvio_fe_decode_raw), read sequentially: Prophesee EVT3 (16-bit words) and
EVT2 (32-bit words) -> event records.  Restated from recall of the published format descriptions: unpinned, like the
header's text, which is the specification.  Plain loops, one word at a time; the device chain must equal them byte for
byte.  Also the test-side encoders (greedy; a sensor's encoder is free to choose other words for the same events)."""
import numpy as np

from esvio_amd.events import EVENT_DTYPE

EVT2, EVT3 = 2, 3
BAD_SEC = 1 << 32


def fresh_state(fmt=EVT3):
    """the decoder state of a fresh handle (both formats share the dict: EVT2 reads seen / th / wraps only)"""
    return dict(seen=0, th=0, wraps=0, tl=0, y=0, bx=0, bp=0)


def _result(ev, untimed, other, state, t_offset_us):
    """(x, y, p, t) tuples -> (records, info): ticks = t + t_offset_us; BAD when ticks < 0 or sec >= 2^32"""
    rec = np.zeros(len(ev), EVENT_DTYPE)  # (zeros: the padding bytes are 0)
    bad = 0
    secs, nsecs = [], []
    for (x, y, p, t) in ev:  # Python integers: nothing overflows
        ticks = t + t_offset_us
        sec, usec = divmod(ticks, 10 ** 6) if ticks >= 0 else (0, 0)
        if ticks < 0 or sec >= BAD_SEC:
            bad += 1
            sec = usec = 0  # (dst is unspecified when there is a BAD event)
        secs.append(sec)
        nsecs.append(usec * 1000)
    if ev:
        rec["x"] = [e[0] & 0xFFFF for e in ev]
        rec["y"] = [e[1] & 0xFFFF for e in ev]
        rec["polarity"] = [e[2] for e in ev]
        rec["sec"], rec["nsec"] = secs, nsecs
    first = ev[0][3] + t_offset_us if ev else None
    last = ev[-1][3] + t_offset_us if ev else None
    info = dict(events=len(ev), untimed=untimed, other=other, bad=bad, wraps=state["wraps"], first_t_us=first, last_t_us=last)
    return rec, info


def decode_evt3(words, state, t_offset_us=0):
    """words: uint16 values in stream order; state: fresh_state() or what an earlier call left — advanced IN PLACE.
    Returns (records, info).  (A caller that wants the failure rule — state unchanged on BAD / too many events — passes a
    copy and keeps it only on success: the device does the same with its pending slot.)"""
    s = state
    ev, untimed, other = [], 0, 0
    for w in (int(v) for v in words):
        typ = w >> 12
        if typ == 0x0:
            s["y"] = w & 0x7FF
        elif typ == 0x2:
            if s["seen"]:
                ev.append((w & 0x7FF, s["y"], (w >> 11) & 1, s["wraps"] * (1 << 24) + s["th"] * 4096 + s["tl"]))
            else:
                untimed += 1
        elif typ == 0x3:
            s["bx"], s["bp"] = w & 0x7FF, (w >> 11) & 1
        elif typ in (0x4, 0x5):
            nbits = 12 if typ == 0x4 else 8
            for i in range(nbits):
                if (w >> i) & 1:
                    if s["seen"]:
                        ev.append(((s["bx"] + i) & 0xFFFF, s["y"], s["bp"], s["wraps"] * (1 << 24) + s["th"] * 4096 + s["tl"]))
                    else:
                        untimed += 1
            s["bx"] = (s["bx"] + nbits) & 0xFFFF
        elif typ == 0x6:
            s["tl"] = w & 0xFFF
        elif typ == 0x8:
            v = w & 0xFFF
            if s["seen"] and v < s["th"] and s["th"] - v >= 2048:
                s["wraps"] += 1
            s["th"], s["seen"] = v, 1
        else:
            other += 1
    return _result(ev, untimed, other, s, t_offset_us)


def decode_evt2(words, state, t_offset_us=0):
    """words: uint32 values in stream order; as decode_evt3"""
    s = state
    ev, untimed, other = [], 0, 0
    for w in (int(v) for v in words):
        typ = w >> 28
        if typ in (0x0, 0x1):
            if s["seen"]:
                ev.append(((w >> 11) & 0x7FF, w & 0x7FF, typ, s["wraps"] * (1 << 34) + s["th"] * 64 + ((w >> 22) & 0x3F)))
            else:
                untimed += 1
        elif typ == 0x8:
            v = w & 0x0FFFFFFF
            if s["seen"] and v < s["th"] and s["th"] - v >= (1 << 27):
                s["wraps"] += 1
            s["th"], s["seen"] = v, 1
        else:
            other += 1
    return _result(ev, untimed, other, s, t_offset_us)


def decode(fmt, words, state, t_offset_us=0):
    return (decode_evt3 if fmt == EVT3 else decode_evt2)(words, state, t_offset_us)


def word_dtype(fmt):
    return np.dtype("<u2") if fmt == EVT3 else np.dtype("<u4")


# ---- test-side encoders ---------------------------------------------------------------------------------------------
def encode_evt3(x, y, p, t_us, vect=True):
    """greedy: TIME_HIGH, TIME_LOW and ADDR_Y when they change (time first); a run with equal (t, y, p) and increasing x
    inside a 12-pixel window becomes VECT_BASE_X + VECT_12, anything else ADDR_X.  t_us must fit 24 bits (no wrap is
    encoded: the decoder's wrap rule is tested on hand-written words).  x, y < 2048."""
    x, y, p, t = (np.asarray(a).astype(np.int64) for a in (x, y, p, t_us))
    assert len(t) == 0 or (t.min() >= 0 and t.max() < (1 << 24) and x.max() < 2048 and y.max() < 2048)
    out = []
    th = tl = cy = None
    i, n = 0, len(t)
    while i < n:
        h, lo = int(t[i]) >> 12, int(t[i]) & 0xFFF
        if h != th:
            out.append(0x8000 | h)
            th = h
        if lo != tl:
            out.append(0x6000 | lo)
            tl = lo
        if int(y[i]) != cy:
            cy = int(y[i])
            out.append(0x0000 | cy)
        j = i + 1
        if vect:
            while j < n and t[j] == t[i] and y[j] == y[i] and p[j] == p[i] and x[j] > x[j - 1] and x[j] - x[i] < 12:
                j += 1
        if j - i >= 2:
            mask = 0
            for k in range(i, j):
                mask |= 1 << int(x[k] - x[i])
            out.append(0x3000 | (int(p[i]) << 11) | int(x[i]))
            out.append(0x4000 | mask)
        else:
            j = i + 1
            out.append(0x2000 | (int(p[i]) << 11) | int(x[i]))
        i = j
    return np.array(out, dtype="<u2")


def encode_evt2(x, y, p, t_us):
    """TIME_HIGH when t >> 6 changes, then CD_OFF / CD_ON with the low 6 bits.  t_us must fit 34 bits."""
    x, y, p, t = (np.asarray(a).astype(np.int64) for a in (x, y, p, t_us))
    assert len(t) == 0 or (t.min() >= 0 and t.max() < (1 << 34) and x.max() < 2048 and y.max() < 2048)
    out = []
    th = None
    for i in range(len(t)):
        h = int(t[i]) >> 6
        if h != th:
            out.append(0x80000000 | h)
            th = h
        out.append((int(p[i]) << 28) | ((int(t[i]) & 0x3F) << 22) | (int(x[i]) << 11) | int(y[i]))
    return np.array(out, dtype="<u4")


def encode(fmt, x, y, p, t_us, vect=True):
    return encode_evt3(x, y, p, t_us, vect) if fmt == EVT3 else encode_evt2(x, y, p, t_us)


def readout_order(x, y, p, t_us):
    """a sensor's read-out order inside equal stamps: (t, y, p, x) — so that vector words occur.  Returns the index."""
    return np.lexsort((np.asarray(x), np.asarray(p), np.asarray(y), np.asarray(t_us)))
