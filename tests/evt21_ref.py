"""The EVT2.1 rule and the trigger rule of include/esvio_fe.h (esvio_fe_decode_raw with ESVIO_FE_RAW_EVT21,
esvio_fe_decode_triggers), read sequentially.  Restated from recall of the published format descriptions: unpinned,
like the header's text, which is the specification.  Plain loops, one word at a time; the device chains must equal
them byte for byte.  Also a greedy test-side EVT2.1 encoder (a sensor's encoder is free to choose other words)."""
import numpy as np

import evt_ref as R

EVT2, EVT3, EVT21 = R.EVT2, R.EVT3, 21
BAD_SEC = 1 << 32
TRIGGER_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("id", "u1"), ("value", "u1"), ("_pad", "u1", (6,))])


def fresh_state():
    """the decoder state of a fresh handle — the event decoders' and the trigger decoder's (which reads seen / th /
    wraps / tl only)"""
    return R.fresh_state()


def word_dtype(fmt):
    return np.dtype("<u8") if fmt == EVT21 else R.word_dtype(fmt)


def decode_evt21(words, state, t_offset_us=0):
    """words: uint64 values in stream order; state advanced IN PLACE.  Returns (records, info) as evt_ref's decoders."""
    s = state
    ev, untimed, other = [], 0, 0
    for w in (int(v) for v in words):
        typ = w >> 60
        if typ in (0x0, 0x1):
            bx, y, tlow, mask = (w >> 43) & 0x7FF, (w >> 32) & 0x7FF, (w >> 54) & 0x3F, w & 0xFFFFFFFF
            for i in range(32):
                if (mask >> i) & 1:
                    if s["seen"]:
                        ev.append((bx + i, y, typ, s["wraps"] * (1 << 34) + s["th"] * 64 + tlow))
                    else:
                        untimed += 1
        elif typ == 0x8:
            v = (w >> 32) & 0x0FFFFFFF
            if s["seen"] and v < s["th"] and s["th"] - v >= (1 << 27):
                s["wraps"] += 1
            s["th"], s["seen"] = v, 1
        else:
            other += 1
    return R._result(ev, untimed, other, s, t_offset_us)


def decode(fmt, words, state, t_offset_us=0):
    return decode_evt21(words, state, t_offset_us) if fmt == EVT21 else R.decode(fmt, words, state, t_offset_us)


def decode_triggers(fmt, words, state, t_offset_us=0):
    """the trigger decoder over words of format fmt; state (its own: not the event decoder's) advanced IN PLACE.
    Returns (records, info): TRIGGER_DTYPE records in word order; info = triggers, untimed, bad, wraps, first_t_us,
    last_t_us (ticks; None if no trigger)"""
    s = state
    trig, untimed = [], 0
    for w in (int(v) for v in words):
        if fmt == EVT3:
            typ = w >> 12
            if typ == 0x6:
                s["tl"] = w & 0xFFF
            elif typ == 0x8:
                v = w & 0xFFF
                if s["seen"] and v < s["th"] and s["th"] - v >= 2048:
                    s["wraps"] += 1
                s["th"], s["seen"] = v, 1
            elif typ == 0xA:
                if s["seen"]:
                    trig.append(((w >> 8) & 0xF, w & 1, s["wraps"] * (1 << 24) + s["th"] * 4096 + s["tl"]))
                else:
                    untimed += 1
            continue
        if fmt == EVT2:
            typ, v, tlow, tid, val = w >> 28, w & 0x0FFFFFFF, (w >> 22) & 0x3F, (w >> 8) & 0x1F, w & 1
        else:
            typ, v, tlow, tid, val = w >> 60, (w >> 32) & 0x0FFFFFFF, (w >> 54) & 0x3F, (w >> 40) & 0x1F, (w >> 32) & 1
        if typ == 0x8:
            if s["seen"] and v < s["th"] and s["th"] - v >= (1 << 27):
                s["wraps"] += 1
            s["th"], s["seen"] = v, 1
        elif typ == 0xA:
            if s["seen"]:
                trig.append((tid, val, s["wraps"] * (1 << 34) + s["th"] * 64 + tlow))
            else:
                untimed += 1
    rec = np.zeros(len(trig), TRIGGER_DTYPE)  # (zeros: the padding bytes are 0)
    bad = 0
    for k, (tid, val, t) in enumerate(trig):  # Python integers: nothing overflows
        ticks = t + t_offset_us
        sec, usec = divmod(ticks, 10 ** 6) if ticks >= 0 else (0, 0)
        if ticks < 0 or sec >= BAD_SEC:
            bad += 1
            sec = usec = 0  # (dst is unspecified when there is a BAD trigger)
        rec[k] = (sec, usec * 1000, tid, val, 0)
    info = dict(triggers=len(trig), untimed=untimed, bad=bad, wraps=s["wraps"],
                first_t_us=trig[0][2] + t_offset_us if trig else None, last_t_us=trig[-1][2] + t_offset_us if trig else None)
    return rec, info


# ---- test-side encoder ----------------------------------------------------------------------------------------------
def th_word(v):
    return (0x8 << 60) | ((v & 0x0FFFFFFF) << 32)


def event_word(p, tlow, bx, y, mask):
    return ((p & 1) << 60) | ((tlow & 0x3F) << 54) | ((bx & 0x7FF) << 43) | ((y & 0x7FF) << 32) | (mask & 0xFFFFFFFF)


def trigger_word(fmt, tid, value, tlow=0):
    """an EXT_TRIGGER word of format fmt (EVT3 has no tlow: its time is the state's)"""
    if fmt == EVT3:
        return 0xA000 | ((tid & 0xF) << 8) | (value & 1)
    if fmt == EVT2:
        return (0xA << 28) | ((tlow & 0x3F) << 22) | ((tid & 0x1F) << 8) | (value & 1)
    return (0xA << 60) | ((tlow & 0x3F) << 54) | ((tid & 0x1F) << 40) | ((value & 1) << 32)


def encode_evt21(x, y, p, t_us):
    """greedy: TIME_HIGH when t >> 6 changes; a run with equal (t, y, p) and increasing x inside a 32-pixel window
    becomes one word whose bx is the run's first x (not 32-aligned).  t_us must fit 34 bits; x, y < 2048."""
    x, y, p, t = (np.asarray(a).astype(np.int64) for a in (x, y, p, t_us))
    assert len(t) == 0 or (t.min() >= 0 and t.max() < (1 << 34) and x.max() < 2048 and y.max() < 2048)
    out = []
    th = None
    i, n = 0, len(t)
    while i < n:
        h = int(t[i]) >> 6
        if h != th:
            out.append(th_word(h))
            th = h
        j = i + 1
        while j < n and t[j] == t[i] and y[j] == y[i] and p[j] == p[i] and x[j] > x[j - 1] and x[j] - x[i] < 32:
            j += 1
        mask = 0
        for k in range(i, j):
            mask |= 1 << int(x[k] - x[i])
        out.append(event_word(int(p[i]), int(t[i]) & 0x3F, int(x[i]), int(y[i]), mask))
        i = j
    return np.array(out, dtype="<u8")


def encode(fmt, x, y, p, t_us, vect=True):
    return encode_evt21(x, y, p, t_us) if fmt == EVT21 else R.encode(fmt, x, y, p, t_us, vect)
