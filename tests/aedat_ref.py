"""The sequential reading of the libcaer / AEDAT 3.1 rule in include/esvio_fe.h, written from that text alone: plain
loops over Python integers, one byte string in, records out — and a packet writer for the tests.  Not part of the library.

A Walker is one walker state of the rule (a handle has two per camera): feed() takes a chunk that may end anywhere and
returns what the chunk completes."""
import struct

import numpy as np

from esvio_amd.events import EVENT_DTYPE

SPECIAL, POLARITY, IMU6, FRAME = 0, 1, 3, 2
KEEP_INVALID = 1
HEADER = struct.Struct("<hhiiiiii")  # eventType, eventSource, eventSize, eventTSOffset, eventTSOverflow, eventCapacity, eventNumber, eventValid
SIZES = {SPECIAL: 8, POLARITY: 8, IMU6: 36}
IMU_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("acc", "<f8", (3,)), ("gyr", "<f8", (3,))])
TRIGGER_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("id", "u1"), ("value", "u1"), ("_pad", "u1", (6,))])


class Malformed(ValueError):
    pass


class Bad(ValueError):
    """a BAD stamp failed the call; .bad is the exact count"""

    def __init__(self, bad):
        super().__init__("%d BAD" % bad)
        self.bad = bad


# ---- the writer --------------------------------------------------------------------------------------------------------
def packet(etype, events, overflow=0, capacity=None, size=None, ts_offset=4, number=None, valid=0, source=1):
    """one packet: the header and the payload; `events` a list of byte strings of one size (padding is 0xEE bytes)"""
    size = (SIZES.get(etype, len(events[0]) if events else 8)) if size is None else size
    number = len(events) if number is None else number
    capacity = number if capacity is None else capacity
    body = b"".join(events)
    pad = max(capacity * size - len(body), 0) if size > 0 and capacity > 0 else 0
    return HEADER.pack(etype, source, size, ts_offset, overflow, capacity, number, valid) + body + b"\xee" * pad


def polarity(x, y, p, ts, valid=1):
    return struct.pack("<Ii", (valid & 1) | (p & 1) << 1 | (y & 0x7FFF) << 2 | (x & 0x7FFF) << 17, ts)


def special(stype, ts, valid=1):
    return struct.pack("<Ii", (valid & 1) | (stype & 0x7F) << 1, ts)


def imu6(ts, acc, gyr, temp=25.0, valid=1):
    return struct.pack("<Ii7f", valid & 1, ts, *acc, *gyr, temp)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def stamp(ts, overflow, t_offset_ns):
    """(sec, nsec, ticks_ns) or None for a BAD stamp: exact integers"""
    if ts < 0 or overflow < 0:
        return None
    ts64 = (overflow << 31) | (ts & 0xFFFFFFFF)
    ticks = ts64 * 1000 + t_offset_ns
    if ticks < 0 or ticks // 10 ** 9 >= 2 ** 32:
        return None
    return ticks // 10 ** 9, ticks % 10 ** 9, ticks


def check_header(etype, size, ts_offset, capacity, number):
    if size <= 0 or capacity < 0 or number < 0 or number > capacity:
        raise Malformed("counts")
    if etype in SIZES and (size != SIZES[etype] or ts_offset != 4):
        raise Malformed("size / TSOffset of a known type")


class Walker:
    """mode "events": decodes type 1; mode "side": decodes types 0 and 3"""

    def __init__(self, mode):
        self.mode = mode
        self.hdr = b""          # header bytes collected so far
        self.etype = self.size = self.overflow = 0
        self.events_left = 0    # records of a decoded packet still to come
        self.payload_left = 0   # payload bytes still to come
        self.rec = b""          # the bytes of a record cut by the chunk's end

    def copy(self):
        w = Walker(self.mode)
        w.__dict__.update(self.__dict__)
        return w

    def feed(self, chunk, t_offset_ns=0, flags=0):
        """the chunk through a COPY of the state; returns (state after, result dict).  Raises Malformed / Bad: the
        caller's state is then as it was."""
        w = self.copy()
        out = {"events": [], "imu": [], "triggers": [], "invalid": 0, "bad": 0, "resets": 0, "other_specials": 0,
               "polarity_packets": 0, "special_packets": 0, "imu_packets": 0, "other_packets": 0, "ticks": [],
               "records": []}  # records: the raw polarity records in order with their overflow (the walk's own output)
        pos, n = 0, len(chunk)
        while pos < n:
            if w.payload_left == 0:
                take = min(28 - len(w.hdr), n - pos)
                w.hdr += chunk[pos:pos + take]
                pos += take
                if len(w.hdr) < 28:
                    break
                etype, _, size, ts_offset, overflow, capacity, number, _ = HEADER.unpack(w.hdr)
                check_header(etype, size, ts_offset, capacity, number)
                w.hdr = b""
                w.etype, w.size, w.overflow = etype, size, overflow
                decoded = etype == POLARITY if w.mode == "events" else etype in (SPECIAL, IMU6)
                w.events_left = number if decoded else 0
                w.payload_left = capacity * size
                key = {POLARITY: "polarity_packets", SPECIAL: "special_packets", IMU6: "imu_packets"}.get(etype, "other_packets")
                out[key] += 1
            elif w.events_left:
                take = min(w.size - len(w.rec), n - pos)
                w.rec += chunk[pos:pos + take]
                pos += take
                w.payload_left -= take
                if len(w.rec) < w.size:
                    break
                w._record(w.rec, t_offset_ns, flags, out)
                w.rec = b""
                w.events_left -= 1
            else:
                skip = min(w.payload_left, n - pos)
                pos += skip
                w.payload_left -= skip
        if out["bad"]:
            raise Bad(out["bad"])
        return w, out

    def _record(self, rec, t_offset_ns, flags, out):
        data, ts = struct.unpack_from("<Ii", rec)
        if self.etype == POLARITY:
            out["records"].append((rec, self.overflow))
        if not (data & 1) and not (flags & KEEP_INVALID):
            out["invalid"] += 1
            return
        if self.etype == SPECIAL:
            stype = (data >> 1) & 0x7F
            if stype == 1:
                out["resets"] += 1
                return
            if stype not in (2, 3, 4):
                out["other_specials"] += 1
                return
        st = stamp(ts, self.overflow, t_offset_ns)
        if st is None:
            out["bad"] += 1
            return
        sec, nsec, ticks = st
        if self.etype == POLARITY:
            out["events"].append(((data >> 17) & 0x7FFF, (data >> 2) & 0x7FFF, sec, nsec, (data >> 1) & 1))
            out["ticks"].append(ticks)
        elif self.etype == SPECIAL:
            out["triggers"].append((sec, nsec, stype, int(stype != 3)))
        else:
            f = np.frombuffer(rec, "<f4", 6, 8)  # ax ay az gx gy gz
            # the float negated first, then widened to double, then the operations left to right
            acc = (np.float64(-f[0]) * 9.81, np.float64(f[1]) * 9.81, np.float64(-f[2]) * 9.81)
            gyr = tuple(np.float64(s) / 180.0 * np.pi for s in (-f[3], f[4], -f[5]))
            out["imu"].append((sec, nsec, acc, gyr))


def events_array(ev):
    a = np.zeros(len(ev), EVENT_DTYPE)
    for i, (x, y, sec, nsec, p) in enumerate(ev):
        a[i] = (x, y, sec, nsec, p)
    return a


def imu_array(imu):
    a = np.zeros(len(imu), IMU_DTYPE)
    for i, (sec, nsec, acc, gyr) in enumerate(imu):
        a[i] = (sec, nsec, acc, gyr)
    return a


def trigger_array(tr):
    a = np.zeros(len(tr), TRIGGER_DTYPE)
    for i, (sec, nsec, tid, value) in enumerate(tr):
        a["sec"][i], a["nsec"][i], a["id"][i], a["value"][i] = sec, nsec, tid, value
    return a


def decode(data, t_offset_ns=0, flags=0, mode="events"):
    """a whole stream through a fresh walker"""
    return Walker(mode).feed(data, t_offset_ns, flags)[1]


def decode_fast(data, t_offset_ns=0, flags=0):
    """the event rule over a whole, well-formed stream with numpy: the same integers as decode(), for streams too long
    for the byte loop (checked against it in tests/test_aedat_ref.py).  Returns (EVENT_DTYPE records, info dict)."""
    pos, n, parts, info = 0, len(data), [], {"invalid": 0, "bad": 0, "polarity_packets": 0, "other_packets": 0}
    while pos + 28 <= n:
        etype, _, size, ts_offset, overflow, capacity, number, _ = HEADER.unpack_from(data, pos)
        check_header(etype, size, ts_offset, capacity, number)
        pos += 28
        if etype == POLARITY:
            info["polarity_packets"] += 1
            k = min(number, (n - pos) // 8)
            rec = np.frombuffer(data, "<u4", 2 * k, pos).reshape(k, 2).astype(np.int64)
            parts.append(np.concatenate([rec, np.full((k, 1), overflow, np.int64)], axis=1))
        elif etype not in SIZES:
            info["other_packets"] += 1
        pos += capacity * size
    rec = np.concatenate(parts) if parts else np.zeros((0, 3), np.int64)
    if not flags & KEEP_INVALID:
        info["invalid"] = int((rec[:, 0] & 1 == 0).sum())
        rec = rec[rec[:, 0] & 1 == 1]
    data_w, ts, ovf = rec[:, 0], rec[:, 1], rec[:, 2]
    bad = (ts >= 2 ** 31) | (ovf < 0) | (ovf >= 2 ** 22)  # (ts as an int32 is negative; ts64 >= 2^53)
    ticks = (np.where(bad, 0, ovf) << 31 | np.where(bad, 0, ts)).astype(object) * 1000 + int(t_offset_ns)
    bad |= np.array([t < 0 or t >= 2 ** 32 * 10 ** 9 for t in ticks], bool)
    info["bad"] = int(bad.sum())
    ev = np.zeros(len(rec), EVENT_DTYPE)
    if not info["bad"]:
        t = ticks.astype(np.int64) if len(rec) else np.zeros(0, np.int64)
        ev["x"], ev["y"], ev["polarity"] = (data_w >> 17) & 0x7FFF, (data_w >> 2) & 0x7FFF, (data_w >> 1) & 1
        ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
        info["first_t_us"], info["last_t_us"] = (int(t[0]) // 1000, int(t[-1]) // 1000) if len(t) else (None, None)
    info["events"] = len(rec)
    return ev, info


def small_stream():
    """the ~300-byte stream the cut tests share: three polarity packets of 3 - 5 events (one of them invalid, one packet
    with padding, the last with overflow 1), a special packet, an IMU6 packet, a type-2 packet"""
    p1 = packet(POLARITY, [polarity(5, 7, 1, 100), polarity(345, 259, 0, 101), polarity(0, 0, 1, 101)])
    sp = packet(SPECIAL, [special(1, 102), special(2, 103)])
    p2 = packet(POLARITY, [polarity(1, 2, 0, 110), polarity(3, 4, 1, 111, valid=0), polarity(5, 6, 1, 112), polarity(7, 8, 0, 113)],
                capacity=5)
    im = packet(IMU6, [imu6(114, (0.1, -0.2, 0.98), (1.5, -2.5, 3.25))])
    fr = packet(FRAME, [bytes(range(12))], size=12)
    p3 = packet(POLARITY, [polarity(10 + k, 20 + k, k & 1, 5 + k) for k in range(5)], overflow=1)
    return p1 + sp + p2 + im + fr + p3
