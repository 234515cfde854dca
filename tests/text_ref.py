"""The sequential reading of include/esvio_fe.h "text event files", and writers that follow the lines of the three
writers the rule cites.  Dicts, lists, int() and string methods; nothing here knows of tiles or of the device.

    read(state, order, time, flags, data, t_offset_ns, cap) -> (records, info, ok, state')
        state   {"tail": bytes, "skip": bool, "skip_len": int}   (fresh(): the state of a new handle)
        records [(x, y, sec, nsec, polarity), ...] in line order
        info    the fields of esvio_fe_text_info (first_malformed None: no malformed line; first_t_ns, last_t_ns and
                carried: of a call that succeeds)
        ok      False: the call is refused, state' is state
"""
import numpy as np

TXYP, XYPT = 1, 2
SEC_DECIMAL, INT_US, INT_NS = 1, 2, 3
END, SKIP_MALFORMED = 1, 2
SEPARATORS = b" \t,"
TICK_LIMIT = (1 << 32) * 10 ** 9


def fresh():
    return {"tail": b"", "skip": False, "skip_len": 0}


def stamp_ns(token, time):
    """the stamp token's nanoseconds, or None: malformed"""
    if time == SEC_DECIMAL:
        whole, dot, frac = token.partition(b".")
        if not whole.isdigit() or len(whole) > 10:
            return None
        if dot and not frac.isdigit():
            return None  # (an empty fraction, or a byte that is no digit)
        return int(whole) * 10 ** 9 + int(frac[:9].ljust(9, b"0") or b"0")
    if not token.isdigit() or len(token) > 19:
        return None
    return int(token) * 1000 if time == INT_US else int(token)


def classify(body, order, time, t_offset_ns=0):
    """one line's body -> ("blank" | "comment" | "malformed" | "bad", None) or ("event", (x, y, sec, nsec, p, ticks))"""
    if len(body) > 64:
        return "malformed", None
    s = body.strip(SEPARATORS)
    if not s:
        return "blank", None
    if s[:1] in (b"#", b"%"):
        return "comment", None
    tokens = [t for t in s.replace(b"\t", b" ").replace(b",", b" ").split(b" ") if t]
    if len(tokens) != 4:
        return "malformed", None
    tok = dict(zip("txyp" if order == TXYP else "xypt", tokens))
    xy = []
    for k in "xy":
        if not tok[k].isdigit() or len(tok[k]) > 5 or int(tok[k]) > 65535:
            return "malformed", None
        xy.append(int(tok[k]))
    if tok["p"] not in (b"0", b"1", b"-1"):
        return "malformed", None
    ns = stamp_ns(tok["t"], time)
    if ns is None:
        return "malformed", None
    ticks = ns + t_offset_ns
    if ticks < 0 or ticks >= TICK_LIMIT:
        return "bad", None
    return "event", (xy[0], xy[1], ticks // 10 ** 9, ticks % 10 ** 9, 1 if tok["p"] == b"1" else 0, ticks)


def read(state, order, time, flags, data, t_offset_ns=0, cap=None):
    data = bytes(data)
    info = dict(events=0, lines=0, comments=0, blank=0, malformed=0, bad=0, first_malformed=None, first_t_ns=None, last_t_ns=None,
                carried=len(state["tail"]))
    records, ticks = [], []
    st = dict(state)

    def line(body, at):  # body None: a line whose body passed 64 bytes long ago
        cls, rec = ("malformed", None) if body is None else classify(body, order, time, t_offset_ns)
        info["lines"] += 1
        if cls in ("event", "bad"):
            info["events"] += 1
            info["bad"] += cls == "bad"
            if rec:
                records.append(rec[:5])
                ticks.append(rec[5])
        else:
            info[{"comment": "comments"}.get(cls, cls)] += 1
            if cls == "malformed" and info["first_malformed"] is None:
                info["first_malformed"] = at

    pos = 0
    while True:
        nl = data.find(b"\n", pos)
        if nl < 0:
            break
        at = pos - (st["skip_len"] if st["skip"] else len(st["tail"]))
        if st["skip"]:
            line(None, at)
        else:
            body = st["tail"] + data[pos:nl]
            line(body[:-1] if body.endswith(b"\r") else body, at)
        st, pos = fresh(), nl + 1
    rest = data[pos:]
    if st["skip"]:
        st["skip_len"] += len(rest)
    else:
        tail = st["tail"] + rest
        if len(tail) > 65 or (len(tail) == 65 and not tail.endswith(b"\r")):  # the body has passed 64 bytes
            st = {"tail": b"", "skip": True, "skip_len": len(tail)}
        else:
            st = {"tail": tail, "skip": False, "skip_len": 0}
    if flags & END:
        if st["skip"]:
            line(None, len(data) - st["skip_len"])
        elif st["tail"]:
            line(st["tail"], len(data) - len(st["tail"]))
        st = fresh()
    ok = not ((info["malformed"] and not flags & SKIP_MALFORMED) or info["bad"] or (cap is not None and info["events"] > cap))
    if ok:
        info["carried"] = len(st["tail"])
        if ticks:
            info["first_t_ns"], info["last_t_ns"] = ticks[0], ticks[-1]
    return records, info, ok, (st if ok else state)


def records_array(records):
    """the records as esvio_amd.events.EVENT_DTYPE (the padding bytes 0)"""
    from esvio_amd.events import EVENT_DTYPE
    ev = np.zeros(len(records), EVENT_DTYPE)
    for k, name in enumerate(("x", "y", "sec", "nsec", "polarity")):
        ev[name] = [r[k] for r in records]
    return ev


# ---- the cited writers' lines (events: (x, y, sec, nsec, polarity) tuples)
def write_davis(events):
    """extract_davis_bag_files.py: timestamp_str = str(secs) + "." + str(nsecs).zfill(9), then x, y, "1" / "0\""""
    return "".join(str(sec) + "." + str(nsec).zfill(9) + " " + str(x) + " " + str(y) + " " + ("1" if p else "0") + "\n"
                   for x, y, sec, nsec, p in events).encode()


def write_dvs(events):
    """extract_dvs_bag_files.py: x, y, 1 / 0, to_nsec() / 1000 in integers"""
    return "".join(str(x) + " " + str(y) + " " + str(1 if p else 0) + " " + str((sec * 10 ** 9 + nsec) // 1000) + "\n"
                   for x, y, sec, nsec, p in events).encode()


def write_cpp(events):
    """writer.cpp: the same columns through operator<< (an int polarity), std::endl"""
    return write_dvs(events)


def write_csv(events):
    """a Prophesee CSV export: x,y,p,t in microseconds"""
    return "".join("%d,%d,%d,%d\n" % (x, y, 1 if p else 0, (sec * 10 ** 9 + nsec) // 1000) for x, y, sec, nsec, p in events).encode()
