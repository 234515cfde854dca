"""Inputs for the ingest chains at recording-sized calls: more tiles than the top scan has lanes.

Every chain that turns a stream into records is reduce (a summary per tile) -> ONE workgroup scans the summaries ->
emit.  A lane of that workgroup owns per = ceil(tiles / lanes) consecutive tiles.  With S = the scan's lanes the cases
here have S tiles (the last call with per == 1), S + 1 tiles (per == 2: lanes 0 .. S/2 - 1 own two tiles, lane S/2 one,
every lane behind it none) and 2S + 1 tiles (per == 3: an uneven split); the last tile always holds ONE item, so the
tile-count edge and the short-tail edge coincide.  Seeded numpy and the restatements beside this file; no device code.

  geometry       the tile sizes and scan widths as they stand (the GPU module passes the library's own)
  ownership      which lanes own how many tiles
  scan_model     the top scan as the kernels do it, and wrong variants of it
  *_case         a chain's input at a tile count;  *_expect: what the restatement says of it
  *_summaries    the per-tile summaries of a case, its prefixes and totals, from the restatement: what scan_model
                 must reproduce (tests/test_ingest_scale_cases.py)
"""
import numpy as np

import aedat_ref as A
import ba_filter2_ref as F2
import evt21_ref as R21
import slice_at_ref as SA
import slice_ref as SR
import text_ref as T
from esvio_amd.events import EVENT_DTYPE

EVT2, EVT3, EVT21 = R21.EVT2, R21.EVT3, R21.EVT21
LANES = {"raw": 256, "aedat": 256, "text": 256, "slice": 256, "filter": 1024, "pick": 256}
TILE = {"raw": 4096, "aedat": 1024, "text": 4096, "slice": 1024, "filter": 1024, "pick": 2048}  # raw, text: bytes
WAVE = 64


def geometry():
    return {k: (LANES[k], TILE[k]) for k in LANES}


def tile_counts(lanes):
    return {"S": lanes, "S+1": lanes + 1, "2S+1": 2 * lanes + 1}


def ownership(tiles, lanes):
    """per, and the tiles each lane owns: [(lo, hi)] as the kernels clamp them"""
    per = -(-tiles // lanes)
    own = [(min(t * per, tiles), min(min(t * per, tiles) + per, tiles)) for t in range(lanes)]
    return per, own


# ---- the top scan, as the kernels do it -----------------------------------------------------------------------------------
VARIANTS = ("per1", "total_from_predecessor", "reversed_fold", "no_clamp")


def scan_model(sums, lanes, combine, identity, seed, variant=None, beyond=None):
    """sums[j]: tile j's summary.  Returns (prefix, total, outside): prefix[j] = seed combined with every tile in front
    of j (None where no lane wrote one), total = what lane `lanes - 1` holds behind its write-back, outside = the
    indices >= len(sums) a lane read or wrote.  The steps are the kernels': per; lo / hi; a serial fold per lane; an
    inclusive scan inside each wave of 64 lanes (Hillis-Steele, as the shuffles do it); the waves' partials folded in
    order; the serial write-back; the last lane's run as the call's total.

    variant: "per1" — per forced to 1, the tiles beyond `lanes` never looked at; "total_from_predecessor" — the total
    taken in front of the last owning lane's run; "reversed_fold" — a lane folds its tiles last to first;
    "no_clamp" — hi = lo + per without min(.., tiles): the summaries behind the end read as `beyond` (the identity when
    None) — what such a kernel changes first is memory that is not its own, so the model reports the indices."""
    tiles = len(sums)
    per = 1 if variant == "per1" else -(-tiles // lanes)
    beyond = identity if beyond is None else beyond
    outside = []

    def read(j):
        if j >= tiles:
            outside.append(j)
            return beyond
        return sums[j]

    lo = [min(t * per, tiles) for t in range(lanes)]
    hi = [l + per if variant == "no_clamp" else min(l + per, tiles) for l in lo]
    lane_sum = []
    for t in range(lanes):
        s = identity
        js = range(lo[t], hi[t])
        for j in (reversed(js) if variant == "reversed_fold" else js):
            s = combine(s, read(j))
        lane_sum.append(s)
    incl = list(lane_sum)
    for w0 in range(0, lanes, WAVE):
        o = 1
        while o < WAVE:
            prev = list(incl[w0:w0 + WAVE])
            for l in range(o, min(WAVE, lanes - w0)):
                incl[w0 + l] = combine(prev[l - o], prev[l])
            o <<= 1
    part = [incl[min(w0 + WAVE, lanes) - 1] for w0 in range(0, lanes, WAVE)]
    prefix, total, before_last_owner = [None] * tiles, None, None
    for t in range(lanes):
        run = seed
        for w in range(t // WAVE):
            run = combine(run, part[w])
        if t % WAVE:
            run = combine(run, incl[t - 1])
        if lo[t] < tiles:
            before_last_owner = run
        for j in range(lo[t], hi[t]):
            s = read(j)
            if j < tiles:
                prefix[j] = run
            run = combine(run, s)
        if t == lanes - 1:
            total = run
    if variant == "total_from_predecessor":
        total = before_last_owner
    return prefix, total, sorted(set(outside))


def add(a, b):
    return a + b


# ---- raw: EVT3 / EVT2 / EVT2.1, events and triggers -------------------------------------------------------------------------
def raw_word_bytes(fmt):
    return R21.word_dtype(fmt).itemsize


def _raw_words(fmt):
    """the word builders of a format: other, th(v), event(rng, k) -> k event words, trigger(rng, k), the top TIME_HIGH"""
    if fmt == EVT3:
        return dict(other=0xE000, th=lambda v: 0x8000 | v, top=0xFFF, half=2048,
                    event=lambda rng, k: 0x2000 | rng.integers(0, 2, k) << 11 | rng.integers(0, 640, k),
                    trigger=lambda rng, k: 0xA000 | rng.integers(0, 16, k) << 8 | rng.integers(0, 2, k))
    if fmt == EVT2:
        return dict(other=0xE0000000, th=lambda v: 0x80000000 | v, top=0x0FFFFFFF, half=1 << 27,
                    event=lambda rng, k: rng.integers(0, 2, k) << 28 | rng.integers(0, 64, k) << 22 | rng.integers(0, 64, k) << 11 | rng.integers(0, 48, k),
                    trigger=lambda rng, k: 0xA << 28 | rng.integers(0, 64, k) << 22 | rng.integers(0, 32, k) << 8 | rng.integers(0, 2, k))
    return dict(other=0xE << 60, th=lambda v: 0x8 << 60 | v << 32, top=0x0FFFFFFF, half=1 << 27,
                event=lambda rng, k: (rng.integers(0, 2, k).astype(np.uint64) << np.uint64(60) | rng.integers(0, 64, k).astype(np.uint64) << np.uint64(54)
                                      | rng.integers(0, 600, k).astype(np.uint64) << np.uint64(43) | rng.integers(0, 480, k).astype(np.uint64) << np.uint64(32)
                                      | rng.integers(0, 1 << 32, k).astype(np.uint64) & rng.integers(0, 1 << 32, k).astype(np.uint64)),
                trigger=lambda rng, k: (np.uint64(0xA << 60) | rng.integers(0, 64, k).astype(np.uint64) << np.uint64(54)
                                        | rng.integers(0, 32, k).astype(np.uint64) << np.uint64(40) | rng.integers(0, 2, k).astype(np.uint64) << np.uint64(32)))


RAW_EVENTS_PER_TILE = (0, 0, 0, 1, 5, 40, 300)


def raw_case(fmt, tiles, lanes=LANES["raw"], tile_bytes=TILE["raw"], dense=False, seed=0):
    """(tiles - 1) full tiles and one word.  What lies where (TW = words per tile, per = tiles per lane):
      every word is an "other" word unless something below replaces it
      tile j gets RAW_EVENTS_PER_TILE[random] event words and a third as many trigger words at random places — most
        tiles none: runs of tiles whose transformer only counts `other`
      TIME_HIGH: the first one in tile 1 (tile 0's events are untimed); a wrap INSIDE lane 40's run (top in its first
        tile's last word, 1 in the next word); a wrap on the BOUNDARY of lanes 100 | 101 (top in the last word lane 100
        owns, 2 in the first word lane 101 owns); none behind it — every later lane takes the time base from lane 101
      EVT3: ADDR_Y in tiles j % 37 == 3, TIME_LOW in tiles j % 29 == 5; a vector base in lane 10's first tile, used by
        VECT_12 / VECT_8 words in lane 12's first tile; another base in the third tile from the end with one vector word
        behind it — the call ends with an open base
      the last word (alone in its tile) is an event word
    dense (EVT2.1): every event word's mask has ~24 bits — more records than words, for the second emit launch.
    `follow`: the small second call, no setter of its own: its records show the state the big call left."""
    rng = np.random.default_rng(1000 * fmt + tiles + seed)
    wb = raw_word_bytes(fmt)
    TW = tile_bytes // wb
    n = (tiles - 1) * TW + 1
    per, own = ownership(tiles, lanes)
    K = _raw_words(fmt)
    w = np.full(n, K["other"], np.uint64)
    per_tile = rng.choice(RAW_EVENTS_PER_TILE, tiles)
    per_tile[0] = RAW_EVENTS_PER_TILE[-1]         # events and triggers in front of the first TIME_HIGH: untimed
    for j in range(tiles):
        a, b = j * TW, min((j + 1) * TW, n)
        k = min(int(per_tile[j]), b - a)
        if k:
            at = a + rng.choice(b - a, k, replace=False)
            ev = K["event"](rng, k).astype(np.uint64)
            if dense:
                ev |= np.uint64(0x00FFFFFF)
            w[at] = ev
            w[at[:k // 3]] = K["trigger"](rng, k // 3).astype(np.uint64)
    marks = {}
    first_th = TW + 100
    w[first_th] = K["th"](5)
    a40, a100, a101 = own[40][0], own[100][1] - 1, own[101][0]
    w[(a40 + 1) * TW - 1], w[(a40 + 1) * TW] = K["th"](K["top"]), K["th"](1)
    w[(a100 + 1) * TW - 1], w[a101 * TW] = K["th"](K["top"]), K["th"](2)
    marks.update(first_th=first_th, wrap_inside=((a40 + 1) * TW - 1, (a40 + 1) * TW), wrap_boundary=((a100 + 1) * TW - 1, a101 * TW))
    if fmt == EVT3:
        for j in range(tiles - 1):
            if j % 37 == 3:
                w[j * TW + 11] = 0x0000 | int(rng.integers(0, 480))
            if j % 29 == 5:
                w[j * TW + 13] = 0x6000 | int(rng.integers(0, 4096))
        base, use = own[10][0] * TW + 7, own[12][0] * TW + 20
        w[base] = 0x3000 | 1 << 11 | 300
        w[use:use + 4] = [0x4FFF, 0x4A05, 0x50F0, 0x4001]
        late = (tiles - 3) * TW + 50
        w[late], w[late + 1] = 0x3000 | 77, 0x4F0F
        marks.update(vect_base=base, vect_use=use, late_base=late)
    w[n - 1] = K["event"](rng, 1).astype(np.uint64)[0] | np.uint64(0x00FFFFFF if dense else 0)
    if fmt == EVT3:
        follow = np.array([0x2000 | 33, 0x4F0F, 0x50FF, 0x2800 | 34, 0xA301, 0xE000], np.uint64)
    else:
        follow = np.concatenate([K["event"](rng, 3), K["trigger"](rng, 1), K["event"](rng, 2)]).astype(np.uint64)
    dt = R21.word_dtype(fmt)
    return dict(fmt=fmt, tiles=tiles, per=per, own=own, TW=TW, words=w.astype(dt), follow=follow.astype(dt), marks=marks)


def raw_plain(fmt, tiles, tile_bytes=TILE["raw"], seed=0):
    """the other camera of a two-camera call: (tiles - 1) full tiles and one word, a few tiles in all — a time base in
    word 3, events and others, one wrap in the middle; `follow` as raw_case's"""
    rng = np.random.default_rng(50 + fmt + tiles + seed)
    TW = tile_bytes // raw_word_bytes(fmt)
    n = (tiles - 1) * TW + 1
    K = _raw_words(fmt)
    w = np.full(n, K["other"], np.uint64)
    at = rng.choice(n, n // 5, replace=False)
    w[at] = K["event"](rng, len(at)).astype(np.uint64)
    w[3], w[n // 2], w[n // 2 + 1] = K["th"](9), K["th"](K["top"]), K["th"](0)
    w[n - 1] = K["event"](rng, 1).astype(np.uint64)[0]
    dt = R21.word_dtype(fmt)
    return dict(fmt=fmt, tiles=tiles, TW=TW, words=w.astype(dt), follow=K["event"](rng, 4).astype(dt))


def raw_expect(case):
    """the restatement over the big call and the follow-up, events and triggers (each decoder has a state of its own)"""
    out = {}
    st, ts = R21.fresh_state(), R21.fresh_state()
    for name in ("words", "follow"):
        out[name] = dict(events=R21.decode(case["fmt"], case[name], st), triggers=R21.decode_triggers(case["fmt"], case[name], ts))
    return out


def _raw_xf(fmt, words):
    """a run of words as a transformer of the decoder state, from the restatement: the run decoded from the fresh state
    tells the events in front of its first TIME_HIGH (untimed there), those behind it, the others, the wraps between its
    TIME_HIGH words and the fields as the run leaves them; which fields the run sets is read off the words' types"""
    s = R21.fresh_state()
    _, info = R21.decode(fmt, words, s)
    w = np.asarray(words).astype(np.uint64)
    typ = (w >> np.uint64(12 if fmt == EVT3 else 28 if fmt == EVT2 else 60)).astype(np.int64)
    ths = np.flatnonzero(typ == 8)
    x = dict(has_th=bool(len(ths)), th_first=0, th_last=s["th"], wraps=s["wraps"], before=info["untimed"], after=info["events"],
             other=info["other"], has_tl=False, tl=s["tl"], has_y=False, y=s["y"], has_bx=False, bx=s["bx"], bp=s["bp"])
    if len(ths):
        v = int(w[ths[0]])
        x["th_first"] = v & 0xFFF if fmt == EVT3 else v & 0x0FFFFFFF if fmt == EVT2 else (v >> 32) & 0x0FFFFFFF
    if fmt == EVT3:
        x["has_tl"], x["has_y"], x["has_bx"] = bool((typ == 6).any()), bool((typ == 0).any()), bool((typ == 3).any())
    return x


RAW_IDENTITY = dict(has_th=False, th_first=0, th_last=0, wraps=0, before=0, after=0, other=0, has_tl=False, tl=0, has_y=False, y=0,
                    has_bx=False, bx=0, bp=0)


def raw_combine(half):
    def combine(a, b):
        """a, then b"""
        c = dict(other=a["other"] + b["other"])
        if a["has_th"] and b["has_th"]:
            wrap = b["th_first"] < a["th_last"] and a["th_last"] - b["th_first"] >= half
            c.update(has_th=True, th_first=a["th_first"], th_last=b["th_last"], wraps=a["wraps"] + b["wraps"] + int(wrap),
                     before=a["before"], after=a["after"] + b["before"] + b["after"])
        elif a["has_th"]:
            c.update(has_th=True, th_first=a["th_first"], th_last=a["th_last"], wraps=a["wraps"], before=a["before"],
                     after=a["after"] + b["before"] + b["after"])
        else:
            c.update(has_th=b["has_th"], th_first=b["th_first"], th_last=b["th_last"], wraps=b["wraps"],
                     before=a["before"] + b["before"], after=b["after"])
        for k in ("tl", "y"):
            c["has_" + k] = a["has_" + k] or b["has_" + k]
            c[k] = b[k] if b["has_" + k] else a[k]
        c["has_bx"] = a["has_bx"] or b["has_bx"]
        c["bx"], c["bp"] = (b["bx"], b["bp"]) if b["has_bx"] else ((a["bx"] + b["bx"]) & 0xFFFF, a["bp"])
        return c
    return combine


def raw_state_xf(state):
    """a carried decoder state as the transformer that sets it"""
    return dict(RAW_IDENTITY, has_th=bool(state["seen"]), th_first=state["th"], th_last=state["th"], has_tl=True, tl=state["tl"],
                has_y=True, y=state["y"], has_bx=True, bx=state["bx"], bp=state["bp"])


def raw_xf_view(x):
    """what the emit kernels and the result block read of a run: the fields and the three counts"""
    return (x["has_th"], x["th_last"] if x["has_th"] else 0, x["wraps"], x["tl"], x["y"], x["bx"], x["bp"], x["before"], x["after"], x["other"])


def raw_summaries(case):
    """(sums, prefix, total) of the big call from the fresh state: sums[j] tile j's transformer, prefix[j] the view of
    the state and counts in front of tile j, total the view behind the call — prefix and total from the restatement run
    tile by tile over ONE carried state, which is the sequential decode of the whole call"""
    fmt, TW, w = case["fmt"], case["TW"], case["words"]
    sums, prefix = [], []
    s, ev, unt, oth = R21.fresh_state(), 0, 0, 0
    for j in range(case["tiles"]):
        tile = w[j * TW:(j + 1) * TW]
        sums.append(_raw_xf(fmt, tile))
        prefix.append((bool(s["seen"]), s["th"], s["wraps"], s["tl"], s["y"], s["bx"], s["bp"], unt, ev, oth))
        _, info = R21.decode(fmt, tile, s)
        ev, unt, oth = ev + info["events"], unt + info["untimed"], oth + info["other"]
    total = (bool(s["seen"]), s["th"], s["wraps"], s["tl"], s["y"], s["bx"], s["bp"], unt, ev, oth)
    return sums, prefix, total


# ---- AEDAT 3.1 -----------------------------------------------------------------------------------------------------------
def aedat_case(tiles, lanes=LANES["aedat"], tile=TILE["aedat"], seed=0):
    """(tiles - 1) * tile + 1 polarity records.  A tile's share of valid records is 0, 1 or a fraction, by its class:
    runs of two and of three tiles are wholly invalid, some tiles wholly valid.  Packets of 50 000 records with
    eventTSOverflow 0; behind `step` — a record of tile S (with S + 1 tiles its only one; in the S-tile case the middle of the
    last full tile) — packets with overflow 1: a new run of the walk's run table.  The chunk ends 4 bytes into a record of a packet that declares 5
    more: `follow`, the second call, completes it."""
    rng = np.random.default_rng(77 + tiles + seed)
    n = (tiles - 1) * tile + 1
    per, own = ownership(tiles, lanes)
    cls = rng.choice(5, tiles)                       # 0: all invalid, 1: all valid, 2..4: a share
    for j in range(3, tiles - 4, 23):
        cls[j:j + 2 + (j // 23) % 2] = 0             # runs of two / three wholly invalid tiles
    cls[tiles - 1] = 1                               # the last record counts
    share = np.array([0.0, 1.0, 0.1, 0.5, 0.9])[cls]
    valid = rng.random(n + 5) < np.repeat(share, tile)[:n + 5]
    valid[np.repeat(cls, tile)[:n + 5] == 1] = True
    valid[n:] = [True, False, True, True, True]
    step = min(lanes * tile + 517, n - 1) if tiles > lanes else (tiles - 2) * tile + tile // 2
    x, y, p = rng.integers(0, 346, n + 5), rng.integers(0, 260, n + 5), rng.integers(0, 2, n + 5)
    ts = 1000 + np.arange(n + 5, dtype=np.int64) // 3
    ts[step:] -= ts[step] - 5                        # the stamps begin again behind the overflow step
    rec = np.zeros((n + 5, 2), "<u4")
    rec[:, 0] = valid.astype(np.int64) | p << 1 | y << 2 | x << 17
    rec[:, 1] = ts
    raw = rec.tobytes()
    edges = sorted(set(list(range(0, n + 5, 50_000)) + [step, n + 5]))
    data = b"".join(A.packet(A.POLARITY, [raw[8 * a:8 * b]], overflow=int(a >= step), number=b - a) for a, b in zip(edges, edges[1:]))
    cut = 28 * sum(1 for a in edges[:-1] if a <= n) + 8 * n + 4   # the headers in front of record n, n records, 4 bytes
    return dict(tiles=tiles, per=per, own=own, tile=tile, n=n, valid=valid, step=step, cls=cls, data=data[:cut], follow=data[cut:])


def aedat_expect(case):
    """the sequential reading over both calls: [(records, result dict)]"""
    w, out = A.Walker("events"), []
    for name in ("data", "follow"):
        w, o = w.feed(case[name])
        out.append((A.events_array(o["events"]), o))
    return out


def aedat_summaries(case):
    """valid records per tile, from the walk's own record list"""
    _, o = A.Walker("events").feed(case["data"])
    v = np.array([r[0][0] & 1 for r in o["records"]], np.int64)
    assert len(v) == case["n"]
    T_ = case["tile"]
    sums = [int(v[j * T_:(j + 1) * T_].sum()) for j in range(case["tiles"])]
    return sums, [int(v[:j * T_].sum()) for j in range(case["tiles"])], len(o["events"])


# ---- text -------------------------------------------------------------------------------------------------------------------
def text_case(tiles, lanes=LANES["text"], tile=TILE["text"], late=False, seed=0):
    """(tiles - 1) * tile + 1 bytes of "sec.nsec x y p" lines (extract_davis_bag_files.py's).  The mix of lines goes by
    the tile a line begins in: event lines alone, comments, blank lines, or all of them.  Malformed lines (a fifth
    column) only behind `first_bad`, which lies in the last tile but two — a large first_malformed — unless an overlong
    line comes first: with 2S + 1 tiles and not `late`, one line of two and a half tiles lies wholly in front of tile S
    and one straddles its start (tiles without a line start inside a lane's run); with `late` only the straddling one is
    kept out and the first malformed line lies behind tile S.  The chunk ends inside an event line; `follow` is the rest
    of that line and three more."""
    rng = np.random.default_rng(31 + tiles + seed + 7 * late)
    n = (tiles - 1) * tile + 1
    per, own = ownership(tiles, lanes)
    cls = rng.choice(4, tiles + 2)
    first_bad = (tiles - 3) * tile + 100
    over = {}
    if tiles > 2 * lanes:
        over = {lanes * tile - tile // 2: "straddling"} if not late else {}
        if not late:
            over[(lanes // 3) * tile + 200] = "in front"
        else:
            first_bad = (lanes + 5) * tile + 100
            over[(lanes + 40) * tile + 9] = "behind"
    parts, pos, t_ns, k = [], 0, 5 * 10 ** 9, 0
    pending = sorted(over)
    marks = dict(overlong=[], first_bad=None)
    while pos < n + 200:
        if pending and pos >= pending[0]:
            pending.pop(0)
            line = b"x" * (5 * tile // 2) + b"\n"
            marks["overlong"].append(pos)
        else:
            c = cls[pos // tile]
            r = rng.integers(0, 8)
            t_ns += int(rng.integers(1, 5000))
            ev = b"%d.%09d %d %d %d\n" % (t_ns // 10 ** 9, t_ns % 10 ** 9, rng.integers(0, 346), rng.integers(0, 260), k & 1)
            if pos >= first_bad and r == 0:
                line = ev[:-1] + b" 9\n"
                if marks["first_bad"] is None:
                    marks["first_bad"] = pos
            elif c == 1 and r < 6:
                line = b"# c %d\n" % k
            elif c == 2 and r < 6:
                line = (b"\n", b" \n", b"\r\n")[k % 3]
            elif c == 3 and r < 3:
                line = (b"% x\n", b"\t\n", b"#\r\n")[k % 3]
            else:
                line = ev
            k += 1
        parts.append(line)
        pos += len(line)
    data = b"".join(parts)
    # the byte the big call ends on is no '\n' and lies inside an EVENT line whose first byte the call holds
    while not _ends_in_event_line(data, n):
        data = b" " + data
        marks = dict(overlong=[o + 1 for o in marks["overlong"]], first_bad=marks["first_bad"] + 1)
    end = data.index(b"\n", n)
    for _ in range(3):
        end = data.index(b"\n", end + 1)
    return dict(tiles=tiles, per=per, own=own, tile=tile, n=n, data=data[:n], follow=data[n:end + 1], marks=marks, cls=cls)


def _ends_in_event_line(data, n):
    start = data.rfind(b"\n", 0, n) + 1
    line = data[start:data.index(b"\n", n)]
    return data[n - 1:n] != b"\n" and start < n - 1 and len(line) <= 64 and T.classify(line, T.TXYP, T.SEC_DECIMAL)[0] == "event"


def text_expect(case):
    """the sequential reading over both calls: [(records array, info)], and the state behind the big call"""
    st, out = T.fresh(), []
    for name in ("data", "follow"):
        recs, info, ok, st2 = T.read(st, T.TXYP, T.SEC_DECIMAL, T.SKIP_MALFORMED, case[name])
        assert ok
        out.append((T.records_array(recs), info, st2))
        st = st2
    return out


def text_summaries(case):
    """per tile (by the byte a line begins on) the event lines; every line classified by the restatement's classify —
    (sums, prefix, total, per-tile class counts)"""
    data, tile = case["data"], case["tile"]
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    starts = np.concatenate([[0], nl[:-1] + 1]) if len(nl) else np.zeros(0, np.int64)
    counts = np.zeros((case["tiles"], 4), np.int64)   # event, comment, blank, malformed
    for s, e in zip(starts.tolist(), nl.tolist()):
        body = data[s:e]
        if body.endswith(b"\r"):
            body = body[:-1]
        c = T.classify(body, T.TXYP, T.SEC_DECIMAL)[0]
        counts[s // tile, {"event": 0, "bad": 0, "comment": 1, "blank": 2, "malformed": 3}[c]] += 1
    sums = counts[:, 0].tolist()
    return sums, np.concatenate([[0], np.cumsum(sums)[:-1]]).tolist(), int(counts[:, 0].sum()), counts


# ---- slicing ----------------------------------------------------------------------------------------------------------------
SLICE_FREQ, SLICE_ORIGIN, SLICE_PERIOD_NS = 30.0, (10, 0), 33_333_333


def slice_case(tiles, lanes=LANES["slice"], tile=TILE["slice"], seed=0):
    """(tiles - 1) * tile + 1 events.  Event i lies 1 ms + i ns inside window w_i, and w_i rises by one at few places:
    early ones, the last event of tile S - 1, the first event of tile S (where the stream has them), the last event of
    the last full tile and the stream's last event — so long runs of tiles have one running maximum.  One and a half
    tiles inside lane 120's run step back three windows: a tile whose own maximum lies below the prefix.  `follow`: 300
    more events that close two more windows.  `bounds`: the same windows' ends as stamps, for slicing at given stamps."""
    n = (tiles - 1) * tile + 1
    per, own = ownership(tiles, lanes)
    closes = {5 * tile + 3, 20 * tile, 50 * tile + 1000, 100 * tile + 17, (tiles - 1) * tile - 1, (tiles - 1) * tile}
    if tiles > lanes:
        closes |= {lanes * tile - 1, lanes * tile}
    closes = sorted(c for c in closes if 0 < c < n)
    i = np.arange(n + 300, dtype=np.int64)
    w = np.searchsorted(np.array(closes + [n + 100, n + 200]), i, side="right")
    back = (own[120][0] * tile + tile // 2, 0)
    back = (back[0], back[0] + 3 * tile // 2)
    assert w[back[0]] >= 3 and back[1] < n
    w[back[0]:back[1]] -= 3
    t = SLICE_ORIGIN[0] * 10 ** 9 + w * SLICE_PERIOD_NS + 1_000_000 + i
    ev = np.zeros(n + 300, EVENT_DTYPE)
    rng = np.random.default_rng(5 + tiles + seed)
    ev["x"], ev["y"], ev["polarity"] = rng.integers(0, 64, n + 300), rng.integers(0, 48, n + 300), rng.integers(0, 2, n + 300)
    ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    s = SR.Slicer(SLICE_FREQ, SLICE_ORIGIN)
    bounds = [s.boundary(k) for k in range(len(closes) + 4)]
    return dict(tiles=tiles, per=per, own=own, tile=tile, n=n, ev=ev[:n], follow=ev[n:], closes=closes, back=back, bounds=bounds)


def slice_expect(case, at=False):
    """the restatement over both calls: [(cuts, info)]; at: slicing at the given stamps, the second call with the
    boundaries from the closed count on"""
    out = []
    if at:
        s, b = SA.SlicerAt(), list(case["bounds"])
        for name in ("ev", "follow"):
            ev = case[name]
            cuts, info = s.push(ev["sec"], ev["nsec"], b)
            out.append((cuts, info, list(b)))
            b = b[info["closed"]:]
        return out
    s = SR.Slicer(SLICE_FREQ, SLICE_ORIGIN)
    for name in ("ev", "follow"):
        ev = case[name]
        cuts, info = s.push(ev["sec"], ev["nsec"])
        out.append((cuts, info, None))
    return out


def slice_summaries(case):
    """per tile the largest count of boundaries at or below an event's stamp; prefix[j] = the windows closed in front of
    tile j and the total, both from the restatement's cuts"""
    ev, tile = case["ev"], case["tile"]
    b = np.array([SR.to_sec(*k) for k in case["bounds"]])
    c = np.searchsorted(b, ev["sec"].astype(np.float64) + 1e-9 * ev["nsec"].astype(np.float64), side="right")
    sums = [int(c[j * tile:(j + 1) * tile].max()) for j in range(case["tiles"])]
    cuts, info = SR.Slicer(SLICE_FREQ, SLICE_ORIGIN).push(ev["sec"], ev["nsec"])
    cuts = np.array(cuts)
    return sums, [int((cuts < j * tile).sum()) for j in range(case["tiles"])], info["closed"]


# ---- the filter ---------------------------------------------------------------------------------------------------------------
FILTER_W, FILTER_H, FILTER_WINDOW_NS, FILTER_REFRACTORY_NS = 64, 48, 1_000_000, 5_000


def filter_case(blocks, lanes=LANES["filter"], block=TILE["filter"], seed=0):
    """(blocks - 1) * block + 1 events on a 64 x 48 sensor, a pattern per block: 0 — 2 ms between events, each far from
    the one before: nothing has support; 1 — three pixels of a row in turn, 2 us apart: every event has support and its
    own pixel's stamp is 6 us old (such blocks come in pairs, so that the second one keeps all of its events); 2 — the
    same with every pixel hit twice, 1 us apart: the refractory test drops every second event; 3.. — random pixels of a
    small square, 1 .. 2000 us apart, a few of them outside the sensor: a share that goes with the square's side.  The
    last blocks are of kind 1, so the last event, alone in its block, is kept."""
    rng = np.random.default_rng(900 + blocks + seed)
    n = (blocks - 1) * block + 1
    per, own = ownership(blocks, lanes)
    kind = rng.choice(6, blocks)
    kind[1::8] = 1
    kind[2::8] = 1
    kind[blocks - 3:] = 1
    kb = np.repeat(kind, block)[:n]
    i = np.arange(n)
    side = np.where(kb >= 3, 4 * kb, 1)
    x = np.select([kb == 0, kb == 1, kb == 2], [(7 * i) % FILTER_W, 20 + i % 3, 30 + (i >> 1) % 3], 5 + rng.integers(0, 24, n) % side)
    y = np.select([kb == 0, kb == 1, kb == 2], [(5 * (i // 9)) % FILTER_H, 20, 30], 9 + rng.integers(0, 24, n) % side)
    out = (kb >= 3) & (rng.integers(0, 97, n) == 0)
    x = np.where(out, FILTER_W + rng.integers(0, 9, n), x)
    dt = np.select([kb == 0, kb == 1, kb == 2], [2_000_000, 2_000, 1_000], rng.integers(1, 2000, n) * 1000)
    t = 10 ** 9 + np.cumsum(dt)
    ev = np.zeros(n, EVENT_DTYPE)
    ev["x"], ev["y"], ev["polarity"] = x, y, rng.integers(0, 2, n)
    ev["sec"], ev["nsec"] = t // 10 ** 9, t % 10 ** 9
    return dict(tiles=blocks, per=per, own=own, tile=block, n=n, ev=ev, kind=kind)


def filter_fast(B, W, H, ev, window_ns, min_support=1, refractory_ns=0):
    """ba_filter2_ref.filter_events with numpy: the same flags, count and plane, for calls too long for the loop (proved
    equal to it in tests/test_ingest_scale_cases.py; the loop stays the authority).  The stamp a pixel holds when event
    i looks at it is that of the last earlier event of the call on that pixel, else the plane's: the events sorted by
    (pixel, index), one bisection per event and neighbour."""
    n = len(ev)
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    t = ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"].astype(np.int64)
    idx = np.flatnonzero((x < W) & (y < H))
    flags = np.zeros(n, np.uint8)
    if not len(idx):
        return flags, n
    xi, yi, ti = x[idx], y[idx], t[idx]
    pix = xi + yi * W
    order = np.argsort(pix, kind="stable")
    key = pix[order] * n + idx[order]
    ts = ti[order]

    def stamp_at(q, ok):
        """the stamp pixel q holds in front of each event (NONE where !ok)"""
        q = np.where(ok, q, 0)
        pos = np.searchsorted(key, q * n + idx, side="left") - 1
        hit = (pos >= 0) & (key[np.maximum(pos, 0)] // n == q)
        return np.where(ok, np.where(hit, ts[np.maximum(pos, 0)], B[q]), F2.NONE)

    keep = np.ones(len(idx), bool)
    if min_support > 0:
        support = np.zeros(len(idx), np.int64)
        for dx, dy in F2.NEIGHBOURS:
            u, v = xi + dx, yi + dy
            ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            b = stamp_at(u + v * W, ok)
            support += ok & (b != F2.NONE) & (ti - b < window_ns)
        keep = support >= min_support
    if refractory_ns > 0:
        own = stamp_at(pix, np.ones(len(idx), bool))
        keep &= ~((own != F2.NONE) & (ti - own < refractory_ns))
    flags[idx] = keep
    last = np.flatnonzero(np.concatenate([key[1:] // n != key[:-1] // n, [True]]))
    B[key[last] // n] = ts[last]
    return flags, n - len(idx)


def filter_expect(case, refractory, fast=True):
    """(flags, rejected, plane behind the call) from a fresh plane"""
    B = F2.fresh_plane(FILTER_W, FILTER_H)
    f = filter_fast if fast else F2.filter_events
    flags, rej = f(B, FILTER_W, FILTER_H, case["ev"], FILTER_WINDOW_NS, 1, FILTER_REFRACTORY_NS if refractory else 0)
    return flags, rej, B


def filter_summaries(case, flags):
    tile = case["tile"]
    sums = [int(flags[j * tile:(j + 1) * tile].sum()) for j in range(case["tiles"])]
    return sums, np.concatenate([[0], np.cumsum(sums)[:-1]]).tolist(), int(flags.sum())


# ---- the seeding pick ---------------------------------------------------------------------------------------------------------
PICK_KINDS = ("whole sum", "first non-zero", "below first non-zero", "on a running sum", "between", "beyond")


def pick_case(tiles, lanes=LANES["pick"], tile=TILE["pick"], seed=0):
    """(tiles - 1) * tile + 1 values up to 256 (at that size values this small sum to 2^27 at the most, so every
    seventh tile holds values up to 2^22: the sums pass 32 bits), zero runs over the whole tiles on either side of B,
    the first value lane S/2 owns, and segments that lie inside lane S/2 - 1's tiles, end on B, are empty at B, straddle
    B by one value and by more than a tile"""
    rng = np.random.default_rng(4 + tiles + seed)
    n = (tiles - 1) * tile + 1
    per, own = ownership(tiles, lanes)
    md = rng.integers(0, 257, n).astype(np.uint32)
    for j in range(0, tiles - 1, 7):
        md[j * tile:(j + 1) * tile] = rng.integers(0, 1 << 22, tile)
    B = own[lanes // 2][0] * tile if own[lanes // 2][0] < tiles else n
    B = min(B, n)
    md[B - tile:min(B + tile, n)] = 0
    edges = [0, 5000, B - 3 * tile - 7, B - 2 * tile + 5, B - tile // 2, B, B, min(B + 1, n), min(B + tile + 9, n), n]
    return dict(tiles=tiles, per=per, own=own, tile=tile, n=n, md=md, seg_off=np.array(edges, np.uint32), B=B)


def pick_cuts(case, kind):
    md, edges = case["md"], case["seg_off"].tolist()
    cut = []
    for a, b in zip(edges, edges[1:]):
        seg = md[a:b].astype(np.int64)
        total, nz = int(seg.sum()), seg[seg > 0]
        if kind == "whole sum" or not len(nz):
            cut.append(float(total))
        elif kind == "first non-zero":
            cut.append(float(nz[0]))
        elif kind == "below first non-zero":
            cut.append(float(nz[0]) - 0.5)
        elif kind == "on a running sum":
            cut.append(float(np.cumsum(seg)[len(seg) // 2]))
        elif kind == "between":
            cut.append(float(np.cumsum(seg)[len(seg) // 3]) + 0.25)
        else:
            cut.append(float(total) + 1.0)
    return np.array(cut)


def pick_summaries(case):
    md, tile = case["md"].astype(np.uint64), case["tile"]
    sums = [int(md[j * tile:(j + 1) * tile].sum()) for j in range(case["tiles"])]
    run = np.cumsum(md)
    return sums, [int(run[j * tile - 1]) if j else 0 for j in range(case["tiles"])], int(run[-1])
