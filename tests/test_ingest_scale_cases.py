"""CPU: the inputs of tests/ingest_scale_cases.py reach the edges they are built for — the tile counts around the top
scan's width S, which lanes own how many tiles, the properties each chain's fold needs to be wrong-able — and a numpy
model of the top scan reproduces the restatement's prefixes and totals from the per-tile summaries while its wrong
variants do not.  Also: the vectorised filter restatement equals the loop (the loop stays the authority)."""
import functools

import numpy as np
import pytest

import ba_filter2_ref as F2
import ba_filter_cases as BK
import evt21_ref as R21
import ingest_scale_cases as K
import text_ref as T

KINDS = ("S", "S+1", "2S+1")
FMTS = (K.EVT3, K.EVT2, K.EVT21)


def tiles_of(chain, kind):
    return K.tile_counts(K.LANES[chain])[kind]


@functools.lru_cache(maxsize=None)
def raw(fmt, kind):
    return K.raw_case(fmt, tiles_of("raw", kind))


@functools.lru_cache(maxsize=None)
def raw_exp(fmt, kind):
    return K.raw_expect(raw(fmt, kind))


@functools.lru_cache(maxsize=None)
def aedat(kind):
    return K.aedat_case(tiles_of("aedat", kind))


@functools.lru_cache(maxsize=None)
def text(kind, late=False):
    return K.text_case(tiles_of("text", kind), late=late)


@functools.lru_cache(maxsize=None)
def slices(kind):
    return K.slice_case(tiles_of("slice", kind))


@functools.lru_cache(maxsize=None)
def filt(kind):
    return K.filter_case(tiles_of("filter", kind))


@functools.lru_cache(maxsize=None)
def pick(kind):
    return K.pick_case(tiles_of("pick", kind))


# ---- the geometry ----------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_ones_the_evidence_here_is_about():
    assert K.geometry() == {"raw": (256, 4096), "aedat": (256, 1024), "text": (256, 4096), "slice": (256, 1024),
                            "filter": (1024, 1024), "pick": (256, 2048)}


def test_the_tap_returns_the_scan_widths_without_a_device():
    import ctypes as C
    from esvio_amd import frontend as FE
    L, s = FE.load_library(), FE.scan_lanes()
    assert "esvio_fe_scan_lanes" in FE.TEST_SYMBOLS and C.sizeof(FE.ScanLanes) == 32 and L.esvio_fe_scan_lanes(None) == -1
    assert {k: getattr(s, k) for k in K.LANES} == K.LANES
    assert (s.filter_block_events, s.pick_tile_values) == (K.TILE["filter"], K.TILE["pick"])
    assert (L.esvio_fe_raw_tile_bytes(), L.esvio_fe_aedat_tile_events(), FE.text_limits().tile_bytes, L.esvio_fe_slice_tile_events()) == \
        (K.TILE["raw"], K.TILE["aedat"], K.TILE["text"], K.TILE["slice"])


def check_ownership(case, chain, kind, items):
    S, T_ = K.LANES[chain], case["tile"]
    tiles, own = case["tiles"], case["own"]
    owned = [hi - lo for lo, hi in own]
    assert tiles == {"S": S, "S+1": S + 1, "2S+1": 2 * S + 1}[kind] and items == (tiles - 1) * T_ + 1   # one item in the last tile
    assert sum(owned) == tiles and [lo for lo, hi in own if hi > lo] == sorted(lo for lo, hi in own if hi > lo)
    if kind == "S":
        assert case["per"] == 1 and owned == [1] * S                      # lane S - 1 owns a real tile
    elif kind == "S+1":
        assert case["per"] == 2 and owned == [2] * (S // 2) + [1] + [0] * (S // 2 - 1)
        assert own[S - 1] == (tiles, tiles)                               # ... and the last lane nothing: lo == hi == tiles
    else:
        n3 = tiles // 3                                                   # 2S + 1 = 3 * 171 for S = 256
        assert case["per"] == 3 and owned == [3] * n3 + [tiles - 3 * n3] * (tiles % 3 != 0) + [0] * (S - n3 - (tiles % 3 != 0))
        assert n3 % K.WAVE != 0 and S - n3 > K.WAVE                       # the owners end inside a wave; a whole wave owns nothing


@pytest.mark.parametrize("kind", KINDS)
def test_tile_counts_and_owning_lanes(kind):
    for fmt in FMTS:
        c = raw(fmt, kind)
        check_ownership(dict(c, tile=c["TW"]), "raw", kind, len(c["words"]))
        assert c["words"].nbytes == (c["tiles"] - 1) * K.TILE["raw"] + K.raw_word_bytes(fmt)
    check_ownership(aedat(kind), "aedat", kind, aedat(kind)["n"])
    check_ownership(text(kind), "text", kind, len(text(kind)["data"]))
    check_ownership(slices(kind), "slice", kind, len(slices(kind)["ev"]))
    check_ownership(pick(kind), "pick", kind, len(pick(kind)["md"]))
    if kind != "2S+1":
        check_ownership(filt(kind), "filter", kind, len(filt(kind)["ev"]))
    if kind == "2S+1":
        check_ownership(text(kind, True), "text", kind, len(text(kind, True)["data"]))


# ---- the model against the restatement, and its wrong variants -----------------------------------------------------------------
def run_variants(sums, prefix, total, lanes, combine, identity, seed, view=lambda v: v):
    """the right model must equal (prefix, total) and stay inside; -> {variant: what differs}"""
    def views(r):
        return [None if p is None else view(p) for p in r[0]], (None if r[1] is None else view(r[1])), r[2]
    right = views(K.scan_model(sums, lanes, combine, identity, seed))
    assert right[0] == list(prefix) and right[1] == total and right[2] == []
    out = {}
    for v in K.VARIANTS:
        got = views(K.scan_model(sums, lanes, combine, identity, seed, v))
        out[v] = {n for n, a, b in zip(("prefix", "total", "outside"), got, right) if a != b}
    return out


def expected(kind, commutative=True, last_tile_counts=True, has_total=True):
    """what each wrong variant must change at a tile count.  per1 and no_clamp are the right scan while per == 1; a
    reversed fold shows only where the fold is not commutative; the total taken in front of the last owning lane's run
    lacks that run — with S and S + 1 tiles the one item of the last tile, so it shows where that item counts"""
    big = kind != "S"
    dropped_count = has_total and (last_tile_counts or kind == "2S+1")   # (with S + 1 tiles per1 drops the last tile alone)
    return {"per1": ({"prefix"} | ({"total"} if dropped_count else set())) if big else set(),
            "no_clamp": {"outside"} if big else set(),
            "reversed_fold": {"prefix"} if big and not commutative else set(),
            "total_from_predecessor": {"total"} if dropped_count else set()}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_raw_scan_model(fmt, kind):
    c = raw(fmt, kind)
    sums, prefix, total = K.raw_summaries(c)
    half = 2048 if fmt == K.EVT3 else 1 << 27
    diff = run_variants(sums, prefix, total, K.LANES["raw"], K.raw_combine(half), K.RAW_IDENTITY, K.raw_state_xf(R21.fresh_state()),
                        K.raw_xf_view)
    want = expected(kind, commutative=False)
    if kind != "S":
        assert "prefix" in diff["reversed_fold"]      # the inputs exercise the fold's order
        diff["reversed_fold"] &= {"prefix"}           # (whether the total moves too is not asked)
    assert diff == want
    info = raw_exp(fmt, kind)["words"]["events"][1]
    assert total[7:] == (info["untimed"], info["events"], info["other"]) and total[2] == info["wraps"]


@pytest.mark.parametrize("kind", KINDS)
def test_counting_scan_models(kind):
    """AEDAT, text, slicing, the filter, the pick: sums and maxima"""
    c = aedat(kind)
    assert run_variants(*K.aedat_summaries(c), K.LANES["aedat"], K.add, 0, 0) == expected(kind)
    for c in [text(kind)] + ([text(kind, True)] if kind == "2S+1" else []):
        sums, prefix, total, _ = K.text_summaries(c)
        assert total == K.text_expect(c)[0][1]["events"]
        # (the last tile holds one byte of an unfinished line: no line of this call, its summary is the identity)
        assert sums[-1] == 0 and run_variants(sums, prefix, total, K.LANES["text"], K.add, 0, 0) == expected(kind, last_tile_counts=False)
    c = slices(kind)
    assert run_variants(*K.slice_summaries(c), K.LANES["slice"], max, 0, 0) == expected(kind)
    c = pick(kind)
    sums, prefix, total = K.pick_summaries(c)   # (k_voc_scan_top writes prefixes alone: there is no total to take wrongly)
    diff = run_variants(sums, prefix, total, K.LANES["pick"], K.add, 0, 0)
    assert {v: d - {"total"} for v, d in diff.items()} == expected(kind, has_total=False)
    if kind != "2S+1":
        c = filt(kind)
        for refr in (False, True):
            flags = K.filter_expect(c, refr)[0]
            assert run_variants(*K.filter_summaries(c, flags), K.LANES["filter"], K.add, 0, 0) == expected(kind)


# ---- what the inputs contain, per chain ---------------------------------------------------------------------------------------
def lane_of(case, tile):
    return next(t for t, (lo, hi) in enumerate(case["own"]) if lo <= tile < hi)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_raw_inputs(fmt, kind):
    c, e = raw(fmt, kind), raw_exp(fmt, kind)
    w, TW, m = c["words"].astype(np.uint64), c["TW"], c["marks"]
    typ = (w >> np.uint64(12 if fmt == K.EVT3 else 28 if fmt == K.EVT2 else 60)).astype(np.int64)
    th_tiles = sorted(set((np.flatnonzero(typ == 8) // TW).tolist()))
    th_lanes = sorted({lane_of(c, t) for t in th_tiles})
    owners = [t for t, (lo, hi) in enumerate(c["own"]) if hi > lo]
    # whole lanes' runs hold no TIME_HIGH, and the last one lies in an earlier wave than lanes that need it
    assert len(th_lanes) <= 5 and th_lanes[-1] == 101 and owners[-1] // K.WAVE > 101 // K.WAVE
    # the two wraps: one inside a lane's run (where a lane owns more than a tile), one between two lanes' runs
    a, b = m["wrap_inside"]
    assert b == a + 1 and a // TW != b // TW and (lane_of(c, a // TW) == lane_of(c, b // TW)) == (c["per"] > 1)
    a, b = m["wrap_boundary"]
    assert b == a + 1 and lane_of(c, b // TW) == lane_of(c, a // TW) + 1
    for name in ("events", "triggers"):
        info = e["words"][name][1]
        assert info["wraps"] == 2 and info["untimed"] > 0 and info["bad"] == 0   # a fresh state: untimed in front of the first TIME_HIGH
    assert e["words"]["events"][1]["events"] > 1000 and e["words"]["triggers"][1]["triggers"] > 500
    assert m["first_th"] // TW == 1 and typ[-1] in ((2,) if fmt == K.EVT3 else (0, 1))      # the last tile's one word is an event
    # tiles of "other" words alone, a whole lane's run of them
    quiet = np.array([bool((typ[j * TW:(j + 1) * TW] >= 0xB).all()) for j in range(c["tiles"])])
    assert any(hi > lo and quiet[lo:hi].all() for lo, hi in c["own"]) and 0.2 < quiet.mean() < 0.7
    if fmt == K.EVT3:
        base, use = m["vect_base"], m["vect_use"]
        assert lane_of(c, use // TW) >= lane_of(c, base // TW) + 2 and not (typ[base + 1:use] == 3).any()
        rec = e["words"]["events"][0]
        assert ((rec["x"] == 300) & (rec["polarity"] == 1)).any() and ((rec["x"] == 300 + 12 + 9) & (rec["polarity"] == 1)).any()
        assert np.flatnonzero(typ == 3)[-1] == m["late_base"] and m["late_base"] // TW == c["tiles"] - 3   # an open base at the end
    # the follow-up is smaller than a tile, has no setter, and its records are the carried state's
    f = c["follow"].astype(np.uint64)
    ftyp = (f >> np.uint64(12 if fmt == K.EVT3 else 28 if fmt == K.EVT2 else 60)).astype(np.int64)
    assert len(f) < TW and not np.isin(ftyp, (8, 3, 6, 0) if fmt == K.EVT3 else (8,)).any()
    assert e["follow"]["events"][1]["events"] >= 5 and e["follow"]["triggers"][1]["triggers"] == 1
    assert R21.decode(fmt, c["follow"], R21.fresh_state())[1]["events"] == 0
    if fmt == K.EVT3:
        assert {77 + 12, 77 + 12 + 1}.issubset(set(e["follow"]["events"][0]["x"].tolist()))   # bx as the big call left it


def test_the_dense_evt21_case_holds_more_records_than_words():
    c = K.raw_case(K.EVT21, tiles_of("raw", "S+1"), dense=True)
    info = K.raw_expect(c)["words"]["events"][1]
    assert len(c["words"]) < info["events"] < 2 * len(c["words"])   # above the one-record-per-word buffers a call begins with


@pytest.mark.parametrize("kind", KINDS)
def test_aedat_inputs(kind):
    c = aedat(kind)
    sums, _, total = K.aedat_summaries(c)
    S, T_ = K.LANES["aedat"], c["tile"]
    z = "".join("0" if s == 0 else "1" for s in sums)
    assert "1001" in z and "10001" in z and sums.count(T_) > 10 and len(set(sums)) > 50   # runs of 2 and 3 invalid tiles; full ones; shares
    assert any(hi - lo > 1 and sum(sums[lo:hi]) == 0 for lo, hi in c["own"]) or c["per"] == 1   # a lane whose whole run is the identity
    assert sums[-1] == 1
    assert (c["step"] // T_ == S) if kind != "S" else (c["step"] // T_ == S - 2)
    (rec, o), (rec2, o2) = K.aedat_expect(c)
    t = rec["sec"].astype(np.int64) * 10 ** 9 + rec["nsec"]
    assert (np.diff(t) > 2 ** 31 * 1000 - 10 ** 9).sum() == 1 and o["polarity_packets"] >= 6     # the overflow step: a second run
    assert len(rec2) == 4 and o2["invalid"] == 1 and o2["polarity_packets"] == 0                 # the cut record and the packet's rest


@pytest.mark.parametrize("kind,late", [(k, False) for k in KINDS] + [("2S+1", True)])
def test_text_inputs(kind, late):
    c = text(kind, late)
    S, T_ = K.LANES["text"], c["tile"]
    _, _, _, counts = K.text_summaries(c)
    ev, com, blank, mal = counts.T
    assert ((ev > 50) & (com + blank + mal == 0)).sum() > 20 and (com > 100).sum() > 20 and (blank > 100).sum() > 20
    (rec, info, st), (rec2, info2, _) = K.text_expect(c)
    assert info["first_malformed"] == (min(c["marks"]["overlong"] + [c["marks"]["first_bad"]]))
    if kind == "2S+1" and not late:
        a, b = c["marks"]["overlong"]
        assert a + 5 * T_ // 2 < S * T_ and b < S * T_ < b + 5 * T_ // 2 and info["first_malformed"] == a
        for o in (a, b):   # tiles without a line start, inside one lane's run
            j = o // T_ + 1
            assert counts[j].sum() == 0 and any(lo <= j and j + 1 < hi + 1 and hi - lo > 1 for lo, hi in c["own"])
    elif kind == "2S+1":
        assert info["first_malformed"] > S * T_ and info["first_malformed"] == c["marks"]["first_bad"]
    else:
        assert info["first_malformed"] >= (c["tiles"] - 3) * T_
    # the big call ends inside a line; the second call's first line is completed from the tail
    assert 0 < info["carried"] == len(st["tail"]) < 64 and not st["skip"] and info2["carried"] == 0 and info2["lines"] == 4
    alone = T.read(T.fresh(), T.TXYP, T.SEC_DECIMAL, T.SKIP_MALFORMED, c["follow"])[0]
    assert len(rec2) >= 1 and (len(alone) < len(rec2) or alone[0] != tuple(rec2[["x", "y", "sec", "nsec", "polarity"]][0].tolist()))


@pytest.mark.parametrize("kind", KINDS)
def test_slice_inputs(kind):
    c = slices(kind)
    S, T_ = K.LANES["slice"], c["tile"]
    sums, prefix, total = K.slice_summaries(c)
    assert total == len(c["closes"]) <= 8 and max(np.diff(c["closes"])) > 100 * T_     # windows close rarely
    if kind != "S":
        assert S * T_ - 1 in c["closes"] and S * T_ in c["closes"]   # the last event of tile S - 1, the first of tile S
    assert c["closes"][-1] == len(c["ev"]) - 1                       # ... and the stream's last event, alone in its tile
    a, b = c["back"]
    assert (b - 1) // T_ - a // T_ == 1 and (lane_of(c, a // T_) == lane_of(c, (b - 1) // T_)) == (c["per"] > 1)
    j = a // T_ + 1
    assert sums[j] == prefix[j] - 3 > 0                              # a tile whose own maximum lies three windows below the prefix
    for at in (False, True):
        (cuts, info, _), (cuts2, info2, b2) = K.slice_expect(c, at)
        assert cuts == c["closes"] and info["closed"] == total and info2["first_window"] == total and info2["closed"] == 2
        assert cuts2 == [100, 200] and (not at or len(b2) == len(c["bounds"]) - total)


@pytest.mark.parametrize("kind", ("S", "S+1"))
def test_filter_inputs(kind):
    c = filt(kind)
    on, off = K.filter_expect(c, True), K.filter_expect(c, False)
    for flags, rej, B in (on, off):
        sums, _, total = K.filter_summaries(c, flags)
        assert sums.count(0) > 50 and sums.count(c["tile"]) > 50 and len(set(sums)) > 20 and sums[-1] == 1 and rej > 1000
    assert int(on[0].sum()) < int(off[0].sum()) - 50_000 and not np.array_equal(on[2], F2.fresh_plane(K.FILTER_W, K.FILTER_H))


@pytest.mark.parametrize("kind", KINDS)
def test_pick_inputs(kind):
    c = pick(kind)
    S, T_, B = K.LANES["pick"], c["tile"], c["B"]
    sums, prefix, total = K.pick_summaries(c)
    assert B == c["own"][S // 2][0] * T_ and c["own"][S // 2 - 1][1] * T_ == B     # where lane S/2's tiles begin
    assert sums[B // T_ - 1] == 0 and sums[B // T_] == 0 and total > 1 << 32 and int(c["md"].max()) > 1 << 20
    seg = list(zip(c["seg_off"].tolist(), c["seg_off"].tolist()[1:]))
    assert any(b < B for a, b in seg) and any(a < b == B for a, b in seg) and any(a == b == B for a, b in seg)
    assert any(a <= B < b for a, b in seg) and c["seg_off"][-1] == c["n"]
    assert (np.diff(c["seg_off"].astype(np.int64)) >= 0).all()


# ---- the vectorised filter restatement -------------------------------------------------------------------------------------------
def test_filter_fast_equals_the_loop():
    """over the filter stage's existing designed cases and a few thousand random events more, with and without the
    support and refractory tests, across two calls on one plane: flags, the rejected count and the plane, bit for bit"""
    rng = np.random.default_rng(8)
    batches = []
    for name in sorted(BK.HAND):
        batches.append((BK.W, BK.H, BK.hand_case(name)[0]))
    batches += [(BK.W, BK.H, BK.sweep_events(n)) for n in BK.SWEEP_SIZES] + [(BK.W, BK.H, BK.hot_pixel_events(1500))]
    for W, H, n, span in ((64, 48, 3000, 20_000), (16, 12, 4000, 3_000), (7, 5, 2500, 500)):
        batches.append((W, H, BK.uniform_events(n, W, H, span, seed=n)))
    ev = np.zeros(5000, K.EVENT_DTYPE)
    ev["x"], ev["y"] = rng.integers(0, 70, 5000), rng.integers(0, 50, 5000)          # some outside 64 x 48
    t = 10 ** 9 + np.cumsum(rng.integers(-2000, 9000, 5000))                            # stamps that step back
    ev["sec"], ev["nsec"], ev["polarity"] = t // 10 ** 9, t % 10 ** 9, rng.integers(0, 2, 5000)
    batches.append((64, 48, ev))
    batches.append((K.FILTER_W, K.FILTER_H, K.filter_case(9)["ev"]))
    for W, H, ev in batches:
        for window, support, refr in ((1_000_000, 1, 0), (50_000, 2, 0), (1_000_000, 1, 5_000), (0, 0, 30_000), (3_000_000, 8, 1)):
            Ba, Bb = F2.fresh_plane(W, H), F2.fresh_plane(W, H)
            for part in (ev[:len(ev) // 2], ev[len(ev) // 2:], ev[:0]):
                fa, ra = F2.filter_events(Ba, W, H, part, window, support, refr)
                fb, rb = K.filter_fast(Bb, W, H, part, window, support, refr)
                assert np.array_equal(fa, fb) and ra == rb and np.array_equal(Ba, Bb), (W, H, window, support, refr)
