"""Inputs for the shared stable radix sort (k_radix_pass through radix_sort_pairs), held to it alone through the tap
esvio_fe_sort_pairs: digit widths, tile and wave edges, padding, bits above the sorted range, digit distributions,
look-back chains and the device-side count.  Seeded numpy; no device code.

  CASES          name -> function returning a Case (keys, vals, passes, bits, n_dev); n_dev None: no device count
  EDGES          name -> function asserting, from the arrays alone, that the case reaches the edge its name claims
  reference      numpy.argsort(keys & mask, kind="stable") applied to keys and vals; whole keys come back
  pass_model     ONE pass as the kernel does it (per wave and round match-any ranks, wave bases, tile counts, the
                 exclusive prefix over earlier tiles by look-back, the global digit base), and wrong variants of it
  model          pass_model chained over the passes, with the digit histograms the tap counts

The geometry is the kernel's: a block owns a tile of 2048 consecutive pairs, each of its 4 waves 512 consecutive pairs
of it in 8 rounds of 64 lanes.
"""
import collections

import numpy as np

TILE, WAVES, ROUNDS, LANES = 2048, 4, 8, 64
WAVE_KEYS = ROUNDS * LANES
assert WAVES * WAVE_KEYS == TILE
PAD_KEY = 0xffffffff                         # what a padding lane of a partial tile loads
FILL_KEY, FILL_VAL = 0x5eedf00d, 0x0badc0de  # what the tap's second buffer of each pair starts as

Case = collections.namedtuple("Case", "keys vals passes bits n_dev")


def blocks(n):
    return (n + TILE - 1) // TILE


def driver_shape(key_bits):
    """(passes, bits) as the SAE sort path and the event filter derive them (fe_stages.cpp sae_update_planes, fe_api.cpp)"""
    passes = (key_bits + 6) // 7
    return passes, (key_bits + passes - 1) // passes


# key_bits 1..28 -> (passes, bits): the table the formula gives, written out; the other drivers use 8 bits
DRIVER_PAIRS = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (1, 4), 5: (1, 5), 6: (1, 6), 7: (1, 7), 8: (2, 4), 9: (2, 5), 10: (2, 5),
                11: (2, 6), 12: (2, 6), 13: (2, 7), 14: (2, 7), 15: (3, 5), 16: (3, 6), 17: (3, 6), 18: (3, 6), 19: (3, 7),
                20: (3, 7), 21: (3, 7), 22: (4, 6), 23: (4, 6), 24: (4, 6), 25: (4, 7), 26: (4, 7), 27: (4, 7), 28: (4, 7)}

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)
SIZE_SHAPES = ((1, 8), (3, 7))
N3 = 3 * TILE + 1   # three tiles plus one pair


# ---- the reference ---------------------------------------------------------------------------------------------------------
def taking_part(case):
    n = len(case.keys)
    return n if case.n_dev is None else min(n, case.n_dev)


def reference(case):
    """-> (keys, vals) the tap must return: the pairs that take part in stable order of their low passes * bits bits; at
    and beyond a device count what the result buffer held before — the fill behind an odd number of passes (the second
    buffer), the input pairs where they lay behind an even one (the first)"""
    m = taking_part(case)
    mask = np.uint32((1 << (case.passes * case.bits)) - 1)
    order = np.argsort(case.keys[:m] & mask, kind="stable")
    ok, ov = tap_buffers(case)[case.passes % 2]
    ok[:m], ov[:m] = case.keys[:m][order], case.vals[:m][order]
    return ok, ov


def tickets(case):
    """the blocks each pass launches: every one takes a ticket, the ones behind a device count too"""
    return np.full(case.passes, blocks(len(case.keys)), np.uint32)


def pass_inputs(case):
    """the keys that take part, in the order each pass reads them: [passes] arrays"""
    m = taking_part(case)
    k, out = case.keys[:m], []
    for p in range(case.passes):
        out.append(k)
        k = k[np.argsort((k >> np.uint32(p * case.bits)) & np.uint32((1 << case.bits) - 1), kind="stable")]
    return out


def digits(keys, p, bits):
    return ((keys >> np.uint32(p * bits)) & np.uint32((1 << bits) - 1)).astype(np.int64)


# ---- one pass as the kernel does it ----------------------------------------------------------------------------------------
VARIANTS = ("padding_placed", "reverse_lanes", "waves_reversed", "aggregate_as_prefix", "match_high_bits", "n_dev_ignored")
# a seventh, which the sort's outputs cannot show (test_sort_cases.py says why): the ballot of valid lanes alone dropped
BLIND_VARIANT = "padding_in_ballot"
_LOWER = np.tril(np.ones((LANES, LANES), bool), -1)   # [i, j]: lane j lies below lane i


def pass_model(src, dst, shift, bits, ghist, n_dev=None, variant=None, published="aggregate"):
    """One stable pass from the buffers src = (keys, vals) into copies of dst = (keys, vals), n pairs each ->
    (keys_out, vals_out, outside).  `outside`: positions at or beyond n a pair was sent to (nothing is written there: the
    model's report of a kernel that would write out of bounds).  published: the state an earlier tile's look-back word is
    found in — "aggregate" (every earlier tile has only published its own counts: the walk goes back to tile 0) or
    "prefix" (every earlier tile is through: the walk stops at once); both are legal and must give the same result."""
    bins = 1 << bits
    keys_in, vals_in = src
    n = len(keys_in)
    m = n if n_dev is None or variant == "n_dev_ignored" else min(n, n_dev)
    keys_out, vals_out = dst[0].copy(), dst[1].copy()
    outside = []
    digit_base = np.concatenate([[0], np.cumsum(ghist[:bins])[:-1]]).astype(np.int64)  # exclusive scan of the global totals
    counts = []   # per tile taken: its per-digit counts, as published
    prefixes = []  # ... and the inclusive prefix it publishes behind its walk
    for tile in range(blocks(n)):
        if n_dev is not None and variant != "n_dev_ignored" and tile * TILE >= m:
            continue   # (tickets go in order: the tiles that hold pairs are 0 .. and nobody looks back at a later one)
        idx = tile * TILE + np.arange(TILE).reshape(WAVES, ROUNDS, LANES)
        ok = idx < m
        key = np.where(ok, keys_in[np.minimum(idx, n - 1)], np.uint32(PAD_KEY)).astype(np.uint32)
        val = np.where(ok, vals_in[np.minimum(idx, n - 1)], np.uint32(0)).astype(np.uint32)
        d = ((key >> np.uint32(shift)) & np.uint32(bins - 1)).astype(np.int64)
        part = np.ones_like(ok) if variant in ("padding_placed", BLIND_VARIANT) else ok   # lanes in the match-any ballot
        placed = np.ones_like(ok) if variant == "padding_placed" else ok                   # lanes ranked, counted, placed
        grp = (key >> np.uint32(shift)).astype(np.int64) if variant == "match_high_bits" else d
        same = (grp[..., :, None] == grp[..., None, :]) & part[..., None, :]               # [w, r, i, j]: j matches i
        below = _LOWER.T if variant == "reverse_lanes" else _LOWER
        before = (same & below).sum(-1)
        cnt = same.sum(-1)
        wave_cnt = np.zeros((WAVES, 256), np.int64)
        rank = np.zeros((WAVES, ROUNDS, LANES), np.int64)
        for w in range(WAVES):
            for r in range(ROUNDS):
                p = placed[w, r]
                base = np.where(p, wave_cnt[w, d[w, r]], 0)
                rank[w, r] = base + before[w, r]
                lead = p & (before[w, r] == 0)   # one leader per digit
                wave_cnt[w, d[w, r][lead]] = (base + cnt[w, r])[lead]
        cnt_tile = wave_cnt[:, :bins].sum(0)
        # decoupled look-back: the exclusive prefix over the earlier tiles
        if not counts:
            excl = np.zeros(bins, np.int64)
        elif published == "prefix":
            excl = prefixes[-1].copy()
        elif variant == "aggregate_as_prefix":
            excl = counts[-1].copy()   # the walk stops at the first word it finds, whatever its status
        else:
            excl = np.sum(counts, axis=0)
        counts.append(cnt_tile)
        prefixes.append(excl + cnt_tile)
        run = digit_base + excl
        wave_base = np.zeros((WAVES, bins), np.int64)
        for w in (range(WAVES - 1, -1, -1) if variant == "waves_reversed" else range(WAVES)):
            wave_base[w] = run
            run = run + wave_cnt[w, :bins]
        pos = wave_base[np.arange(WAVES)[:, None, None], d] + rank
        pos, kk, vv = pos[placed], key[placed], val[placed]
        inside = (pos >= 0) & (pos < n)
        outside.extend(pos[~inside].tolist())
        keys_out[pos[inside]], vals_out[pos[inside]] = kk[inside], vv[inside]
    return keys_out, vals_out, outside


def tap_buffers(case):
    """the two device buffers as the tap fills them, [(keys, vals)] * 2: the whole input, the fill"""
    n = len(case.keys)
    return [(case.keys.copy(), case.vals.copy()), (np.full(n, FILL_KEY, np.uint32), np.full(n, FILL_VAL, np.uint32))]


def host_histograms(case):
    """ghist[p][d] of the pairs that take part, as the tap counts them"""
    m = taking_part(case)
    return [np.bincount(digits(case.keys[:m], p, case.bits), minlength=1 << case.bits) for p in range(case.passes)]


def model(case, variant=None, published="aggregate"):
    """the passes chained, to and fro between the two buffers of tap_buffers -> (keys, vals, outside)"""
    (cur, other), hist, outside = tap_buffers(case), host_histograms(case), []
    for p in range(case.passes):
        k, v, out = pass_model(cur, other, p * case.bits, case.bits, hist[p], case.n_dev, variant, published)
        other, cur = cur, (k, v)
        outside += out
    return cur[0], cur[1], outside


# ---- the cases -------------------------------------------------------------------------------------------------------------
CASES, EDGES = {}, {}


def _rng(name):
    return np.random.default_rng(np.frombuffer(name.encode().ljust(32, b"\0")[:32], np.uint32))


def _add(name, make, edge):
    assert name not in CASES, name
    CASES[name] = lambda: make(_rng(name))
    EDGES[name] = edge


def _case(keys, vals, passes, bits, n_dev=None):
    keys, vals = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(vals, np.uint32)
    assert keys.shape == vals.shape and keys.ndim == 1
    return Case(keys, vals, passes, bits, n_dev)


def _random32(r, n):
    return r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _index(n):
    return np.arange(n, dtype=np.uint32)


def tile_digit_counts(case, p=0):
    """[tiles, bins]: how many keys of each digit every tile of pass p holds"""
    k = pass_inputs(case)[p]
    d, t = digits(k, p, case.bits), np.arange(len(k)) // TILE
    out = np.zeros((blocks(len(k)), 1 << case.bits), np.int64)
    np.add.at(out, (t, d), 1)
    return out


def round_digits(case, p=0):
    """the digits of pass p's full 64-lane rounds: [rounds, 64]"""
    k = pass_inputs(case)[p]
    full = len(k) // LANES * LANES
    return digits(k[:full], p, case.bits).reshape(-1, LANES)


# sizes: random 32-bit keys, the index as value
def _edge_size(n):
    def edge(c):
        assert len(c.keys) == n and c.n_dev is None and np.array_equal(c.vals, _index(n))
        assert blocks(n) == (1 if n <= TILE else 2 if n <= 2 * TILE else 3)
    return edge


for _p, _b in SIZE_SHAPES:
    for _n in SIZES:
        _add("size_%d_%dx%d" % (_n, _p, _b), lambda r, n=_n, p=_p, b=_b: _case(_random32(r, n), _index(n), p, b), _edge_size(_n))


# widths: every bits with one pass; every (passes, bits) the drivers derive; 4 x 8 on full keys
def _edge_width(passes, bits):
    def edge(c):
        assert (c.passes, c.bits) == (passes, bits) and blocks(len(c.keys)) == 3 and len(c.keys) % TILE
        for p in range(passes):   # every digit value of every pass occurs
            assert len(np.unique(digits(c.keys, p, bits))) == 1 << bits
    return edge


for _b in range(1, 9):
    _add("width_1x%d" % _b, lambda r, b=_b: _case(_random32(r, 2 * TILE + 77), _index(2 * TILE + 77), 1, b), _edge_width(1, _b))
for _kb in (8, 10, 12, 14, 15, 18, 21, 24, 28):   # the largest key_bits of every multi-pass pair of DRIVER_PAIRS
    _p, _b = DRIVER_PAIRS[_kb]
    _add("driver_kb%d_%dx%d" % (_kb, _p, _b),
         lambda r, kb=_kb, p=_p, b=_b: _case(r.integers(0, 1 << kb, 2 * TILE + 77, dtype=np.uint64), _index(2 * TILE + 77), p, b),
         _edge_width(_p, _b))
_add("full32_4x8", lambda r: _case(_random32(r, 2 * TILE + 77), _random32(r, 2 * TILE + 77), 4, 8), _edge_width(4, 8))


# digit shapes, at three tiles plus one pair
def _spread(r, d, p, b):
    """keys whose pass-0 digits are d; the digits of the other passes and the bits above random"""
    hi = _random32(r, len(d)) & np.uint32(~((1 << b) - 1) & 0xffffffff)
    return hi | np.asarray(d, np.uint32)


def _edge_all_equal(c):
    t = tile_digit_counts(c)
    assert len(np.unique(c.keys)) == 1 and len(c.keys) == N3
    assert t.max() == TILE and (t.max(1)[:3] == TILE).all()   # a tile's count reaches 2048, a wave's ranks run to 511


def _edge_two(c):
    d = round_digits(c)
    assert (np.sort(np.unique(d)) == np.unique(d[0])).all() and len(np.unique(d[0])) == 2
    assert (d[:, 0::2] == d[0, 0]).all() and (d[:, 1::2] == d[0, 1]).all()   # they alternate lane by lane


def _edge_extremes(c):
    for p in range(c.passes):
        assert set(np.unique(digits(c.keys, p, c.bits))) == {0, (1 << c.bits) - 1}


def _edge_rounds_distinct(c):
    assert c.bits >= 6
    d = round_digits(c)
    assert (np.sort(d, axis=1)[:, 1:] != np.sort(d, axis=1)[:, :-1]).all()   # every round of pass 0: every lane a leader
    assert len(np.unique(d)) == 1 << c.bits                                  # ... and every digit value is used


def _edge_ascending(c):   # already in order (equal keys side by side: one pass of 8 bits has 256 values for 6145 pairs)
    s = c.keys.astype(np.int64)
    assert (np.diff(s) >= 0).all() and s[0] < s[-1] and s[-1] >> (c.passes * c.bits) == 0


def _edge_descending(c):  # the order reversed, but not inside a run of equal keys
    s = c.keys.astype(np.int64)
    assert (np.diff(s) <= 0).all() and s[0] > s[-1] and s[0] >> (c.passes * c.bits) == 0 and (np.diff(s) == 0).any()


def _edge_absent(c):
    t = tile_digit_counts(c)
    gone = np.flatnonzero((t[:-1] == 0).all(0) & (t[-1] > 0))
    assert len(gone) == 1 and 0 < gone[0] < (1 << c.bits) - 1   # (not an end of the range: digits lie behind it)
    assert (t[:, gone[0] + 1:].sum(1)[:-1] > 0).all()


def _make_rounds_distinct(r, p, b):
    rounds = -(-N3 // LANES)
    d = np.concatenate([(r.permutation(1 << b)[:LANES] if b > 6 else r.permutation(LANES)) for _ in range(rounds)])[:N3]
    # (b > 6: a different 64 of the digit values each round, so every value occurs somewhere)
    return _case(_spread(r, d, p, b), _index(N3), p, b)


def _make_absent(r, p, b):
    bins = 1 << b
    gone = bins // 2
    d = r.integers(0, bins - 1, N3)
    d = np.where(d >= gone, d + 1, d)
    d[-1] = gone
    return _case(_spread(r, d, p, b), _index(N3), p, b)


for _p, _b in ((1, 8), (3, 7)):
    _s = "_%dx%d" % (_p, _b)
    _add("all_equal" + _s, lambda r, p=_p, b=_b: _case(np.full(N3, 0x1234abcd, np.uint32), _index(N3), p, b), _edge_all_equal)
    _add("two_alternating" + _s, lambda r, p=_p, b=_b: _case(_spread(r, np.where(np.arange(N3) % 2, 5, (1 << b) - 3), p, b), _index(N3), p, b),
         _edge_two)
    _add("extremes" + _s, lambda r, p=_p, b=_b: _case(np.where(r.integers(0, 2, (p, N3)).astype(bool), (1 << b) - 1, 0).astype(np.uint32).T
                                                      @ (1 << (b * np.arange(p))).astype(np.uint32), _index(N3), p, b), _edge_extremes)
    _add("rounds_distinct" + _s, lambda r, p=_p, b=_b: _make_rounds_distinct(r, p, b), _edge_rounds_distinct)
    _add("ascending" + _s, lambda r, p=_p, b=_b: _case(np.sort(r.integers(0, 1 << (p * b), N3)), _index(N3), p, b), _edge_ascending)
    _add("descending" + _s, lambda r, p=_p, b=_b: _case(np.sort(r.integers(0, 1 << (p * b), N3))[::-1], _index(N3), p, b), _edge_descending)
    _add("absent_until_last" + _s, lambda r, p=_p, b=_b: _make_absent(r, p, b), _edge_absent)
_add("rounds_distinct_1x6", lambda r: _make_rounds_distinct(r, 1, 6), _edge_rounds_distinct)
_add("rounds_distinct_1x7", lambda r: _make_rounds_distinct(r, 1, 7), _edge_rounds_distinct)


# padding: a partial last tile whose real keys include 0xffffffff; 0xffffffff as every key
N_PART = TILE + 700   # the last tile: 700 pairs, ending inside wave 1's round 2


def _edge_ff_some(c):
    k = c.keys
    assert len(k) == N_PART and k[-1] == PAD_KEY and (k[TILE:] == PAD_KEY).sum() > 10 and (k[TILE:] != PAD_KEY).sum() > 100
    last_round = k[len(k) // LANES * LANES:]   # real 0xffffffff keys and padding lanes in one 64-lane round
    assert 0 < len(last_round) < LANES and (last_round == PAD_KEY).any() and (last_round != PAD_KEY).any()
    assert (k[:TILE] == PAD_KEY).any()


def _edge_ff_all(c):
    assert len(c.keys) == N_PART and (c.keys == PAD_KEY).all() and len(np.unique(c.vals)) == len(c.vals)


def _make_ff_some(r, p, b):
    k = _random32(r, N_PART)
    k[r.random(N_PART) < 0.1] = PAD_KEY
    k[-1] = PAD_KEY
    k[-2] = 0x7fffffff
    return _case(k, _index(N_PART), p, b)


for _p, _b in ((4, 8), (3, 7)):
    _s = "_%dx%d" % (_p, _b)
    _add("partial_ff_some" + _s, lambda r, p=_p, b=_b: _make_ff_some(r, p, b), _edge_ff_some)
    _add("partial_ff_all" + _s, lambda r, p=_p, b=_b: _case(np.full(N_PART, PAD_KEY, np.uint32), _index(N_PART)[::-1], p, b), _edge_ff_all)


# bits above the sorted range: random there, heavy duplicates below
def _edge_high_bits(index_vals):
    def edge(c):
        sorted_bits = c.passes * c.bits
        assert sorted_bits < 32 and len(np.unique(c.keys >> np.uint32(sorted_bits))) > len(c.keys) // 2
        low = c.keys & np.uint32((1 << sorted_bits) - 1)
        assert len(np.unique(low)) <= 4 and np.bincount(low).max() > len(c.keys) // 8
        hi_sorted = reference(c)[0] >> np.uint32(sorted_bits)
        assert (np.diff(hi_sorted.astype(np.int64)) < 0).sum() > len(c.keys) // 4   # sorting whole keys would differ
        assert np.array_equal(c.vals, _index(len(c.keys))) == index_vals
    return edge


def _make_high(r, p, b, index_vals):
    low = r.choice(r.choice(1 << (p * b), 4, replace=False), N3).astype(np.uint32)
    k = (_random32(r, N3) << np.uint32(p * b)) | low
    return _case(k, _index(N3) if index_vals else _random32(r, N3), p, b)


for _p, _b in ((1, 8), (2, 5), (3, 6)):   # 24, 22 and 14 bits above
    _s = "_%dx%d" % (_p, _b)
    _add("high_bits_dups" + _s, lambda r, p=_p, b=_b: _make_high(r, p, b, True), _edge_high_bits(True))
    _add("high_bits_random_vals" + _s, lambda r, p=_p, b=_b: _make_high(r, p, b, False), _edge_high_bits(False))


# look-back
def _edge_lookback41(c):
    t = tile_digit_counts(c)
    assert t.shape[0] == 41 and len(c.keys) == 41 * TILE
    held = np.flatnonzero((t[0] > 0) & (t[-1] > 0) & (t[1:-1] == 0).all(0))
    assert len(held) == 1 and t[0, held[0]] > 100 and t[-1, held[0]] > 100   # its walk goes back all 40 tiles


def _make_lookback41(r):
    n = 41 * TILE
    d = r.integers(0, 255, n)
    d = np.where(d >= 7, d + 1, d)   # digit 7 nowhere ...
    for lo in (0, 40 * TILE):        # ... but in tile 0 and the last tile
        at = lo + r.choice(TILE, 300, replace=False)
        d[at] = 7
    return _case(_spread(r, d, 1, 8), _index(n), 1, 8)


def _edge_lookback300(c):
    assert len(c.keys) == 300 * TILE + 1 and (c.passes, c.bits) == (4, 8) and blocks(len(c.keys)) == 301 > 256   # more tiles than CUs


_add("lookback_41_tiles_1x8", _make_lookback41, _edge_lookback41)
_add("lookback_300_tiles_4x8", lambda r: _case(_random32(r, 300 * TILE + 1), _random32(r, 300 * TILE + 1), 4, 8), _edge_lookback300)


# the device-side count, the launch sized for three tiles plus one pair
def _edge_n_dev(n_dev):
    def edge(c):
        assert len(c.keys) == N3 and c.n_dev == n_dev and blocks(N3) == 4
        assert taking_part(c) == min(n_dev, N3)
        ok, ov = reference(c)
        if c.passes % 2:
            assert (ok[taking_part(c):] == FILL_KEY).all() and (ov[taking_part(c):] == FILL_VAL).all()
        else:
            assert np.array_equal(ok[taking_part(c):], c.keys[taking_part(c):]) and np.array_equal(ov[taking_part(c):], c.vals[taking_part(c):])
        assert not (c.keys == FILL_KEY).any() and not (c.vals == FILL_VAL).any()   # a written position cannot look unwritten
    return edge


for _p, _b in ((1, 8), (3, 7), (2, 6)):
    for _nd in (0, 1, TILE, TILE + 1, N3, N3 + 5):
        _add("n_dev_%d_%dx%d" % (_nd, _p, _b), lambda r, p=_p, b=_b, nd=_nd: _case(_random32(r, N3) | np.uint32(1 << 31), _index(N3), p, b, nd),
             _edge_n_dev(_nd))

NAMES = tuple(CASES)
LARGEST = "lookback_300_tiles_4x8"
