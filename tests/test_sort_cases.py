"""CPU: the inputs of tests/sort_cases.py are what their names claim, a numpy model of one k_radix_pass — per wave and
round match-any ranks, wave bases, tile counts, the look-back's exclusive prefix, the global digit base — chained over
the passes reproduces the argsort reference on every one of them, and six wrong variants of it do not: the evidence that
tests/test_sort_gpu.py, which runs the same cases through esvio_fe_sort_pairs, would notice a subtly wrong kernel."""
import numpy as np
import pytest

import sort_cases as K
from esvio_amd import frontend as FE


@pytest.fixture(scope="module")
def memo():
    """a case and its reference, computed once per module and handed out read-only"""
    store = {}

    def get(name):
        if name not in store:
            c = K.CASES[name]()
            ref = K.reference(c)
            for a in (c.keys, c.vals) + ref:
                a.setflags(write=False)
            store[name] = (c, ref)
        return store[name]
    return get


def same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and not got[2]


def test_tap_is_declared_and_refuses_no_handle():
    L = FE.load_library()
    assert "esvio_fe_sort_pairs" in FE.TEST_SYMBOLS and hasattr(L, "esvio_fe_sort_pairs")
    assert L.esvio_fe_sort_pairs(None, None, None, 0, 1, 8, -1, None, None, None, None) == -1


def test_driver_pairs_are_the_formula():
    """the table written out in sort_cases.py is what the drivers' formula gives for key_bits 1..28, its widths are 1..7,
    and every pair of it is run: the single-pass ones by width_1x*, the others by driver_kb*"""
    assert K.DRIVER_PAIRS == {kb: K.driver_shape(kb) for kb in range(1, 29)}
    assert {b for _, b in K.DRIVER_PAIRS.values()} == set(range(1, 8))
    run = {(K.CASES[n]().passes, K.CASES[n]().bits) for n in K.NAMES if n.startswith(("width_", "driver_", "full32"))}
    assert set(K.DRIVER_PAIRS.values()) <= run and {(1, 8), (4, 8)} <= run
    for p, b in set(K.DRIVER_PAIRS.values()):
        assert 1 <= p <= 4 and p * b <= 32


def test_the_case_list_covers_what_it_must():
    sizes = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)
    for p, b in ((1, 8), (3, 7)):
        for n in sizes:
            assert "size_%d_%dx%d" % (n, p, b) in K.CASES
        for nd in (0, 1, 2048, 2049, K.N3, K.N3 + 5):
            assert "n_dev_%d_%dx%d" % (nd, p, b) in K.CASES
    assert K.N3 == 3 * 2048 + 1 and K.WAVE_KEYS == 512
    assert max(len(K.CASES[n]().keys) for n in K.NAMES if n != K.LARGEST) < len(K.CASES[K.LARGEST]().keys) == 300 * 2048 + 1
    assert set(K.CASES) == set(K.EDGES)


@pytest.mark.parametrize("name", K.NAMES)
def test_case_reaches_its_edge(name, memo):
    c, ref = memo(name)
    assert c.keys.dtype == c.vals.dtype == np.uint32 and 1 <= c.bits <= 8 and 1 <= c.passes <= 4 and 0 < len(c.keys) < 1 << 30
    K.EDGES[name](c)
    # the reference is a permutation of the pairs that take part, ordered by the sorted bits alone, stable
    m, mask = K.taking_part(c), np.uint32((1 << (c.passes * c.bits)) - 1)
    low = (ref[0][:m] & mask).astype(np.int64)
    assert (np.diff(low) >= 0).all()
    pairs_in = np.sort(c.keys[:m].astype(np.uint64) << np.uint64(32) | c.vals[:m])
    assert np.array_equal(np.sort(ref[0][:m].astype(np.uint64) << np.uint64(32) | ref[1][:m]), pairs_in)
    if np.array_equal(c.vals, np.arange(len(c.vals))):   # the index as value: equal keys keep their order
        assert (np.diff(ref[1][:m].astype(np.int64))[np.diff(low) == 0] > 0).all()


@pytest.mark.parametrize("name", K.NAMES)
def test_model_reproduces_the_reference(name, memo):
    """whichever state the earlier tiles' look-back words are found in, and without a position outside the buffers"""
    c, ref = memo(name)
    assert same(K.model(c), ref)
    if name != K.LARGEST:   # (the second legal interleaving takes the walk out of the model: not worth 1200 tiles more)
        assert same(K.model(c, published="prefix"), ref)


# variant -> the named cases that must show it (each designed for it), and cases that cannot (why, in words)
KILLED_BY = {
    # padding lanes ranked, counted and placed like pairs: their 0xffffffff keys land behind the real ones of the top digit
    "padding_placed": ("size_1_1x8", "size_2049_3x7", "partial_ff_some_4x8", "partial_ff_all_3x7", "n_dev_1_1x8", "n_dev_2049_3x7",
                       "n_dev_2049_2x6"),
    # ranks inside a round from the highest lane down: equal digits of one round come out reversed
    "reverse_lanes": ("size_512_1x8", "all_equal_1x8", "two_alternating_3x7", "extremes_1x8", "high_bits_dups_2x5", "partial_ff_all_3x7",
                      "descending_1x8"),
    # wave 3's pairs in front of wave 0's: equal digits in two waves of a tile change places
    "waves_reversed": ("size_513_1x8", "size_2048_3x7", "all_equal_3x7", "rounds_distinct_1x6", "partial_ff_all_4x8", "ascending_1x8"),
    # the walk stops at the first earlier tile's counts: a digit's pairs two tiles back are not counted
    "aggregate_as_prefix": ("size_4097_1x8", "all_equal_1x8", "lookback_41_tiles_1x8", "absent_until_last_3x7", "n_dev_6145_1x8"),
    # the match-any goes on over the bits above the digit: equal digits with different bits above take the same rank
    "match_high_bits": ("high_bits_dups_1x8", "high_bits_dups_2x5", "high_bits_random_vals_3x6", "full32_4x8", "width_1x1",
                        "partial_ff_some_3x7"),
    # the launch's bound taken for the count: the pairs behind the device count are sorted in
    "n_dev_ignored": ("n_dev_0_1x8", "n_dev_1_3x7", "n_dev_2048_1x8", "n_dev_2049_3x7", "n_dev_0_2x6", "n_dev_2049_2x6"),
}
SURVIVES = {
    "padding_placed": ("size_2048_1x8", "size_4096_3x7", "n_dev_2048_1x8", "n_dev_0_3x7"),   # no padding lane, or no block at work
    "reverse_lanes": ("rounds_distinct_1x6", "rounds_distinct_1x7", "rounds_distinct_1x8", "size_1_1x8"),   # every lane a leader
    "waves_reversed": ("size_512_1x8", "size_511_3x7"),                                  # one wave holds every pair
    "aggregate_as_prefix": ("size_4096_1x8", "size_4096_3x7", "n_dev_2049_1x8"),         # two tiles: the first word IS a prefix
    "match_high_bits": ("all_equal_1x8", "all_equal_3x7", "partial_ff_all_4x8"),         # equal digits, equal bits above
    "n_dev_ignored": ("n_dev_6145_1x8", "n_dev_6150_3x7", "size_4097_1x8"),              # the count is the bound, or there is none
}


def test_the_table_names_every_variant():
    assert set(KILLED_BY) == set(K.VARIANTS) == set(SURVIVES)
    for v in K.VARIANTS:
        assert set(KILLED_BY[v]) <= set(K.CASES) and set(SURVIVES[v]) <= set(K.CASES) and not set(KILLED_BY[v]) & set(SURVIVES[v])


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_wrong_variant_differs_where_the_table_says(variant, memo):
    for name in KILLED_BY[variant]:
        c, ref = memo(name)
        assert not same(K.model(c, variant), ref), name
    for name in SURVIVES[variant]:
        c, ref = memo(name)
        assert same(K.model(c, variant), ref), name


def test_every_variant_is_seen_by_most_of_the_net(memo):
    """beyond the named cases: how many of the cases (the largest aside) each variant fails — a floor per variant, so that
    a change of the inputs that blunts the net shows here"""
    floor = {"padding_placed": 60, "reverse_lanes": 60, "waves_reversed": 50, "aggregate_as_prefix": 30, "match_high_bits": 50,
             "n_dev_ignored": 12}
    for variant in K.VARIANTS:
        killed = sum(not same(K.model(c, variant), ref) for c, ref in (memo(n) for n in K.NAMES if n != K.LARGEST))
        print(variant, killed)
        assert killed >= floor[variant], (variant, killed)


def test_padding_in_the_ballot_alone_cannot_show(memo):
    """Dropping ballot(ok) from the match-any, with the padding lanes still neither ranked nor placed, changes no output of
    the sort: padding lanes lie behind every pair of their tile, in the last tile at work, so what they inflate — the count
    the last real 0xffffffff-digit leader leaves in its wave's counter, the last tile's published count of the top digit —
    is read by no pair.  The model agrees on every case; only `padding_placed`, where the lanes are placed too, shows."""
    for name in K.NAMES:
        if name != K.LARGEST:
            c, ref = memo(name)
            assert same(K.model(c, K.BLIND_VARIANT), ref), name


def test_model_reports_positions_outside(memo):
    """a kernel that placed its padding lanes would write behind the buffers' end in a call without a device count: the
    model reports those positions instead of writing them, and the correct pass has none"""
    c, ref = memo("partial_ff_some_4x8")
    assert K.model(c)[2] == []
    outside = K.model(c, "padding_placed")[2]
    assert len(outside) == c.passes * (2 * K.TILE - len(c.keys)) and min(outside) == len(c.keys)
