"""CPU: the designed inputs of tests/gftt_cases.py reach the edges of goodFeaturesToTrack they are named for — negative
responses, exactly-zero maps, the image border, candidate counts around the sort's and the lists' block sizes, a
threshold that equals a candidate bit for bit, tie groups over many rows, masks that move the threshold or leave
nothing — and the oracle's corners on them are what the module's own numpy restatement of the rules gives.  No device
involved; tests/test_gftt_edges_gpu.py runs the same cases through the kernels.

Why the cases exist: the inputs of test_good_features_to_track_matches_oracle (tests/test_parity_gpu.py) never return
two corners with one response, which the last test here records."""
import numpy as np
import pytest

import gftt_cases as GC


@pytest.fixture(scope="module")
def eig_of(oracle):
    """the oracle's response map of an image, computed once per image"""
    maps = {}

    def get(img):
        key = (img.shape, img.tobytes())
        if key not in maps:
            maps[key] = oracle.good_features_to_track(img, 1, 0.01, 1, want_eig=True)[1]
            maps[key].setflags(write=False)
        return maps[key]
    return get


@pytest.fixture(scope="module")
def cases(eig_of):
    return GC.build(eig_of)


def _run(oracle, c):
    return oracle.good_features_to_track(c.img, c.max_corners, c.quality, c.min_distance, c.mask)


# ------------------------------------------------------------------ every list is there, whole
def test_no_case_is_missing(cases):
    assert list(cases["response"]) == list(GC.RESPONSE_SIZES) and len(GC.RESPONSE_SIZES) == 6
    for size, lst in cases["response"].items():
        assert [c.name.split()[0] for c in lst] == list(GC.RESPONSE_KINDS) and len(lst) == 8
        assert all(c.img.shape == size[::-1] and c.img.dtype == np.uint8 for c in lst)
    assert [c.name for c in cases["count"]] == list(GC.COUNT_NAMES) and len(GC.COUNT_NAMES) == 11
    assert GC.COUNT_NS == (1, 2, 255, 256, 257, 2047, 2048, 2049)
    assert [c.name for c in cases["threshold"]] == list(GC.THRESHOLD_NAMES) and len(GC.THRESHOLD_NAMES) == 2
    assert len(cases["tie"]) == GC.N_TIE_CASES == 35
    assert {(c.min_distance, c.max_corners) for c in cases["tie"]} == {(1, GC.TIE_MAX_CNT)} | {
        (md, mc) for md in (2, 2.5, 10) for mc in (1, 7)}
    assert [c.name for c in cases["mask"]] == list(GC.MASK_NAMES) and len(GC.MASK_NAMES) == 6
    assert len(cases["word_edge"]) == GC.N_WORD_EDGE_CASES == 8
    assert [c.name for c in cases["negative_max"]] == list(GC.NEGATIVE_MAX_NAMES) and len(GC.NEGATIVE_MAX_NAMES) == 3
    assert {c.img.shape[1] for c in cases["word_edge"]} == {63, 64, 65, 97}
    allowed = {int(v) for c in cases["mask"] + cases["word_edge"] for v in np.unique(c.mask)} - {0}
    assert allowed == {1, 255}


# ------------------------------------------------------------------ a. response map
@pytest.mark.parametrize("W,H", GC.RESPONSE_SIZES)
def test_response_images_reach_their_edges(eig_of, cases, W, H):
    for c, kind in zip(cases["response"][(W, H)], GC.RESPONSE_KINDS):
        e = eig_of(c.img)
        ref = GC.response_f64(c.img)
        # the project's bound for the oracle's float arithmetic (tests/test_oracle_kat.py)
        assert np.abs(ref - e).max() <= 2e-6 * ref.max(), c.name
        if kind in GC.RANK1_KINDS:
            assert not e.any(), c.name
        if kind in GC.NEGATIVE_KINDS:
            assert (e < 0).any(), c.name
        if kind == "border":
            assert e[0].any() and e[H - 1].any() and e[:, 0].any() and e[:, W - 1].any()
            inner = c.img.copy()
            inner[0], inner[H - 1], inner[:, 0], inner[:, W - 1] = 0, 0, 0, 0
            assert not inner.any()


def test_the_restated_rules_give_the_oracles_corners(oracle, eig_of, cases):
    """candidates, order and greedy of gftt_cases.py on the oracle's map == the oracle's list, on every case"""
    every = [c for lst in cases["response"].values() for c in lst]
    every += cases["count"] + cases["threshold"] + cases["tie"] + cases["mask"] + cases["word_edge"] + cases["negative_max"]
    for c in every:
        assert np.array_equal(_run(oracle, c), GC.expected(eig_of(c.img), c)), c.name


# ------------------------------------------------------------------ b. counts, threshold
def test_counts_are_exactly_the_named_ones(oracle, eig_of, cases):
    want = [0, 0, 0] + list(GC.COUNT_NS)
    for c, n in zip(cases["count"], want):
        assert len(_run(oracle, c)) == n, c.name
        assert len(GC.candidates(eig_of(c.img), None, c.quality)) == n, c.name
    assert not eig_of(cases["count"][2].img).any()  # the constant image
    assert len(GC.sorted_values(eig_of(GC.count_image()))) >= 2049


def test_threshold_equals_a_candidate_bit_for_bit(oracle, eig_of, cases):
    out, inn = cases["threshold"]
    e = eig_of(out.img)
    v = GC.sorted_values(e)[GC.THRESHOLD_K]
    assert GC.threshold(e, None, out.quality).view(np.uint32) == v.view(np.uint32)
    assert GC.threshold(e, None, inn.quality) < v
    assert inn.quality == np.nextafter(out.quality, 0.0)
    a, b = _run(oracle, out), _run(oracle, inn)
    y, x = np.argwhere(e == v)[0]
    assert (e == v).sum() == 1 and len(a) == GC.THRESHOLD_K and len(b) == GC.THRESHOLD_K + 1
    assert [x, y] not in a.tolist() and b[-1].tolist() == [x, y]


# ------------------------------------------------------------------ c. ties
def test_tie_images_have_tie_groups_over_rows(eig_of):
    for kind in GC.TIE_KINDS:
        e = eig_of(GC.tie_image(kind))
        cand = GC.candidates(e, None, 0.01)
        groups, largest, spanning = GC.tie_stats(e, cand)
        assert spanning >= 1 and len(cand) <= GC.TIE_MAX_CNT, kind
        distinct = len(np.unique(e.reshape(-1)[cand]))
        if kind in GC.ONE_VALUE_KINDS:
            assert distinct == 1 and largest == len(cand) > 100, kind
        if kind == "checker":  # plateaus: more than three radix tiles of candidates, few values
            assert len(cand) >= 3 * 2048 and distinct <= 4
        if kind == "tiled":   # groups among distinct values
            assert groups >= 10 and spanning >= 5 and distinct > groups
        if kind == "binary":  # hundreds of candidates in small groups
            assert groups >= 40 and largest <= 8 and len(cand) > 400


def test_tie_cases_return_tied_corners(oracle, eig_of, cases):
    """the whole lists hold every candidate; the short ones are cut inside or right after a tie group"""
    for c in cases["tie"]:
        got = _run(oracle, c)
        e = eig_of(c.img)
        if c.max_corners == GC.TIE_MAX_CNT:
            assert len(got) == len(GC.candidates(e, None, 0.01)) and GC.tied_pairs(e, got) > 0, c.name
        else:
            assert len(got) == c.max_corners, c.name
    assert sum(GC.tied_pairs(eig_of(c.img), _run(oracle, c)) > 0 for c in cases["tie"] if c.max_corners == 7) >= 4


# ------------------------------------------------------------------ d. masks
def test_mask_cases_do_what_they_are_named_for(oracle, eig_of, cases):
    strongest, peaks, one, row0, nothing, last = cases["mask"]
    # the maximum is taken over the allowed pixels: without the strong square the weak ones pass the threshold
    assert len(_run(oracle, strongest)) == 8 > len(_run(oracle, strongest._replace(mask=None))) == 4
    # masked pixels still take part in the 3x3 maximum: the peaks' neighbours stay suppressed
    assert len(_run(oracle, peaks)) == 0 and len(_run(oracle, peaks._replace(mask=None))) > 50
    assert (peaks.mask != 0).sum() > peaks.mask.size * 0.9
    got = _run(oracle, one)
    y, x = np.argwhere(one.mask)[0]
    assert got.tolist() == [[x, y]] and one.mask.sum() == 1
    e = eig_of(row0.img)
    assert len(_run(oracle, row0)) == 0 and (row0.mask != 0).sum() == 1 and row0.mask[0].any() and e[0, 10] > 0
    assert len(_run(oracle, nothing)) == 0 and not nothing.mask.any()
    assert len(_run(oracle, last)) == 0 and (last.mask != 0).sum() == 1 and last.mask[-1, -1]


def test_word_edge_masks_leave_corners_in_their_columns(oracle, cases):
    for c in cases["word_edge"]:
        got = _run(oracle, c)
        col = 31 if "== 31" in c.name else 0
        assert len(got) >= 1 and (got[:, 0].astype(int) % 32 == col).all(), c.name
        assert (c.mask != 0).any(0).sum() == len(range(col, c.img.shape[1], 32)), c.name


def test_negative_maximum_cases_have_a_negative_threshold(oracle, eig_of, cases):
    below, above, several = cases["negative_max"]
    e = eig_of(below.img)
    assert e[below.mask != 0].max() < 0 and (below.mask != 0).sum() > 100
    assert GC.threshold(e, below.mask, below.quality) < 0 and GC.threshold(e, above.mask, above.quality) < 0
    assert len(_run(oracle, below)) == 0
    got = _run(oracle, above).astype(int)
    assert len(got) > 20 and (e[got[:, 1], got[:, 0]] < 0).all()
    # several values below zero: the list runs from the one nearest zero down, each value a tie group of its own
    e = eig_of(several.img)
    got = _run(oracle, several).astype(int)
    v = e[got[:, 1], got[:, 0]]
    distinct = len(np.unique(v))
    assert distinct > 1 and distinct == 3 and len(got) == 14 and (v < 0).all() and (np.diff(v) <= 0).all()
    assert GC.tied_pairs(e, got) > 0 and GC.threshold(e, several.mask, several.quality) < v.min()


# ------------------------------------------------------------------ the reason this file exists
@pytest.mark.parametrize("W,H,md,use_mask", GC.PARITY_PARAMS)
def test_the_existing_device_tests_inputs_return_no_tied_pair(oracle, W, H, md, use_mask):
    """test_good_features_to_track_matches_oracle at 160x120 and 346x260: no two returned corners share a response, so
    it cannot tell which way the sort breaks ties"""
    for img, mask in GC.parity_inputs(W, H, md, use_mask):
        for maxc in (150, 7):
            c, e = oracle.good_features_to_track(img, maxc, 0.01, md, mask, want_eig=True)
            assert len(c) > 3 and GC.tied_pairs(e, c) == 0
        assert not (e < 0).any()
