"""The planes of tests/arc_cases.py reach the edges of Arc* they are for — shown from the oracle and one independent
transcription alone, without a GPU: the oracle agrees with the transcription on every planted ring; every counted
family has rings that pass and rings that fail; the rings tell three plausible mistakes in the loop from the right
code; the pre-check triples flip where the reference's comparisons flip; the border cases sit on the limit; the
selection case has corner centres that render to TS_LK_THRESHOLD and next to it."""
import operator

import numpy as np
import pytest

from esvio_amd.events import event_times

import arc_cases as AC

ALL_FAMILIES = [(f, W, H) for f in AC.FAMILIES for W, H in AC.family_sizes(f)]


def _oracle_flags(oracle, W, H, L0, L1, S0, S1, ev, **kw):
    d = oracle.Detector(W, H, **dict(dict(min_dist=AC.MIN_DIST), **kw))
    d.set_sae(0, L0, L1, S0, S1)
    return d.corner_flags(ev)


def test_grid():
    assert len(AC.centres(346, 260)) == 1064
    for W, H in AC.SIZES:
        cs = AC.centres(W, H)
        seen = np.zeros((H, W), np.int32)
        for x, y in cs:
            for dx, dy in AC.SMALL + AC.LARGE:
                seen[y + dy, x + dx] += 1  # (raises where a ring leaves the plane)
        assert seen.max() == 1  # every ring pixel is one centre's own
        assert min(x for x, _ in cs) == 4 and min(y for _, y in cs) == 4  # the large ring touches row and column 0
    # what the sizes are for: a partial last region and bitmap word, an odd pixel count, a region that is a row
    assert (346 * 260) % 256 and (2 * 346 * 260) % 32 and (173 * 131) % 2 and 256 == 256 * 64 // 64
    assert len(AC.twolevel(16)) == 240 and len(AC.twolevel(20)) == 380
    assert AC.ring_python(AC.PASSING[16]) and AC.ring_python(AC.PASSING[20])
    assert int((AC.PASSING[16] == AC.NEW).sum()) == 5 and int((AC.PASSING[20] == AC.NEW).sum()) == 6


@pytest.mark.parametrize("name,W,H", ALL_FAMILIES)
def test_oracle_equals_transcription(oracle, name, W, H):
    n = {1: 0, 0: 0}
    for page in AC.family_pages(name, W, H):
        flags = _oracle_flags(oracle, W, H, *page[:5])
        S = {0: page.S0, 1: page.S1}
        for i, (k, x, y, pol, small, large) in enumerate(page.rings):
            want = AC.arc_python(S[pol], x, y)
            assert want == (AC.ring_python(small) and AC.ring_python(large))  # the plane holds the rings
            assert bool(flags[i]) == want, AC.describe(page, i, int(flags[i]), int(want))
            n[pol] += 1
    assert n[1] == len(AC.family(name, 16)) and n[0] == len(AC.family(name, 20))


@pytest.mark.parametrize("N", [16, 20])
@pytest.mark.parametrize("name", AC.COUNTED)
def test_shares(name, N):
    """at least 5 % of a counted family's rings pass and at least 5 % fail, per ring size"""
    got = [AC.ring_python(v) for v in AC.family(name, N)]
    share = sum(got) / len(got)
    print("%s N=%d: %d of %d pass" % (name, N, sum(got), len(got)))
    assert 0.05 <= share <= 0.95, (name, N, sum(got), len(got))
    if name == "twolevel":
        assert sum(got) == {16: 96, 20: 160}[N]  # lengths 4..6 and 10..12 of 16; 5..8 and 12..15 of 20


def test_families_hold_the_ties_they_promise():
    for N in (16, 20):
        for v in AC.family("noisy", N) + AC.family("overlap", N) + AC.family("ternary", N):
            assert len(set(v.tolist())) <= 6
        assert any(len(set(v.tolist())) < N - 4 for v in AC.family("noisy", N))
        assert all(len(set(v.tolist())) == N for v in AC.family("perm", N))
        ov = AC.family("overlap", N)
        assert sum(1 for v in ov if (v == 2.0).sum() >= 2) > len(ov) // 2
        r = AC.family("ramps", N)
        assert any(v[0] == v.max() and v[N - 1] == v.max() for v in r)  # equal maxima at indices 0 and N - 1
        assert sum(1 for v in r if (v == v.max()).sum() >= 3) >= 10
        sym = 0
        for v in r:  # the frontier pixels left and right of the first maximum tie
            m = int(np.argmax(v))
            sym += v[(m - 1) % N] == v[(m + 1) % N]
        assert sym >= 10
        # epoch: the levels are consecutive doubles at 1.7e9 s
        lv = sorted({float(a) for v in AC.family("epoch", N) for a in v})
        assert lv[0] == AC.EPOCH and all(np.nextafter(a, np.inf) == b for a, b in zip(lv, lv[1:])) and len(lv) >= 6
        assert float(event_times(AC.records([0], [0], AC.family_time_us("epoch"), 1))[0]) > lv[-1]
    # every field of the packed ranks, the large ring's second word included, is an arc's start
    for N in (16, 20):
        assert {int(np.argmax(v)) for v in AC.twolevel(N)} == set(range(N))


def _accept_size_below_kmax(size, N, kmin, kmax):
    return size < kmax or (N - kmax <= size <= N - kmin)


def _accept_upper_exclusive(size, N, kmin, kmax):
    return size <= kmax or (N - kmax <= size < N - kmin)


WRONG = {
    "join with > for >=": dict(join=operator.gt),
    "size < kmax for <=": dict(accepts=_accept_size_below_kmax),
    "exclusive upper bound at N - kmin": dict(accepts=_accept_upper_exclusive),
}


@pytest.mark.parametrize("N", [16, 20])
@pytest.mark.parametrize("wrong", list(WRONG))
def test_rings_tell_a_wrong_loop_from_the_right_one(wrong, N):
    """each deliberately wrong transcription changes the answer of at least 10 rings of the counted families"""
    rings = [v for name in AC.COUNTED for v in AC.family(name, N)]
    changed = sum(AC.ring_python(v) != AC.ring_python(v, **WRONG[wrong]) for v in rings)
    print("%s N=%d: %d of %d rings change" % (wrong, N, changed, len(rings)))
    assert changed >= 10, (wrong, N, changed)


@pytest.mark.parametrize("thr", AC.THRESHOLDS)
def test_precheck_triples_flip_where_the_comparisons_flip(oracle, thr):
    L0, L1, S0, S1, evs = AC.precheck_planes(thr)
    own = _oracle_flags(oracle, AC.PRE_W, AC.PRE_H, L0, L1, S0, S1, evs["own"], filter_threshold=thr)
    both = _oracle_flags(oracle, AC.PRE_W, AC.PRE_H, L0, L1, S0, S1, evs["both"], filter_threshold=thr)
    assert np.array_equal(both[0::2], own)
    for which in ("own", "other", "both"):
        got = _oracle_flags(oracle, AC.PRE_W, AC.PRE_H, L0, L1, S0, S1, evs[which], filter_threshold=thr)
        assert np.array_equal(got, AC.is_corner_python(L0, L1, S0, S1, evs[which], thr=thr)), which
    cases = AC.precheck_cases(thr)
    assert len(cases) == 8
    k = 0
    for name, t_us, tri in cases:
        et = float(event_times(AC.records([0], [0], t_us, 1))[0])  # formed from sec / nsec as event_times does it
        below, equal, above = (int(own[k + j]) for j in range(3))
        assert (below, equal, above) == (1, 1, 0), (name, below, equal, above)
        if name.startswith("refractory"):
            sums = [c.L_own + thr for c in tri]
            assert sums == [np.nextafter(et, np.inf), et, np.nextafter(et, -np.inf)], name
        else:
            assert [c.L_other for c in tri] == [np.nextafter(et, -np.inf), et, np.nextafter(et, np.inf)], name
        k += 3


@pytest.mark.parametrize("min_dist", AC.BORDER_MIN_DISTS)
def test_border_cases_sit_on_the_limit(oracle, min_dist):
    L0, L1, S0, S1, ev = AC.border_planes(min_dist)
    flags = _oracle_flags(oracle, AC.BORDER_W, AC.BORDER_H, L0, L1, S0, S1, ev, min_dist=min_dist)
    assert np.array_equal(flags, AC.is_corner_python(L0, L1, S0, S1, ev, min_dist=min_dist))
    b = min_dist + 1
    for k, (side, outside, on) in enumerate(AC.border_cases(min_dist)):
        assert flags[4 * k:4 * k + 4].tolist() == [0, 0, 1, 1], (side, min_dist, flags[4 * k:4 * k + 4].tolist())
        moved = [abs(outside[0] - on[0]), abs(outside[1] - on[1])]
        assert sorted(moved) == [1, 18]
    (_, l_out, l_on), (_, t_out, t_on), (_, r_out, r_on), (_, b_out, b_on) = AC.border_cases(min_dist)
    assert (l_out[0], l_on[0], t_out[1], t_on[1]) == (b - 1, b, b - 1, b)
    assert (r_on[0], r_out[0]) == (AC.BORDER_W - b - 1, AC.BORDER_W - b)
    assert (b_on[1], b_out[1]) == (AC.BORDER_H - b - 1, AC.BORDER_H - b)


def test_event_batches(oracle):
    page = AC.event_page()
    flags = _oracle_flags(oracle, AC.EV_W, AC.EV_H, *page[:5])
    assert 100 < flags.sum() < len(flags) - 100 and len(flags) > 257
    for pol in (0, 1):
        assert flags[page.events["polarity"] == pol].any()
    ev = AC.outside_events(page)
    out = (ev["x"] >= AC.EV_W) | (ev["y"] >= AC.EV_H)
    assert out.sum() == 7 and {(AC.EV_W, 4), (4, AC.EV_H), (0xffff, 0xffff)} <= set(zip(ev["x"][out].tolist(), ev["y"][out].tolist()))
    f2 = _oracle_flags(oracle, AC.EV_W, AC.EV_H, *page[:4], ev)
    assert not f2[out].any() and np.array_equal(f2[~out], flags)
    assert np.array_equal(f2, AC.is_corner_python(*page[:4], ev))
    rep = AC.repeated_pixel_events(page)
    f3 = _oracle_flags(oracle, AC.EV_W, AC.EV_H, *page[:4], rep)
    assert len(rep) > 3 * 256 and np.array_equal(f3, AC.is_corner_python(*page[:4], rep))
    first_late = int(np.argmin(f3 | (np.arange(len(rep)) % 7 == 3)))
    assert 256 < first_late < 3 * 256  # the flags of one pixel change in the middle of the batch
    assert f3[:first_late][np.arange(first_late) % 7 != 3].all() and not f3[first_late:].any()
    assert not f3[np.arange(len(rep)) % 7 == 3].any()


def test_selection_case_renders_centres_around_the_threshold(oracle):
    L0, L1, S0, S1, ev, mask, t = AC.selection_case()
    W, H = AC.SEL_W, AC.SEL_H
    d = oracle.Detector(W, H, min_dist=AC.SEL_MIN_DIST, decay_ms=1000 * AC.DECAY_S)
    d.set_sae(0, L0, L1, S0, S1)
    ts = d.time_surface(0, t)
    flags = d.corner_flags(ev)
    assert np.array_equal(flags, AC.is_corner_python(L0, L1, S0, S1, ev, min_dist=AC.SEL_MIN_DIST))
    at = ts[ev["y"], ev["x"]]
    for byte in (127, 128, 129):
        assert (flags.astype(bool) & (at == byte)).sum() >= 20, byte  # corner centres at 128 and next to it
    cs = AC.centres(W, H)
    old = [c for i, c in enumerate(cs) if i % 32 == 4]
    assert all(ts[y, x] == 128 and S1[y, x] > 0 for x, y in old)  # 128 from a stamp, not from an empty pixel
    assert (flags.astype(bool) & (mask[ev["y"], ev["x"]] == 255)).sum() >= 20  # blocked corners
    xy, idx = d.features_to_track(ev, 300, AC.SEL_MIN_DIST, mask, ts)
    assert len(idx) > 100
    assert not (at[idx] == 128).any() and not mask[ev["y"][idx], ev["x"][idx]].any()
    # duplicates: a pixel's two candidates of one polarity lie in different 256-event blocks
    n = len(ev) // 2
    second = 2 * n - 1 - np.arange(n)
    assert np.array_equal(ev[:n], ev[second])
    far = (second // 256 != np.arange(n) // 256) & flags[:n].astype(bool)
    assert far.sum() > 100
    for b in AC.epoch_batches():
        assert len(b) > 256 and d.corner_flags(b).sum() > 20
