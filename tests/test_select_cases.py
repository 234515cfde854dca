"""CPU: the selection's reference (tests/select_ref.py) is the rule both oracles and OpenCV's recordings follow, and
the case families of tests/select_cases.py reach the edges they are named for — shown by deliberately wrong copies of
the reference, each of which must change the outcome of the family meant for it.  No device involved;
tests/test_select_edges_gpu.py runs the same cases through the three kernels."""
import os

import numpy as np
import pytest

from esvio_amd.events import make_events

import select_cases as SC
import select_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _filled(W, H, cx, cy, hw, clip=True):
    m = bytearray(W * H)
    SR.fill_disc(m, W, H, cx, cy, hw, clip)
    return np.frombuffer(bytes(m), np.uint8).reshape(H, W)


# ------------------------------------------------------------------------------------------------ disc tables
def test_midpoint_table_is_the_oracles_at_every_radius(oracle):
    for r in range(1, 64):
        assert SR.midpoint_halfwidths(r) == list(oracle.disc_halfwidths(r)), r
    for d in range(1, 64):
        assert SR.euclid_halfwidths(d) == [int(v) for v in oracle.euclid_halfwidths(d) if v >= 0], d


def test_filled_clipped_disc_is_the_oracles_and_cv2s(oracle):
    W, H = 97, 67
    for r in (1, 3, 10, 15, 16, 31, 32, 63):
        hw = SR.midpoint_halfwidths(r)
        for cx, cy in ((0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (48, 33), (1, 65), (95, 2), (31, 32), (64, 0)):
            b = np.zeros((H, W), np.uint8)
            oracle.circle_fill(b, cx, cy, r, 255)
            assert np.array_equal(_filled(W, H, cx, cy, hw), b), (r, cx, cy)
    # the centres OpenCV was asked to draw (tests/golden/cv2_pin_inputs.npz) at the shipped radii: against cv2 itself
    # where it is installed, against its returned outputs where they are committed, against the oracle always
    inp = np.load(os.path.join(ROOT, "tests", "golden", "cv2_pin_inputs.npz"))
    H, W = inp["ts_cur_left"].shape
    try:
        import cv2
    except ImportError:
        cv2 = None
    outputs = os.path.join(ROOT, "tests", "golden", "cv2_pin_outputs.npz")
    out = np.load(outputs) if os.path.exists(outputs) else {}
    for r in (10, 20, 30):
        for k, (cx, cy) in enumerate(inp["circle_centres"]):
            mine = _filled(W, H, int(cx), int(cy), SR.midpoint_halfwidths(r))
            b = np.zeros((H, W), np.uint8)
            oracle.circle_fill(b, int(cx), int(cy), r, 255)
            assert np.array_equal(mine, b), (r, k)
            if cv2 is not None:
                a = np.zeros((H, W), np.uint8)
                cv2.circle(a, (int(cx), int(cy)), r, 255, -1)
                assert np.array_equal(mine, a), (r, k)
            if "circle_%d_%d" % (r, k) in out:
                assert np.array_equal(np.packbits(mine), out["circle_%d_%d" % (r, k)]), (r, k)


@pytest.mark.parametrize("kind", ["circle", "euclid"])
def test_tables_are_symmetric_euclidean_threshold_sets(kind):
    """dx <= hw[dy] iff dy <= hw[dx] (the 16-wave kernel's greedy takes "lies in the other's disc" for symmetric), and
    the largest dx*dx + dy*dy inside is smaller than the smallest outside: what disc_threshold() (fe_kernels.h) rests
    on when it replaces the table look-up by one comparison — at every radius 1..63"""
    for d in range(1, 64):
        hw = SR.halfwidths(kind, d)
        r = len(hw) - 1
        at = lambda i: hw[i] if i <= r else -1
        inside, outside = -1, None
        for dy in range(r + 2):
            for dx in range(r + 2):
                assert (dx <= at(dy)) == (dy <= at(dx)), (kind, d, dx, dy)
                q = dx * dx + dy * dy
                if dx <= at(dy):
                    inside = max(inside, q)
                else:
                    outside = q if outside is None else min(outside, q)
        assert 0 <= inside < outside, (kind, d, inside, outside)


# ------------------------------------------------------------------------------------------------ the oracles
def _wedge_detector(oracle, W, H):
    """wedge corners on a 16-pixel grid (as test_oracle_kat.py's selection test plants two): every one an Arc* corner"""
    d = oracle.Detector(W, H, min_dist=5)
    yy, xx = np.mgrid[0:H, 0:W]
    S1 = np.full((H, W), 1.0)
    corners = [(cx, cy) for cy in range(8, H - 20, 16) for cx in range(8, W - 20, 16)]
    for cx, cy in corners:
        S1 = np.where((xx >= cx) & (yy >= cy) & (xx < cx + 12) & (yy < cy + 12), 5.0 - 0.001 * (xx - cx + yy - cy), S1)
    d.set_sae(0, np.zeros((H, W)), np.full((H, W), 5.0), np.zeros((H, W)), S1)
    return d, corners


@pytest.mark.parametrize("r", [3, 10, 16, 20, 33])
def test_reference_is_the_oracles_event_selection(oracle, r):
    """oracle.Detector.features_to_track over events of which some are corners == the reference over the corner events
    that pass the time-surface test, with and without a mask, with and without a cut at max_corners"""
    W, H = 173, 131
    d, corners = _wedge_detector(oracle, W, H)
    rng = np.random.default_rng(r)
    pts = np.array(corners)[rng.permutation(len(corners))]
    pts = np.concatenate([pts, pts[::3], rng.integers(20, 100, (40, 2))])  # duplicates; pixels that are no corners
    ev = make_events(pts[:, 0], pts[:, 1], np.full(len(pts), 5_000_000), np.ones(len(pts)))
    flags = d.corner_flags(ev).astype(bool)
    assert flags[:len(corners)].all() and flags.sum() >= 40
    ts = np.full((H, W), 200, np.uint8)
    ts[pts[5, 1], pts[5, 0]] = 128  # TS_LK_THRESHOLD: skipped before the corner test
    cand = np.nonzero(flags & (ts[pts[:, 1], pts[:, 0]] != 128))[0]
    xy = SR.pack_xy(pts[cand, 0], pts[cand, 1])
    mask = np.zeros((H, W), np.uint8)
    mask[40:80, 30:90] = 255
    mask[0:30, :] = 254  # (only 255 blocks)
    for m in (np.zeros((H, W), np.uint8), mask):
        for mc in (1000, 7, 1):
            o_xy, o_idx = d.features_to_track(ev, mc, r, m, ts)
            p, i, c = SR.select(W, H, xy, cand, SR.midpoint_halfwidths(r), m, None, mc)
            assert np.array_equal(p, o_xy) and np.array_equal(i, o_idx) and c[0] == len(o_idx), (r, mc)
    assert 0 < len(SR.select(W, H, xy, cand, SR.midpoint_halfwidths(r), mask)[1]) < len(cand)


@pytest.mark.parametrize("md", [1, 2, 5, 5.5, 16, 17, 30, 33, 40])
def test_reference_is_the_oracles_distance_pass(oracle, md):
    """oracle.good_features_to_track with a min_distance == the reference, open Euclidean disc, over the corners the
    same call returns without one (sorted by response, no distance test) — also through a mask"""
    inp = np.load(os.path.join(ROOT, "tests", "golden", "cv2_pin_inputs.npz"))
    img = inp["tex_a"]
    H, W = img.shape
    allc, eig = oracle.good_features_to_track(img, 0, 0.01, 0, want_eig=True)
    assert len(allc) > 200
    xy = SR.pack_xy(allc[:, 0].astype(np.int64), allc[:, 1].astype(np.int64))
    hw = SR.euclid_halfwidths(md)
    for mc in (0, 50):
        got = oracle.good_features_to_track(img, mc, 0.01, md)
        p, _, _ = SR.select(W, H, xy, np.zeros(xy.size, np.int32), hw, max_corners=mc if mc else None)
        assert np.array_equal(p, got), (md, mc)
    # a mask that leaves the strongest pixel allowed keeps the quality threshold: its blocked pixels are the
    # reference's seed mask (nonzero = allowed there, 255 = blocked here)
    allowed = np.full((H, W), 255, np.uint8)
    allowed[:, W // 2 - 30:W // 2 + 30] = 0
    my, mx = np.unravel_index(int(np.argmax(eig)), eig.shape)
    allowed[my, mx] = 255
    got = oracle.good_features_to_track(img, 0, 0.01, md, mask=allowed)
    p, _, _ = SR.select(W, H, xy, np.zeros(xy.size, np.int32), hw, mask=np.where(allowed == 0, 255, 0).astype(np.uint8))
    assert np.array_equal(p, got) and 0 < len(got) < len(allc), md


# ------------------------------------------------------------------------------------------------ the families
def test_family_a_every_verdict_is_the_anchors_alone():
    """the probes that are refused are exactly the ones on a disc row's last pixel; without the anchors (and the
    fillers, their duplicates) every probe is accepted and nothing else changes; no pixel of one pair lies within
    the disc's reach of another pair's"""
    n_cases = 0
    for cases in (SC.small_cases()["a"], SC.large_cases(SC.LARGE_ONE_WAVE)["a"], SC.large_cases(SC.LARGE_GBM)["a"]):
        for c in cases:
            m = c["meta"]
            r = len(SR.halfwidths(c["kind"], c["d"])) - 1
            _, idx, cnt = SC.expected(c)
            pay = c["payload"]
            n = len(m["probe_idx"])
            anchors = m["anchor_idx"][:n]
            assert set(pay[anchors]) <= set(idx)
            refused = np.array([pay[i] not in set(idx) for i in m["probe_idx"]])
            assert np.array_equal(refused, m["inside"]), c["name"]
            alone = dict(c, xy=c["xy"][m["probe_idx"]], payload=pay[m["probe_idx"]])
            alone.pop("_expected", None)
            assert np.array_equal(SC.expected(alone)[1], pay[m["probe_idx"]]), c["name"]
            x, y = (c["xy"] & 0xffff).astype(np.int64), (c["xy"] >> 16).astype(np.int64)
            ax, ay, px, py = x[anchors], y[anchors], x[m["probe_idx"]], y[m["probe_idx"]]
            for ux, uy in ((ax, ay), (px, py)):
                for vx, vy in ((ax, ay), (px, py)):
                    dist = np.maximum(np.abs(ux[:, None] - vx[None, :]), np.abs(uy[:, None] - vy[None, :]))
                    dist[np.arange(n), np.arange(n)] = r + 1
                    assert dist.min() > r, c["name"]
            if "bitmap" in c["name"]:
                assert m["probe_idx"][0] >= 1100 + n and n <= 32
            n_cases += 1
    assert n_cases > 1000


def test_family_sizes_lengths_and_floors():
    S = SC.small_cases()
    assert sorted({c["xy"].size for c in S["d"]}) == sorted(SC.D_TOTALS)
    for c in S["d"]:
        acc = SC.expected(c)[2][0]
        assert acc == (c["xy"].size if " far " in c["name"] else min(c["xy"].size, 1)), c["name"]
    # (e) the live candidates per sub-chunk are what the names say
    for c in S["e"]:
        if "live" in c["meta"] or "acc" in c["meta"]:
            pos = int(c["name"].split(" at ")[1])
            sub = c["xy"][64 * pos:64 * pos + 64]
            live = (c["mask"][sub >> 16, sub & 0xffff] != 255).sum()
            assert live == c["meta"].get("live", 20), c["name"]
            if "acc" in c["meta"]:
                chunk_pay = set(c["payload"][64 * pos:64 * pos + 64])
                assert len(chunk_pay & set(SC.expected(c)[1])) == c["meta"]["acc"], c["name"]
            others = np.concatenate([c["xy"][:64 * pos], c["xy"][64 * pos + 64:256]])
            assert (c["mask"][others >> 16, others & 0xffff] == 255).all()
    # (f) the cuts cut
    for c in S["f"]:
        assert SC.expected(c)[2][0] == min(c["max_corners"], c["meta"]["full"]), c["name"]
    # (g)
    for c in S["g"]:
        if "all blocked" in c["name"]:
            assert SC.expected(c)[2][0] == 0
        if "all but one" in c["name"]:
            assert SC.expected(c)[2][0] == 1 and SC.pack_xy(*SC.expected(c)[0][0].astype(np.int64)) == c["meta"]["only"]
    # (h) the first copy's payload comes back
    for c in S["h"]:
        _, idx, _ = SC.expected(c)
        first = {}
        for v, p in zip(c["xy"].tolist(), c["payload"].tolist()):
            first.setdefault(v, p)
        assert set(idx.tolist()) <= set(first.values()), c["name"]
    # (i) 20 accepted, 20 refused, by the reference alone
    for cases in (S["i"], SC.large_cases(SC.LARGE_ONE_WAVE)["i"], SC.large_cases(SC.LARGE_GBM)["i"]):
        for c in cases:
            acc, _, tot = SC.expected(c)[2]
            assert acc >= 20 and tot - acc >= 20, (c["name"], acc, tot)
    # every size, every radius class somewhere
    assert {(c["W"], c["H"]) for f in S.values() for c in f} == set(SC.SMALL)
    assert {(c["kind"], c["d"]) for c in S["a"]} == set(SC.DISCS)


def test_family_c_reads_every_bit():
    """per anchor set: the blocked call's probes and the free calls' probes are every pixel of the sensor once; blocked
    probes are all refused, free probes all accepted (their classes keep them out of each other's discs)"""
    groups = {}
    for c in SC.small_cases()["c"]:
        key = (c["W"], c["H"], c["d"], c["name"].split(" ")[3])
        groups.setdefault(key, []).append(c)
    assert len(groups) >= 20
    for key, cs in groups.items():
        seen = np.zeros((key[1], key[0]), np.int32)
        for c in cs:
            na = c["meta"]["n_anchor"]
            pr = c["xy"][na:]
            np.add.at(seen, (pr >> 16, pr & 0xffff), 1)
            got = set(SC.expected(c)[1].tolist())
            acc = np.array([p in got for p in c["payload"][na:].tolist()])
            assert (not acc.any()) if c["meta"]["blocked"] else acc.all(), c["name"]
        assert (seen == 1).all(), key


# ------------------------------------------------------------------------------------------------ wrong copies
def _changed(cases, **wrong):
    return sum(0 if SC.same(SC.expected(c), SC.expected(c, **dict(wrong))) else 1 for c in cases)


def wrong_copy_counts():
    """{wrong copy: (cases it changes, cases of the family meant for it)}; the single-row copies: (rows caught, rows)"""
    S = SC.small_cases()
    out = {}
    rows = caught = changed = 0
    for disc in SC.DISCS:
        hw = SR.halfwidths(*disc)
        mine = [c for c in S["a"] if (c["kind"], c["d"]) == disc]
        for ady in range(len(hw) + 1):
            with_row = [c for c in mine if (c["meta"]["ady"] == ady).any()]
            for delta in (-1, 1):
                if ady == len(hw) and delta < 0:
                    continue  # (the row behind the last one is empty already)
                t = list(hw) + [-1]
                t[ady] += delta
                while t and t[-1] < 0:
                    t.pop()
                n = _changed(with_row, hw=t)
                rows, caught, changed = rows + 1, caught + (n > 0), changed + n
    out["one row's half-width off by one (a)"] = (caught, rows, changed)
    for d in (5, 30, 40):
        mine = [c for c in S["a"] if (c["kind"], c["d"]) == ("euclid", d)]
        out["<= for < in the Euclidean disc, d = %d (a)" % d] = (_changed(mine, hw=SR.euclid_halfwidths(d, closed=True)), len(mine))
    out["disc rows not clipped (b)"] = (_changed(S["b"], clip=False), len(S["b"]))
    out["disc rows not clipped (c)"] = (_changed(S["c"], clip=False), len(S["c"]))
    hi = S["h"] + S["i"]
    out["a refused candidate stamps too (h, i)"] = (_changed(hi, stamp_refused=True), len(hi))
    out["max_corners looked at per 64 (f)"] = (_changed(S["f"], cap_every=64), len(S["f"]))
    stamps = [c for c in S["b"] + S["g"] if c["stamps"] is not None]
    out["kept points truncated, not rounded (b, g)"] = (_changed(stamps, rounding=np.trunc), len(stamps))
    return out


def test_wrong_copies_are_caught():
    counts = wrong_copy_counts()
    for k, v in counts.items():
        print("%-50s %s" % (k, " / ".join(str(x) for x in v)))
    caught, rows, _ = counts.pop("one row's half-width off by one (a)")
    assert caught == rows and rows > 800, (caught, rows)
    for k, (n, of) in counts.items():
        assert n >= 1, k
