"""CPU: the designed inputs of tests/mc_cases.py reach the edges of the motion-compensated SAE write they are named
for -- every branch of Matrix3f::exp() and every count of squarings, the acceleration gate at exactly 5, the time gate at
a ratio of exactly 1, the kBorder band, the landing bound, a homogeneous coordinate of exactly 0, many sources on one
pixel -- and the oracle's planes on them are the planes of the module's float64 restatement on every pixel outside the
unsure set.  Deliberately wrong variants of the restatement fail that comparison.  No device involved;
tests/test_mc_edges_gpu.py runs the same cases through the kernels.

Why the cases exist: test_motion_compensated_sae (tests/test_parity_gpu.py) compares the device with the oracle, which
states the same float arithmetic a second time from the same recollection; nothing there is aimed at a gate, a border or
a branch threshold."""
import numpy as np
import pytest

import mc_cases as MC
from esvio_amd.events import event_times

SIZES = list(MC.SIZES)


@pytest.fixture(scope="module")
def oracle_planes(oracle):
    """the oracle's planes after a case's first batch, computed once per case"""
    done = {}

    def get(case):
        key = (case.W, case.H, case.name)
        if key not in done:
            done[key] = MC.oracle_planes(oracle, case, upto=1)
        return done[key]
    return get


def _warps(case, rules=MC.EXACT):
    b = case.batches[0]
    return [MC.warp64(ev, MC._t0(b.L), b.motion, case.W, case.H, rules) for ev in (b.L, b.R)]


def _plain_planes(oracle, case):
    det = oracle.Detector(case.W, case.H)
    det.create_sae(0, case.batches[0].L)
    det.create_sae(1, case.batches[0].R)
    return [det.get_sae(0), det.get_sae(1)]


def _same(a, b):
    return all(np.array_equal(x, y) for cam in (0, 1) for x, y in zip(a[cam], b[cam]))


# ------------------------------------------------------------------ every list is there, whole
def test_no_case_is_missing():
    names = MC.case_names()
    assert len(names) == 24 and len(set(names)) == 24
    assert [n for n in names if n.startswith("dense_")][:6] == ["dense_" + k for k in MC.DENSE_MOTIONS]
    for W, H in SIZES:
        cases = MC.build()[(W, H)]
        assert [c.name for c in cases] == names
        for c in cases:
            assert len(c.batches) == (2 if c.name == "many_to_one" else 1)
            for b in c.batches:
                for ev in (b.L, b.R):
                    assert W * H - 1 <= len(ev) <= W * H <= 33800 and ev.dtype.itemsize == 16
                    assert int(ev["x"].max()) == W - 1 and int(ev["y"].max()) == H - 1
                    assert len(np.unique(ev["x"].astype(np.int64) + W * ev["y"].astype(np.int64))) == len(ev)
    assert set(MC.ORACLE_ONLY) <= set(names) and MC.float64_case_names() == [n for n in names if n != "many_to_one"]


def test_the_band_is_the_measured_one(oracle):
    """DELTA is 4 x the measured disagreement, rounded up to a power of two (the measurement itself, over all 69
    cases, is `python tests/mc_cases.py`; here: the constants belong together, and one size's measurement is no
    larger than the recorded one)"""
    assert MC.DELTA == 2.0 ** np.ceil(np.log2(4 * MC.MEASURED_DISAGREEMENT))
    worst, ndiff, ntot = MC.measure(oracle, sizes=MC.SIZES[2:])
    assert 0 < worst <= MC.MEASURED_DISAGREEMENT < 1e-3 and 0 < ndiff < 1e-4 * ntot


# ------------------------------------------------------------------ the rotation
def test_closed_form_rotation_equals_expm_in_every_band():
    from scipy.linalg import expm
    c = MC.get(176, 176, "pade")
    b = c.batches[0]
    band, sq, _ = MC.pade_band(b.L, MC._t0(b.L), b.motion)
    om = MC.motion_inputs(b.motion)[0]
    dt = event_times(b.L) - MC._t0(b.L)
    picked = 0
    for bd, s in ((3, 0), (5, 0), (7, 0), (7, 1), (7, 2), (7, 3)):
        idx = np.nonzero((band == bd) & (sq == s))[0]
        assert len(idx) >= 5, (bd, s)
        for i in idx[:: max(1, len(idx) // 5)][:5]:
            r = om * dt[i]
            S = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            assert np.abs(MC.rotation64(r)[0] - expm(S)).max() < 1e-12, (bd, s, i)
            picked += 1
    assert picked == 30
    # the series limit joins the closed form: both sides of the switch at 1e-3, and exactly 0
    for t in (0.0, 1e-9, 0.999e-3, 1.001e-3):
        r = np.array([0.6, -0.48, 0.64]) * t
        S = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        assert np.abs(MC.rotation64(r)[0] - expm(S)).max() < 1e-15


@pytest.mark.parametrize("W,H", SIZES)
def test_pade_case_has_events_in_every_branch_and_squaring_count(W, H):
    c = MC.get(W, H, "pade")
    b = c.batches[0]
    for ev, wp in zip((b.L, b.R), _warps(c)):
        band, sq, l1 = MC.pade_band(ev, MC._t0(b.L), b.motion)
        band, sq, l1 = band[wp.applied], sq[wp.applied], l1[wp.applied]
        for bd, s, at_least in ((3, 0, 100), (5, 0, 500), (7, 0, 500), (7, 1, 1000), (7, 2, 1000), (7, 3, 1000)):
            assert ((band == bd) & (sq == s)).sum() >= at_least, (bd, s)
        assert sq.max() == 3
        # Pade 7 below half of its norm bound: frexp's exponent is negative there and is clipped to 0 squarings
        assert ((band == 7) & (l1 < 0.5 * MC.PADE7_MAXNORM)).sum() >= 10
        # one batch, so events lie on both sides of each threshold; the nearest ones are close to it
        for thr in (MC.PADE3_BELOW, MC.PADE5_BELOW, MC.PADE7_MAXNORM, 2 * MC.PADE7_MAXNORM, 4 * MC.PADE7_MAXNORM):
            assert 0 < (thr - l1[l1 < thr]).min() < 0.01 * thr and 0 <= (l1[l1 >= thr] - thr).min() < 0.01 * thr


# ------------------------------------------------------------------ the gates
@pytest.mark.parametrize("W,H", SIZES)
def test_acceleration_gate_cases(oracle, oracle_planes, W, H):
    plain = None
    for name, warps in (("accel_5", False), ("accel_5_plus", True), ("accel_0", False)):
        c = MC.get(W, H, name)
        an = MC.motion_inputs(c.batches[0].motion)[3]
        assert (an == 5.0, an > 5) == {"accel_5": (True, False), "accel_5_plus": (False, True), "accel_0": (False, False)}[name]
        applied = sum(int(w.applied.sum()) for w in _warps(c))
        assert (applied > 30000) == warps and (applied == 0) == (not warps)
        plain = plain or _plain_planes(oracle, c)
        assert _same(oracle_planes(c), plain) == (not warps), name
    # above the gate the result is the warp's: the planes of the same motion with the usual acceleration
    assert _same(oracle_planes(MC.get(W, H, "accel_5_plus")), oracle_planes(MC.get(W, H, "dense_omega_9")))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("prefix", ["gate", "gate_epoch"])
def test_time_gate_cases(oracle, oracle_planes, W, H, prefix):
    c = MC.get(W, H, prefix + "_t1_on_event")
    b = c.batches[0]
    t0, t1 = MC._t0(b.L), b.motion["t1"]
    for cam, (ev, wp) in enumerate(zip((b.L, b.R), _warps(c))):
        et = event_times(ev)
        on = np.nonzero(et == t1)[0]
        assert len(on) == 1                                    # an event stamped t1 itself, in either stream
        i = int(on[0])
        assert (et[i] - t0) / (t1 - t0) == 1.0 and not wp.applied[i]
        inner = (ev["x"] > 6) & (ev["x"] <= W - 6) & (ev["y"] > 6) & (ev["y"] <= H - 6)
        assert inner[i] and np.array_equal(wp.applied, inner & (et < t1))
        assert wp.applied[:i].sum() > 10000 and (et[i + 1:] > t1).all() and len(et) - i > 3000
        # it would move if the gate let it through
        le = MC.warp64(ev, t0, b.motion, W, H, MC.EXACT._replace(time_le=True))
        assert le.applied[i] and le.sure[i] and (le.x[i], le.y[i]) != (ev["x"][i], ev["y"][i])
        if cam == 1:  # right events stamped before the first left one: a negative dt, warped
            early = et < t0
            assert early.sum() > 5000 and np.array_equal(wp.applied[early], inner[early])
            moved = (wp.x != ev["x"]) | (wp.y != ev["y"])
            assert (moved & early).sum() > 1000
    if prefix == "gate_epoch":  # et - t0 is quantised by the double: not whole microseconds
        dt_us = (event_times(b.L) - t0) * 1e6
        assert t0 > 1.6e9 and np.abs(dt_us - np.round(dt_us)).max() > 0.05
    else:
        dt_us = (event_times(b.L) - t0) * 1e6
        assert np.abs(dt_us - np.round(dt_us)).max() < 1e-3
    plain = _plain_planes(oracle, c)
    assert not _same(oracle_planes(c), plain)
    for name in ("_t1_eq_t0", "_t1_before_t0"):  # dt_batch == 0, < 0: nothing is warped
        z = MC.get(W, H, prefix + name)
        assert z.batches[0].L is b.L and z.batches[0].R is b.R
        assert (z.batches[0].motion["t1"] - t0 == 0) == (name == "_t1_eq_t0") and z.batches[0].motion["t1"] <= t0
        assert sum(int(w.applied.sum()) for w in _warps(z)) == 0
        assert _same(oracle_planes(z), plain)


# ------------------------------------------------------------------ the border band and the landing bound
@pytest.mark.parametrize("W,H", SIZES)
def test_frame_cases_reach_the_border_band_and_the_landing_bound(W, H):
    for name, inward_low in (("frame_pos", True), ("frame_neg", False)):
        c = MC.get(W, H, name)
        b = c.batches[0]
        for ev, wp in zip((b.L, b.R), _warps(c)):
            x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
            mid_y, mid_x = (y > 20) & (y < H - 20), (x > 20) & (x < W - 20)
            moved = wp.sure & ((wp.x != x) | (wp.y != y))
            for src, mid, N in ((x, mid_y, W), (y, mid_x, H)):
                # only 7 ... N - 6 are warped: the band is asymmetric
                for k, inside in ((6, False), (7, True), (N - 6, True), (N - 5, False)):
                    sel = (src == k) & mid
                    assert sel.sum() >= 100 and wp.applied[sel].all() == inside and wp.applied[sel].any() == inside
                # ... and the warped ones next to the band really move, on the side the motion carries inwards
                assert moved[(src == (7 if inward_low else N - 6)) & mid].sum() >= 100
            # the landing bound: floor(u) of 1 ... N - 2 is taken, 0 and N - 1 (and beyond) are refused
            with np.errstate(invalid="ignore"):
                fu, fv = np.floor(wp.u), np.floor(wp.v)
            for f, other_in, dst, N in ((fu, (fv > 0) & (fv < H - 1), wp.x, W), (fv, (fu > 0) & (fu < W - 1), wp.y, H)):
                near, far = (N - 2, N - 1) if inward_low else (1, 0)
                ok = wp.sure & wp.applied & other_in
                assert ((f == near) & ok).sum() >= 50 and (dst[(f == near) & ok] == near).all()
                assert ((f == far) & ok).sum() >= 50 and not moved[(f == far) & ok].any()
                assert ((f == (N if inward_low else -1)) & ok).sum() >= 50


# ------------------------------------------------------------------ division by zero, overflow
@pytest.mark.parametrize("W,H", SIZES)
def test_division_cases(oracle, oracle_planes, W, H):
    ex0, ey0 = W // 2 + 9, H // 2 - 3
    for name in ("div_zero", "div_zero_split", "div_negative", "div_huge"):
        c = MC.get(W, H, name)
        b = c.batches[0]
        om, vsum, (fx, fy, cx, cy), _ = MC.motion_inputs(b.motion)
        assert (om == 0).all() and fx == fy == 128.0 and cx == W // 2 and cy == H // 2
        assert vsum[2] == {"div_zero": 128, "div_zero_split": 128, "div_negative": 130, "div_huge": 128 - 2.0 ** -10}[name]
        for ev, wp in zip((b.L, b.R), _warps(c)):
            x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
            rows = wp.applied & (np.abs(y - H // 2) <= MC.DIV_ROWS)
            assert rows.sum() == 17 * (W - 12) and ((event_times(ev) - MC._t0(b.L))[rows] == 2.0 ** -6).all()
            u, v, w2 = wp.u[rows], wp.v[rows], wp.w2[rows]
            if name.startswith("div_zero"):
                assert (w2 == 0).all() and not np.isfinite(u).any() and not np.isfinite(v).any()
                nan_u, nan_v = np.isnan(u), np.isnan(v)
                if name == "div_zero":  # the numerator is 0 too on one column and one row: 0/0
                    assert np.array_equal(nan_u, x[rows] == ex0) and nan_u.sum() == 17
                    assert np.array_equal(nan_v, y[rows] == ey0) and nan_v.sum() == W - 12
                    assert wp.wild.sum() == 1 and (x[wp.wild], y[wp.wild]) == (ex0, ey0)
                else:
                    assert not nan_u.any() and not nan_v.any() and not wp.wild.any()
            elif name == "div_negative":
                assert (w2 == -2.0 ** -6).all() and (u < -64).all()
            else:
                assert (w2 == 2.0 ** -17).all() and np.isfinite(u).all() and (u > 2.0 ** 17).all()
            assert wp.sure[rows & ~wp.wild].all()
            assert np.array_equal(wp.x[rows], x[rows]) and np.array_equal(wp.y[rows], y[rows])  # they stay
            # the rest of the batch is not idle: events in front of the singular stamp zoom out and move
            assert (wp.sure & ((wp.x != x) | (wp.y != y))).sum() > 1000
        # the oracle leaves every one of them on its own pixel: the stamp t0 + 2^-6 is on no other pixel (and still on
        # most of their own: an event that moves may land on one later)
        t_div = MC._t0(b.L) + 2.0 ** -6
        for cam, ev in ((0, b.L), (1, b.R)):
            pl = oracle_planes(c)[cam]
            at = (pl[0] == t_div) | (pl[1] == t_div)
            want = np.zeros((H, W), bool)
            sel = event_times(ev) == t_div
            want[ev["y"][sel], ev["x"][sel]] = True
            assert sel.sum() >= 17 * W - 1 and not (at & ~want).any() and at.sum() > 0.5 * want.sum(), (name, cam)


# ------------------------------------------------------------------ many-to-one
@pytest.mark.parametrize("W,H", SIZES)
def test_many_to_one_case(oracle, W, H):
    c = MC.get(W, H, "many_to_one")
    assert "many_to_one" in MC.ORACLE_ONLY
    for bi, b in enumerate(c.batches):
        for cam, ev in ((0, b.L), (1, b.R)):
            wp = MC.warp64(ev, MC._t0(b.L), b.motion, W, H)
            moved = wp.sure & wp.applied & ((wp.x != ev["x"]) | (wp.y != ev["y"]))
            assert moved.sum() > 0.9 * wp.applied.sum()
            assert (wp.w2[wp.applied] > 1.45).all() and (wp.w2[wp.applied] < 2.55).all()
            key = wp.x[moved] + W * wp.y[moved]
            uniq, first, cnt = np.unique(key, return_index=True, return_counts=True)
            assert 3.0 < cnt.mean() < 6.0 and cnt.max() >= 8          # about four sources per target
            # on the shared targets: pairs inside and outside feature_filter_threshold, and of mixed polarity
            order = np.argsort(key, kind="stable")
            k, t, p = key[order], event_times(ev)[moved][order], ev["polarity"][moved][order]
            same = k[1:] == k[:-1]
            gap = np.abs(np.diff(t))[same]
            assert (gap < MC.FILTER_THRESHOLD).sum() > 1000 and (gap > MC.FILTER_THRESHOLD).sum() > 1000
            assert (np.diff(p.astype(np.int64))[same] != 0).sum() > 1000
            # stamps are shuffled against pixel order: the stream order on a target is not the raster order of the sources
            src = (ev["x"].astype(np.int64) + W * ev["y"].astype(np.int64))[moved][order]
            assert (np.diff(src)[same] < 0).sum() > 1000 and (np.diff(src)[same] > 0).sum() > 1000
    # sae_ differs from sae_latest_ and depends on the stream order; the second batch's result on the first's state
    b = c.batches[0]
    one = MC.oracle_planes(oracle, c, upto=1)
    two = MC.oracle_planes(oracle, c)
    for cam, ev in ((0, b.L), (1, b.R)):
        assert sum(int((one[cam][k] != one[cam][k + 2]).sum()) for k in (0, 1)) > 1000
        det = oracle.Detector(W, H)
        rev = ev[np.r_[0, len(ev) - 1:0:-1]]  # (the first left event stays first: it is the batch's t0)
        det.create_sae_mc(cam, rev, b.L[:1], oracle.make_motion(**b.motion))
        assert sum(int((det.get_sae(cam)[k + 2] != one[cam][k + 2]).sum()) for k in (0, 1)) > 100
        fresh = MC.Case("second only", W, H, c.batches[1:])
        assert sum(int((MC.oracle_planes(oracle, fresh)[cam][k + 2] != two[cam][k + 2]).sum()) for k in (0, 1)) > 100
        # float64's landing pixels of the sure events are the oracle's (those still readable from the planes)
        wp = MC.warp64(ev, MC._t0(b.L), b.motion, W, H)
        ox, oy = MC.landing_from_planes(ev, one[cam])
        known = (ox >= 0) & wp.sure
        assert known.sum() > 5000
        assert np.array_equal(ox[known], wp.x[known]) and np.array_equal(oy[known], wp.y[known])


# ------------------------------------------------------------------ the tiled update's tiles
@pytest.mark.parametrize("W,H", SIZES)
def test_large_rotations_leave_the_source_tile_in_every_direction(W, H):
    for name in MC.LEAVES_TILE:
        assert MC.tile_exits(MC.get(W, H, name)) == {"-x", "+x", "-y", "+y"}, name


# ------------------------------------------------------------------ the oracle against float64
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", MC.float64_case_names())
def test_oracle_planes_are_the_float64_planes_outside_the_unsure_set(oracle_planes, W, H, name):
    c = MC.get(W, H, name)
    bad = MC.mismatch64(c, oracle_planes(c))
    assert not bad, (len(bad), bad[0], MC.events_landing_on(c, bad[0][0], bad[0][2], bad[0][3]))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", MC.case_names())
def test_unsure_share_is_under_the_cap(W, H, name):
    share, unsure, applied = MC.unsure_share(MC.get(W, H, name))
    assert share <= MC.UNSURE_CAP, (unsure, applied)
    if name in MC.float64_case_names():  # the comparison is not hollow: nearly every pixel is compared
        for planes, mask, _, _ in MC.expected64(W, H, name):
            assert mask.sum() <= 0.02 * W * H


# ------------------------------------------------------------------ teeth
WRONG = {  # a deliberately wrong rule -> the cases on which the comparison with the oracle has to fail
    "R not transposed": (MC.EXACT._replace(transpose=False), ("dense_default", "dense_omega_9", "pade")),
    "translation dropped": (MC.EXACT._replace(translation=False), ("dense_v50", "div_zero", "div_negative")),
    "kBorder low side 5": (MC.EXACT._replace(border_lo=5), ("frame_pos",)),
    "kBorder low side 7": (MC.EXACT._replace(border_lo=7), ("frame_pos",)),
    "kBorder high side 5": (MC.EXACT._replace(border_hi=5), ("frame_neg",)),
    "kBorder high side 7": (MC.EXACT._replace(border_hi=7), ("frame_neg",)),
    "landing from 0": (MC.EXACT._replace(land_lo=-1), ("frame_neg",)),
    "landing from 2": (MC.EXACT._replace(land_lo=1), ("frame_neg",)),
    "landing to W-1": (MC.EXACT._replace(land_hi=0), ("frame_pos",)),
    "landing to W-3": (MC.EXACT._replace(land_hi=2), ("frame_pos",)),
    "time gate <= 1": (MC.EXACT._replace(time_le=True), ("gate_t1_on_event", "gate_epoch_t1_on_event")),
    "acceleration gate >= 5": (MC.EXACT._replace(accel_ge=True), ("accel_5",)),
}


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("wrong", list(WRONG))
def test_a_wrong_restatement_fails_the_comparison(oracle_planes, W, H, wrong):
    rules, names = WRONG[wrong]
    for name in names:
        c = MC.get(W, H, name)
        assert MC.mismatch64(c, oracle_planes(c), rules), (wrong, name)
