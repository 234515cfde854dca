"""CPU: the restatement tests/addr_filter_ref.py against answers derived by hand from the text of include/esvio_fe.h
(step 1a of the filter rule, hot-pixel learning and selection) — written out here, produced by no implementation — and
the figures about the shared inputs that the GPU tests rely on to be non-vacuous."""
import numpy as np

import addr_filter_cases as A
import addr_filter_ref as RA
import ba_filter2_ref as R2
import ba_filter_cases as K

W, H = A.W, A.H


def run(rows, stage, min_support=1, window=K.WINDOW, refractory=0, pol=None):
    ev = K.records(rows)
    if pol is not None:
        ev["polarity"] = pol
    B = RA.fresh_plane(W, H)
    flags, rej, by_stage = RA.filter_events(B, W, H, ev, window, min_support, refractory, stage)
    return ev, B, flags.tolist(), rej, by_stage


def test_a_masked_pixel_supports_nothing_and_stamps_nothing():
    rows = [(10, 10, 0, 100), (11, 10, 0, 200)]
    masked = RA.Stage(A.FULL, use_mask=1, mask=[A.pix((10, 10))])
    ev, B, flags, rej, by = run(rows, masked)
    assert flags == [0, 0] and rej == 1 and by == 1
    assert B[A.pix((10, 10))] == RA.NONE and B[A.pix((11, 10))] == 200
    assert run(rows, None)[2:4] == ([0, 1], 0)
    # use_mask with no mask set, and a mask that use_mask does not ask for, reject nothing
    assert run(rows, RA.Stage(A.FULL, use_mask=1, mask=None))[2:4] == ([0, 1], 0)
    assert run(rows, RA.Stage(A.FULL, use_mask=0, mask=[A.pix((10, 10))]))[2:4] == ([0, 1], 0)


def test_roi_edges_are_inclusive():
    x0, y0, x1, y1 = A.ROI
    stage = RA.Stage(A.ROI)
    corners = [(x0, y0), (x1, y0), (x0, y1), (x1, y1)]
    outside = [(x0 - 1, y0), (x0, y0 - 1), (x1 + 1, y0), (x1, y0 - 1), (x0 - 1, y1), (x0, y1 + 1), (x1 + 1, y1), (x1, y1 + 1)]
    rows = [(x, y, 0, 100 + i) for i, (x, y) in enumerate(corners + outside)]
    ev, B, flags, rej, by = run(rows, stage, min_support=0)
    assert flags == [1] * 4 + [0] * 8 and rej == 8 and by == 8
    assert sorted(np.flatnonzero(B != RA.NONE).tolist()) == sorted(A.pix(c) for c in corners)


def test_pixels_that_straddle_mask_words():
    assert [A.pix(p) for p in A.STRADDLE] == [31, 32, 63, 64, 1763] and (W * H + 31) // 32 == 56 and 1763 // 32 == 55
    rows = [(x, y, 0, 100 + i) for i, (x, y) in enumerate(A.STRADDLE)]
    for k, p in enumerate(A.STRADDLE):  # each masked alone: exactly that event goes
        stage = RA.Stage(A.FULL, use_mask=1, mask=[A.pix(p)])
        ev, B, flags, rej, by = run(rows, stage, min_support=0)
        assert flags == [int(j != k) for j in range(5)] and rej == 1
    ev, B, flags, rej, by = run(rows, RA.Stage(A.FULL, use_mask=1, mask=[A.pix(p) for p in A.STRADDLE]), min_support=0)
    assert flags == [0] * 5 and rej == 5 and (B == RA.NONE).all()


def test_polarity_suppression_and_flatten():
    rows = [(10, 10, 0, 100), (11, 10, 0, 200), (12, 10, 0, 300), (13, 10, 0, 400)]
    pol = [1, 0, 255, 0]  # ON = polarity byte != 0
    for mode, want in ((1, [1, 0, 1, 0]), (2, [0, 1, 0, 1])):
        for flatten in (0, 1, 2):
            stage = RA.Stage(A.FULL, polarity=mode, flatten=flatten)
            ev, B, flags, rej, by = run(rows, stage, min_support=0, pol=pol)
            assert flags == want and rej == 2
            kept, last = RA.kept_of(ev, np.array(flags), stage)
            src = [p for p, f in zip(pol, want) if f]
            assert kept[:, 12].tolist() == (src if flatten == 0 else [1 if flatten == 1 else 0] * 2)
            assert (kept[:, :12] == RA.raw_records(ev)[np.array(want) != 0][:, :12]).all() and last.tolist() == kept[-1].tolist()
    # a suppressed event between two supporters stamps nothing: (11,10) is OFF and goes, (12,10) finds no neighbour
    ev, B, flags, rej, by = run(rows[:3], RA.Stage(A.FULL, polarity=1), min_support=1, pol=[1, 0, 1])
    assert flags == [0, 0, 0] and rej == 1
    assert run(rows[:3], None, min_support=1, pol=[1, 0, 1])[2] == [0, 1, 1]


def test_without_a_stage_the_loop_is_ba_filter2_refs():
    for n in K.SWEEP_SIZES:
        ev = K.sweep_events(n)
        for prm in ((1_000_000, 1, 4_000_000), (0, 0, 4_000_000), (1_000_000, 2, 0)):
            Ba, Bb = RA.fresh_plane(W, H), R2.fresh_plane(W, H)
            fa, ra, by = RA.filter_events(Ba, W, H, ev, *prm)
            fb, rb = R2.filter_events(Bb, W, H, ev, *prm)
            assert by == 0 and ra == rb and np.array_equal(fa, fb) and np.array_equal(Ba, Bb)


def test_a_stage_equals_the_stream_without_its_rejected_events():
    """S with a stage == S' without one on a fresh plane: flags of the survivors, kept bytes, the plane afterwards"""
    streams = [A.with_outsiders(K.hot_pixel_events(), W, H), A.with_outsiders(A.uniform4097(), W, H)]
    stages = [RA.Stage(A.FULL, use_mask=1, mask=[A.pix(A.HOT)]), RA.Stage(A.ROI, polarity=1, flatten=2),
              RA.Stage(A.ROI, polarity=2, flatten=1, use_mask=1, mask=[A.pix((10, 10)), A.pix((20, 15))])]
    for ev in streams:
        for stage in stages:
            for prm in ((2000, 1, 4000), (0, 0, 0)):
                Ba, Bb = RA.fresh_plane(W, H), RA.fresh_plane(W, H)
                fa, ra, by = RA.filter_events(Ba, W, H, ev, *prm, stage=stage)
                prime = RA.without_stage(ev, stage, W, H)
                fb, rb, _ = RA.filter_events(Bb, W, H, prime, *prm)
                assert len(prime) == len(ev) - by and 0 < by < len(ev) and ra == rb + by
                xs, ys, ps = ev["x"].tolist(), ev["y"].tolist(), ev["polarity"].tolist()
                alive = np.array([not (xs[i] < W and ys[i] < H and stage.rejects(xs[i], ys[i], ps[i], W)) for i in range(len(ev))])
                assert np.array_equal(fa[alive], fb) and not fa[~alive].any()
                assert RA.kept_of(ev, fa, stage)[0].tobytes() == RA.kept_of(prime, fb)[0].tobytes()
                assert np.array_equal(Ba, Bb)


# ---- learning and selection on K.hot_pixel_events(): the figures, counted with numpy ---------------------------------
def _hot_stream_figures():
    ev = K.hot_pixel_events()
    t = ev["sec"].astype(np.int64) * 10 ** 9 + ev["nsec"].astype(np.int64)
    counts = np.bincount(ev["x"].astype(np.int64) + ev["y"].astype(np.int64) * W, minlength=W * H)
    return ev, t, counts


def test_the_hot_stream_is_what_the_selections_below_assume():
    ev, t, counts = _hot_stream_figures()
    assert len(ev) == 10_000 and int(t.max() - t.min()) == 15_063_000
    assert counts[A.pix(A.HOT)] == 5000
    ring = [counts[A.pix((20 + dx, 20 + dy))] for dx, dy in RA.NEIGHBOURS]
    assert min(ring) == 300 and max(ring) == 351
    rest = counts.copy()
    rest[[A.pix((20 + dx, 20 + dy)) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]] = 0
    assert rest.max() <= 22
    assert counts[A.pix((21, 19))] == 319 and counts[A.pix((21, 21))] == 319


def test_selections_by_hand():
    ev, t, counts = _hot_stream_figures()
    hot = RA.Hot(W, H)
    hot.learn(ev[:3000])
    hot.learn(ev[3000:])
    assert hot.N == 10_000 and hot.C == counts.tolist()
    xy, cnt, info = hot.select(8, min_rate_hz=100_000)
    assert info == dict(events=10_000, span_ns=15_063_000, threshold=1507, above=1, selected=1)
    assert xy == [(20, 20)] and cnt == [5000]
    xy, cnt, info = hot.select(4, min_rate_hz=10_000)
    assert info["threshold"] == 151 and info["above"] == 9 and info["selected"] == 4
    assert xy == [(20, 20), (20, 21), (19, 19), (21, 19)]  # (21,19) and (21,21) tie at 319: the lower index wins
    xy, cnt, info = hot.select(8, mean_factor=100)
    assert info["threshold"] == 567 == -(-100 * 10_000 // 1764) and info["above"] == 1 and xy == [(20, 20)]
    xy, cnt, info = RA.Hot(W, H).select(8)
    assert xy == [] and info == dict(events=0, span_ns=0, threshold=1, above=0, selected=0)


def test_out_of_sensor_and_bad_events_are_not_counted():
    ev = A.with_outsiders(A.uniform4097(), W, H)
    inside = (ev["x"] < W) & (ev["y"] < H)
    hot = RA.Hot(W, H)
    hot.learn(ev, bad=[5])
    assert inside[5] and hot.N == int(inside.sum()) - 1 and sum(hot.C) == hot.N


def test_figures_the_gpu_cases_rely_on():
    B = RA.fresh_plane(W, H)
    stage = RA.Stage(A.FULL, use_mask=1, mask=[A.pix(A.HOT)])
    assert RA.filter_events(B, W, H, K.hot_pixel_events(), 0, 0, 0, stage)[1:] == (5000, 5000)
    u = A.uniform4097()
    assert RA.filter_events(RA.fresh_plane(W, H), W, H, u, 0, 0, 0, RA.Stage(A.FULL, polarity=1))[1] == 4097 - 2098
    flags, rej, by = RA.filter_events(RA.fresh_plane(W, H), W, H, u, 0, 0, 0, RA.Stage(A.ROI))
    assert int(flags.sum()) == 824 and rej == 4097 - 824
