"""CPU: the numpy restatement of the event images (tests/event_image_ref.py) against answers derived by hand, the
designed inputs (tests/event_image_cases.py) against the edges they are named for, and the restatement's tie to the
oracle: which pixels a batch touches and which polarity came last are what the oracle's sae_latest planes say, and the
warped pixels of the motion-compensated cases are read off the oracle's planes, event by event."""
import numpy as np

import event_image_cases as K
import event_image_ref as R
from esvio_amd.events import event_times, make_events

B, G, Rd = (255, 0, 0), (0, 0, 0), (0, 0, 255)  # ON, nothing, OFF as (B, G, R)


def test_hand_derived_three_events_on_two_pixels():
    # (1,0) ON, (2,1) ON, then (1,0) OFF: the later event wins at (1,0)
    ev = make_events([1, 2, 1], [0, 1, 0], [10, 20, 30], [1, 1, 0])
    want = np.array([[G, Rd, G], [G, G, B]], np.uint8)
    assert np.array_equal(R.event_image(ev, 3, 2), want)
    # stamps are never looked at: the same events with the stamps reversed give the same image
    ev2 = make_events([1, 2, 1], [0, 1, 0], [30, 20, 10], [1, 1, 0])
    assert np.array_equal(R.event_image(ev2, 3, 2), want)


def test_hand_derived_out_of_sensor_event_writes_nothing():
    ev = make_events([3, 0, 0, 65535], [0, 2, 1, 65535], [1, 2, 3, 4], [1, 1, 0, 1])  # x = W, y = H, one inside, 65535
    want = np.array([[G, G, G], [Rd, G, G]], np.uint8)
    assert np.array_equal(R.event_image(ev, 3, 2), want)


def test_hand_derived_accumulate_against_fresh():
    a = make_events([0, 1], [0, 0], [1, 2], [1, 1])
    b = make_events([1, 2], [0, 0], [3, 4], [0, 0])
    first = R.event_image(a, 3, 1)
    assert np.array_equal(first, np.array([[B, B, G]], np.uint8))
    assert np.array_equal(R.event_image(b, 3, 1, base=first), np.array([[B, Rd, Rd]], np.uint8))  # a stage call keeps (0,0)
    assert np.array_equal(R.event_image(b, 3, 1), np.array([[G, Rd, Rd]], np.uint8))              # a track call does not
    assert np.array_equal(first, np.array([[B, B, G]], np.uint8))  # the base is not written
    # pixels: the override, and the drop mark
    assert np.array_equal(R.event_image(a, 3, 1, pixels=[(2, 0), (-1, -1)]), np.array([[G, G, B]], np.uint8))
    assert np.array_equal(R.canvas(first, first), np.array([[B, B, G, B, B, G]], np.uint8))


def test_each_designed_case_reaches_the_edge_it_is_named_for():
    W, H = K.W, K.H
    assert (W * H) % 4 != 0 and (W * 3) % 4 != 0 and W * H > 4 * 256  # a tail group, unaligned rows, several emit blocks
    assert K.SMALL[0] * K.SMALL[1] % 4 == 0  # ... and the small handle has none: both forms of the end
    assert set(K.COUNTS) >= {0, 1, 255, 256, 257} and max(K.COUNTS) > 4 * 256
    assert max(K.COUNTS) > W * H > 257  # one camera's 5000 events take the mark kernel's skipping form, 257 do not
    assert [(a > W * H * (1 + (b > 0))) for a, b in [(nl + nr, nr) for nl, nr in K.THRESHOLD]] == [False, True, False, True]
    Lm, Rm, _ = K.mc_batch()
    assert len(Lm) + len(Rm) > 2 * W * H > 2000 and (Lm["x"][:1000] < W).all() and (Rm["x"][:1000] < W).all()
    for name, (L, Rt) in K.counts().items():
        assert len(L) == len(Rt) == int(name[1:])
        if len(L) > 1:
            assert not np.array_equal(L["x"], Rt["x"])
    for last_on in (True, False):
        ev = K.contention(last_on)
        assert len(ev) == 5000 and set(zip(ev["x"].tolist(), ev["y"].tolist())) == {K.HOT}
        assert (ev["polarity"][1:] != ev["polarity"][:-1]).all() and bool(ev["polarity"][-1]) == last_on
        img = R.event_image(ev, W, H)
        assert tuple(img[K.HOT[1], K.HOT[0]]) == (R.ON if last_on else R.OFF) and np.count_nonzero(img.any(axis=2)) == 1
    st = K.stamps()
    t = {k: event_times(v) for k, v in st.items()}
    assert len(np.unique(t["equal"])) == 1 and (np.diff(t["decreasing"]) < 0).all()
    d = np.diff(t["step_back"])
    assert (d < -0.9).sum() == 1 and (np.delete(d, np.argmin(d)) > 0).all()
    imgs = [R.event_image(v, W, H) for v in st.values()]
    assert all(np.array_equal(imgs[0], i) for i in imgs[1:])  # stream order, whatever the stamps say
    # ... and stream order is not what the stamps would give: by decreasing stamps the FIRST event of a pixel is the latest
    ev = st["decreasing"]
    first_wins = R.event_image(ev[::-1], W, H)
    assert not np.array_equal(first_wins, imgs[0])
    pix = ev["y"].astype(int) * W + ev["x"]
    assert np.bincount(pix).max() > 8  # pixels hit many times
    c = K.corners()
    assert sorted(zip(c["x"].tolist(), c["y"].tolist())) == sorted([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)])
    assert c["polarity"].max() == 255
    lp = K.last_pixel()
    assert int(lp["y"][0]) * W + int(lp["x"][0]) == W * H - 1 >= 4 * (W * H // 4)  # in the group the padding completes
    o = K.out_of_sensor()
    assert {W, 65535} <= set(o["x"].tolist()) and {H, 65535} <= set(o["y"].tolist())
    inside = (o["x"] < W) & (o["y"] < H)
    assert inside.sum() == 2 and np.count_nonzero(R.event_image(o, W, H).any(axis=2)) == 2
    assert ((o["x"] >= W) & (o["y"] < H)).any() and ((o["x"] < W) & (o["y"] >= H)).any()


def test_the_restatement_is_tied_to_the_oracles_sae_latest_planes(oracle):
    W, H = K.W, K.H
    for seed, n in ((1, 257), (2, 5000)):
        ev = K.uniform(n, seed)
        ev["x"][n // 3], ev["y"][n // 2] = W, H  # two the update skips
        assert (np.diff(event_times(ev)) > 0).all()
        fresh, det = oracle.Detector(W, H), oracle.Detector(W, H)
        det.create_sae(0, ev)
        f0, f1 = fresh.get_sae(0)[:2]
        l0, l1 = det.get_sae(0)[:2]  # sae_latest of polarity 0 and 1
        img = R.event_image(ev, W, H)
        touched = (l0 != f0) | (l1 != f1)
        assert np.array_equal(img.any(axis=2), touched) and touched.sum() > 0
        on = l1 > l0  # strictly increasing stamps: the larger stamp is the later event
        assert (img[touched & on] == R.ON).all() and (img[touched & ~on] == R.OFF).all()
        assert (touched & on).any() and (touched & ~on).any()


def test_the_motion_compensated_pixels_come_from_the_oracle_and_a_quarter_of_them_move(oracle):
    L, Rt, t1, m, pxL, pxR = K.mc_case(oracle)
    assert np.sqrt(sum(a * a for a in K.MC["accel"])) > 5
    for ev, px in ((L, pxL), (Rt, pxR)):
        inside = (ev["x"] < K.W) & (ev["y"] < K.H)
        assert (~inside).sum() == 1 and (px[~inside] == -1).all()  # the out-of-sensor event left no pixel
        assert (px[inside] >= 0).all()  # the warp drops none
        moved = (px[:, 0] != ev["x"]) | (px[:, 1] != ev["y"])
        share = (moved & inside).sum() / inside.sum()
        assert share >= 0.25, share
        # the image at the warped pixels differs from the one at the events' own
        assert not np.array_equal(R.event_image(ev, K.W, K.H, pixels=px), R.event_image(ev, K.W, K.H))
    # without |accel| > 5 the oracle writes every event at its own pixel
    still = oracle.make_motion(t1, K.MC["v"], K.MC["v_pre"], (0, 0, 1.0), K.MC["omega"], K.MC["fx"], K.MC["fy"], K.MC["cx"], K.MC["cy"])
    px0 = K.oracle_pixels(oracle, L[:200], L[:1], still, 0)
    assert np.array_equal(px0[:, 0], L["x"][:200]) and np.array_equal(px0[:, 1], L["y"][:200])
