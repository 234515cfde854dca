"""The inputs of tests/lk_cases.py reach what they are for — checked with the oracle's trace alone (no GPU): these are
conditions on the inputs, not measurements of the code under test.  If one fails, the inputs are wrong, not the bound.
Also: the trace tap leaves oracle.lk's results as they are."""
import collections

import numpy as np
import pytest

import lk_cases as LC

ACCUMS = (1, 2)
TWO24 = float(1 << 24)


def _run(O, c, accum):
    return O.lk_trace(c.prev, c.next, c.pts, c.init, max_level=c.max_level, max_count=c.max_count, eps=c.eps,
                      flags=c.flags, accum=accum)


@pytest.fixture(scope="module")
def traces(oracle):
    """every oracle-free case, traced once per mode of the sums: {class: [(case, {accum: (pts, status, trace)})]}"""
    out = collections.defaultdict(list)
    for c in LC.all_cases_without_oracle():
        out[c.name.split("/")[0]].append((c, {a: _run(oracle, c, a) for a in ACCUMS}))
    return out


def test_trace_leaves_the_results_alone(oracle, traces):
    for cls in traces.values():
        for c, runs in cls[::3]:
            for a in ACCUMS + (0, 4):
                p, s, _ = runs[a] if a in runs else _run(oracle, c, a)
                q, t = oracle.lk(c.prev, c.next, c.pts, c.init, max_level=c.max_level, max_count=c.max_count,
                                 eps=c.eps, flags=c.flags, accum=a)
                assert np.array_equal(s, t) and np.array_equal(p.view(np.uint32), q.view(np.uint32)), (c.name, a)


def test_restage_windows_leave_the_staged_tile(oracle, traces):
    assert len(traces["restage"]) == 2 * len(LC.RESTAGE_SHIFTS)
    for a in ACCUMS:
        seen = np.zeros(4, bool)  # right, left, down, up
        for c, runs in traces["restage"]:
            _, st, t = runs[a]
            far = np.zeros((len(c.pts), 4), bool)
            for i in range(len(c.pts)):
                ix = t.inext[i, 0, :max(int(t.iters[i, 0]), 1)].astype(np.int64)
                dx, dy = ix[:, 0] - ix[0, 0], ix[:, 1] - ix[0, 1]
                far[i] = (dx.max() > 12, dx.min() < -12, dy.max() > 6, dy.min() < -6)
            good = far.any(1) & (st == 1)
            assert good.sum() >= 32, (c.name, a, int(good.sum()))
            seen |= far[good].sum(0) >= 32
        assert seen.all(), (a, seen)


def test_borders_reach_every_limit(oracle, traces):
    E = oracle.LK_EXIT
    for a in ACCUMS:
        xs, ys = set(), set()
        n_start = n_outside = n_final = 0
        at_minus_win, at_size = np.zeros(2, int), np.zeros(2, int)  # (x, y) counted apart: the kernel tests them apart
        for c, runs in traces["borders"]:
            _, st, t = runs[a]
            H, W = c.prev.shape
            o = np.floor(c.pts.astype(np.float64) - 10).astype(int)
            xs |= set(o[:, 0].tolist())
            ys |= set(o[:, 1].tolist())
            for i in np.nonzero((t.exit[:, 0] >= 0))[0]:  # level 0: its first iteration's origin is the point's own
                if c.max_level == 0 and t.exit[i, 0] not in (E["window_out_at_start"], E["eig"]):
                    assert tuple(t.inext[i, 0, 0]) == tuple(o[i])
            e0 = t.exit[:, 0]
            n_start += int((e0 == E["window_out_at_start"]).sum())
            n_outside += int(((e0 == E["outside"]) & (t.iters[:, 0] > 0)).sum())
            n_final += int(((e0 != E["window_out_at_start"]) & (e0 != E["eig"]) & (e0 != E["outside"]) & (st == 0)).sum())
            for i in range(len(c.pts)):
                n = int(t.iters[i, 0])
                if n > 1:  # a window that sits ON the last allowed origin in the middle of a run
                    at_minus_win += (t.inext[i, 0, 1:n] == -LC.WIN).any(0)
                if n > 0 and e0[i] == E["outside"]:  # ... and one that stops ON the first forbidden one
                    at_size += t.inext[i, 0, n] == (W, H)
        assert set(LC.border_origins(96)) <= xs and set(LC.border_origins(80)) <= ys
        assert n_start >= 10 and n_outside >= 10 and n_final >= 10, (a, n_start, n_outside, n_final)
        assert at_minus_win.min() >= 10 and at_size.min() >= 10, (a, at_minus_win, at_size)


def test_termination_takes_every_exit(oracle, traces):
    E = oracle.LK_EXIT
    T = np.float32(0.01)
    for a in ACCUMS:
        exits = collections.Counter()
        for c, runs in traces["termination"]:
            p, st, t = runs[a]
            exits.update(t.exit[t.exit >= 0].tolist())
            if min(max(c.max_count, 0), 100) == 0:  # no iterations: every point stays where it started
                assert (t.iters == 0).all()
                assert np.array_equal(p.view(np.uint32), c.pts.view(np.uint32)), c.name
            if c.name.endswith("same_image/eps0"):  # d = 0 exactly: converged at once even with eps 0
                conv = t.exit[:, 0] == E["converged"]
                assert conv.sum() >= 30 and (t.iters[conv, 0] == 1).all() and not t.delta[conv, 0, 0].any()
        for name in oracle.LK_EXITS:
            assert exits[E[name]] >= 10, (a, name, exits)
        # the oscillation test at its limit: |d + prevD| equal to 0.01f, the largest float it accepts
        c, runs = [x for x in traces["termination"] if x[0].name.endswith("oscillation_sum_is_0.01f")][0]
        _, _, t = runs[a]
        d = t.delta[:, 0]
        hit = (t.exit[:, 0] == E["oscillation"]) & (np.abs(d[:, 0, 0] + d[:, 1, 0]) == T) & \
            (np.abs(d[:, 0, 1] + d[:, 1, 1]) <= T)
        assert hit.sum() >= 2, (a, hit)


@pytest.mark.parametrize("accum", ACCUMS)
def test_tiebreak_cannot_be_decided_in_fp32(oracle, accum):
    E = oracle.LK_EXIT
    tb = LC.tiebreak_cases(oracle, accum)
    pairs = collections.defaultdict(list)
    for c, p, k, d2k, stops in tb:
        assert stops == (d2k <= c.eps * c.eps)
        _, _, t = _run(oracle, c, accum)
        dx, dy = (float(v) for v in t.delta[0, 0, k])
        assert float(dx) * dx + float(dy) * dy == d2k  # the same run up to k, whatever eps is
        stopped_at_k = t.exit[0, 0] == E["converged"] and t.iters[0, 0] == k + 1
        assert stopped_at_k == stops, (c.name, t.exit_name(0, 0), int(t.iters[0, 0]))
        assert t.iters[0, 0] >= k + 1
        # the kernel's pre-test: d2 = fma(dx, dx, dy * dy) in fp32 against eps^2 (1 -+ 2^-20)
        d2f = float(np.float32(dx * dx + float(np.float32(dy) * np.float32(dy))))
        assert abs(d2f / (c.eps * c.eps) - 1) < 2.0 ** -21, c.name
        pairs[c.name.split("/eps")[0]].append(stops)
        if "/on_minus_win/" in c.name and not stops:  # the run goes on from a window ON x origin -WIN
            assert t.iters[0, 0] > k + 1 and t.inext[0, 0, k + 1, 0] == -LC.WIN, c.name
    assert len([key for key in pairs if "/on_minus_win/" not in key]) >= 20
    assert len([key for key in pairs if "/on_minus_win/" in key]) >= LC.TIEBREAK_ON_MINUS_WIN
    for key, outcomes in pairs.items():
        assert len(outcomes) == 5 and True in outcomes and False in outcomes, key


def test_saturated_sums_reach_the_top_of_their_range(oracle, traces):
    amax = 0.0
    for c, runs in traces["saturated"]:
        p1, s1, t1 = runs[1]
        p2, s2, t2 = runs[2]
        amax = max(amax, float(t1.A[:, :, 0].max()), float(t1.A[:, :, 2].max()))
        # the trace's own layout of the float chains reproduces the float-order b sums of every iteration, bit for bit
        assert (t2.sat >= 0).all(), c.name
        early = 0  # iterations in which a float chain passes 2^24 before its last third
        for i in range(len(c.pts)):
            for L in range(4):
                early += int((t2.sat[i, L, :int(t2.iters[i, L])] < 2 / 3).sum())
        differ = int((p1.view(np.uint32) != p2.view(np.uint32)).any(1).sum())
        kind = c.name.split("/")[1]
        if kind == "stripes4":  # rank 1 at the largest A11 there is: nobody passes the gate
            assert not s1.any() and not s2.any()
            assert (t1.exit[:, 0] <= oracle.LK_EXIT["eig"]).all()
        else:
            assert early >= 100, (c.name, early)
            assert differ >= 10, (c.name, differ)
            assert max(t1.bmax.max(), t2.bmax.max()) > TWO24
        if kind in ("checker3", "blocks5", "noise"):
            assert s1.sum() >= 30 and s2.sum() >= 30, c.name
    assert amax >= 0.9 * 441 * 4080.0 ** 2 / (1 << 20)


def test_sizes_run_the_levels_they_should(oracle, traces):
    E = oracle.LK_EXIT
    want = {"sizes/42x42": 0, "sizes/43x50": 1, "sizes/61x47": 1, "sizes/173x131": 2, "sizes/346x260/quarters": 3}
    for c, runs in traces["sizes"]:
        for a in ACCUMS:
            _, st, t = runs[a]
            H, W = c.prev.shape
            top = oracle.pyr_levels(W, H)
            assert top == want[c.name]
            assert (t.exit[:, :top + 1] >= 0).all() and (t.exit[:, top + 1:] < 0).all()
            if c.name.endswith("quarters"):  # the gate fails above level 0 and passes there
                above = (t.exit[:, 1:] == E["eig"]).any(1) & (t.exit[:, 0] > E["eig"])
                ran_above = (t.exit[:, 1:] > E["eig"]).any(1)
                assert above.sum() >= 32 and (above & ran_above).sum() >= 10 and st[above].sum() >= 32
            else:
                assert st.sum() >= 30


def test_counts_and_class_sizes():
    cases, too_many = LC.counts_cases()
    assert [len(c.pts) for c in cases] == [1, 2, 3, 4, 5, 7, 8, 9, 11, 12] and len(too_many.pts) == 13
    every = LC.all_cases_without_oracle()
    assert max(len(c.pts) for c in every) <= LC.MAX_POINTS
    assert max(c.prev.shape[1] for c in every) <= LC.LARGEST[0] and max(c.prev.shape[0] for c in every) <= LC.LARGEST[1]
    assert len({c.name for c in every}) == len(every)


@pytest.mark.parametrize("kind", ["blocks", "noise"])
def test_saturated_sequence_keeps_tracks(oracle, kind):
    """the trackImage sequence of test_lk_edges_gpu.py is worth comparing: tracks survive it"""
    frames = LC.saturated_sequence(kind)
    for a in ACCUMS:
        tr = oracle.Tracker(oracle.make_config(160, 120, lk_accum=a, **LC.SEQUENCE_CONFIG))
        for f, img in enumerate(frames):
            r = tr.track_image(0.05 * (f + 1), img, None, True)
        assert (r.track_cnt >= 3).sum() >= 20, (kind, a, len(r.ids))
