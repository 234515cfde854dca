"""The motion-compensated SAE write on the device (k_mc_warp, k_sae_keys<true>, the tiled update, fe_mc.h) on the
designed inputs of tests/mc_cases.py, through all three forms of the update: held to the oracle bit for bit on all four
planes of both cameras, and -- because the oracle states the same float arithmetic from the same recollection -- held
to the module's float64 restatement (closed-form rotation, float64 throughout) on every pixel outside the set that
events within DELTA of an integer may touch.  There a transposed R, a wrong Pade coefficient, a dropped squaring or an
off-by-one in a gate cannot hide behind an oracle that shares it.  tests/test_mc_cases.py shows on the CPU that the
cases reach the edges they are for and that wrong variants of the restatement fail the same comparison."""
import numpy as np
import pytest

from esvio_amd import frontend as FE
from esvio_amd.events import event_times

import mc_cases as MC
from test_parity_gpu import SAE_PATHS

pytestmark = pytest.mark.gpu

PLANES = ("L0", "L1", "S0", "S1")


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's planes after each batch of a case, computed once per case"""
    done = {}

    def get(case):
        key = (case.W, case.H, case.name)
        if key not in done:
            done[key] = [MC.oracle_planes(oracle, case, upto=k + 1) for k in range(len(case.batches))]
        return done[key]
    return get


def _first_difference(case, got, exp, batch):
    """None, or the first pixel at which the device's planes differ from the oracle's, with the events that land there"""
    for cam in (0, 1):
        for k, name in enumerate(PLANES):
            bad = np.argwhere(got[cam][k] != exp[cam][k])
            if len(bad):
                y, x = (int(v) for v in bad[0])
                ev = MC.events_landing_on(MC.Case(case.name, case.W, case.H, case.batches[batch:]), cam, x, y)
                return "%s %dx%d batch %d, camera %d plane %s: %d pixels differ; first (x, y) = (%d, %d): %r, the oracle's %r; " \
                       "events float64 puts there: %r" % (case.name, case.W, case.H, batch, cam, name, len(bad), x, y,
                                                          got[cam][k][y, x], exp[cam][k][y, x], ev)
    return None


@pytest.mark.parametrize("W,H", MC.SIZES)
@pytest.mark.parametrize("name", MC.case_names())
@pytest.mark.parametrize("path", list(SAE_PATHS))
def test_createSAE_stereo_mc_on_the_designed_cases(want, path, name, W, H, monkeypatch):
    """createSAE_stereo_mc into a fresh handle: the oracle's planes bit for bit; the float64 planes outside the unsure
    set (every case but the ones named in mc_cases.ORACLE_ONLY: many_to_one, whose two batches run in a row)"""
    for k, v in SAE_PATHS[path].items():
        monkeypatch.setenv(k, v)
    case = MC.get(W, H, name)
    if path == "tiled" and name in MC.LEAVES_TILE:  # warped events leave their source tile in every direction
        assert MC.tile_exits(case) == {"-x", "+x", "-y", "+y"}
    ft = FE.FeatureTracker(FE.make_config(W, H))
    try:
        for bi, b in enumerate(case.batches):
            assert ft.detector.createSAE_stereo_mc(b.L, b.R, FE.make_motion(**b.motion)) == 0
            got = [ft.detector.get_sae(0), ft.detector.get_sae(1)]
            diff = _first_difference(case, got, want(case)[bi], bi)
            assert diff is None, diff
            if bi == 0 and name not in MC.ORACLE_ONLY:
                bad = MC.mismatch64(case, got)
                assert not bad, "%s %dx%d: %d pixels outside the unsure set differ from float64; first %r; events there: %r" % (
                    name, W, H, len(bad), bad[0], MC.events_landing_on(case, bad[0][0], bad[0][2], bad[0][3]))
    finally:
        ft.close()


@pytest.mark.parametrize("W,H", MC.SIZES)
@pytest.mark.parametrize("name", ["div_zero", "div_huge", "gate_t1_on_event", "gate_epoch_t1_on_event"])
def test_trackEvent_with_measurements_survives_and_leaves_the_oracles_planes(oracle, name, W, H):
    """one trackEvent with a Motion_correction_value on the cases whose warps divide by zero, overflow, or sit on the
    time gate: the call returns, and planes, time surfaces and result members are oracle.Tracker.track_event's"""
    b = MC.get(W, H, name).batches[0]
    ft = FE.FeatureTracker(FE.make_config(W, H))
    tr = oracle.Tracker(oracle.make_config(W, H))
    try:
        t = float(event_times(b.L)[-1])
        ft.trackEvent(t, b.L, b.R, True, measurements=FE.make_motion(**b.motion))
        r = tr.track_event(t, b.L, b.R, True, motion=oracle.make_motion(**b.motion))
        for cam in (0, 1):
            for k, (g, e) in enumerate(zip(ft.detector.get_sae(cam), tr.detector().get_sae(cam))):
                assert np.array_equal(g, e), (cam, PLANES[k], int((g != e).sum()))
            assert np.array_equal(ft.gettimesurface(cam), tr.time_surface(cam)), cam
        assert np.array_equal(ft.ids, r.ids) and np.array_equal(ft.track_cnt, r.track_cnt)
        assert np.array_equal(ft.ids_right, r.ids_right)
        for k in ("cur_pts", "cur_un_pts", "pts_velocity", "cur_right_pts", "cur_un_right_pts", "right_pts_velocity"):
            g, e = getattr(ft, k), getattr(r, k)
            assert g.shape == e.shape and np.array_equal(g.view(np.uint32), e.view(np.uint32)), k
    finally:
        ft.close()
