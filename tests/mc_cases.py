"""Designed inputs for the motion-compensated SAE write and a float64 restatement of it, with no device code.

The write under test: trackEvent's per-event gate (feature_tracker.cpp:627-641), createSAE_left/right with a
Motion_correction_value (event_detector.cc:102-147, :168-210) and motioncorrection (:547-591) -- the warp
K * exp([omega*dt]x)^T * K^-1 plus the translation term, the kBorder band in front of it and the landing bound behind.

The device (esvio_amd/csrc/fe_mc.h) and the oracle (oracle/esvio_oracle.cpp, m3_* / motion_correct) state Eigen's float
arithmetic twice from the same recollection, so "device == oracle" shows only that the two copies agree.  warp64() here
is a third statement that shares nothing with them but the inputs: the rotation in closed form (Rodrigues), everything
in float64, vectorised over the events.  It cannot be bit-equal to float arithmetic, so it says per event whether it is
SURE: u and v farther than a band from every integer, and no gate decided inside the band.  An unsure event comes with
the set of pixels it may be written to, and planes64() leaves those pixels out of the comparison.

The band is measured, not chosen (measure(), `python tests/mc_cases.py`): the largest distance to an integer of any
event that the oracle writes to another pixel than float64 does, times 4, rounded up to a power of two.

tests/test_mc_cases.py checks on the CPU that every case reaches the edge it is named for and that the oracle's planes
are the float64 planes outside the unsure set; tests/test_mc_edges_gpu.py runs the cases through the kernels.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

if __name__ == "__main__":  # `python tests/mc_cases.py`: the measurement; the tests get the path from conftest.py
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from esvio_amd.events import EVENT_DTYPE, event_times, make_events

SIZES = ((176, 176), (169, 169), (200, 169))  # the two smallest event-handle sizes of the suite + a non-square one
TILE = (32, 16)                  # the tiled update's tile at these sizes (make_tile_geom)
FILTER_THRESHOLD = 0.01          # feature_filter_threshold of a default handle
BASE_US = 5_000_000
EPOCH_US = 1_700_000_000_000_000
SPAN_US = 40_000                 # a batch's stamps: distinct microseconds inside 40 ms

# Matrix3f::exp()'s branches by the L1 norm of the skew matrix (unsupported/Eigen/MatrixFunctions, float)
PADE3_BELOW = np.float32(4.258730016922831e-001)
PADE5_BELOW = np.float32(1.880152677804762e+000)
PADE7_MAXNORM = np.float32(3.925724783138660)

# `python tests/mc_cases.py`: over every case compared with float64, the largest distance to an integer (divided by
# (1 + |u| / N) / |w|, as the band of _axis grows with them) of an event whose landing pixel differs between the oracle and warp64: 158 of 3 825 670 events
# differ, the farthest of them by MEASURED_DISAGREEMENT.  DELTA = 4 * that, rounded up to a power of two: the device's
# float rounding may differ from x86's only if something is wrong, and the factor guards against the cases' own spread.
MEASURED_DISAGREEMENT = 2.251e-05  # px
DELTA = 2.0 ** -13              # 1.22e-4 px
UNSURE_CAP = 0.02                # at most this share of a case's warped events may be unsure
ORACLE_ONLY = ("many_to_one",)   # cases compared with the oracle only (many_to_one by design: the order on a pixel
#                                  needs every event sure; a case that cannot stay under UNSURE_CAP would be named here)

# the rules of the write, as parameters: EXACT is the reference's; tests/test_mc_cases.py flips one at a time and
# expects the comparison with the oracle to fail
Rules = namedtuple("Rules", "transpose translation border_lo border_hi land_lo land_hi time_le accel_ge")
EXACT = Rules(transpose=True, translation=True, border_lo=6, border_hi=6, land_lo=0, land_hi=1, time_le=False,
              accel_ge=False)

Batch = namedtuple("Batch", "L R motion")        # events of both cameras + make_motion's keyword arguments
Case = namedtuple("Case", "name W H batches")
Warp = namedtuple("Warp", "applied u v w2 x y sure may wild")


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def motion_inputs(motion):
    """the numbers of a Motion_correction_value as the code takes them: rounded to float first"""
    om = _f32(motion["omega"]).astype(np.float64)
    vsum = (_f32(motion["v"]) + _f32(motion["v_pre"])).astype(np.float64)  # Vector3f + Vector3f
    fx, fy, cx, cy = (float(np.float32(motion[k])) for k in ("fx", "fy", "cx", "cy"))
    a = _f32(motion["accel"]).astype(np.float64)
    an = np.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2)  # sqrt(pow(double) + ...) (event_detector.cc:125)
    return om, vsum, (fx, fy, cx, cy), an


def rotation64(r):
    """exp([r]x) for rotation vectors r (n,3): I + sin(t)/t S + (1-cos(t))/t^2 S^2, the series where t -> 0"""
    r = np.asarray(r, np.float64).reshape(-1, 3)
    t2 = (r * r).sum(1)
    t = np.sqrt(t2)
    small = t < 1e-3
    ts = np.where(small, 1.0, t)
    A = np.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, np.sin(ts) / ts)
    B = np.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 2.0 * np.sin(0.5 * ts) ** 2 / (ts * ts))
    S = np.zeros((len(r), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -r[:, 2], r[:, 1]
    S[:, 1, 0], S[:, 1, 2] = r[:, 2], -r[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -r[:, 1], r[:, 0]
    return np.eye(3)[None] + A[:, None, None] * S + B[:, None, None] * (S @ S)


def _axis(wn, w2, N, delta, ez, rules):
    """one coordinate c = wn / w2 with |error(wn)| <= delta and |error(w2)| <= ez: the integer interval floor(c) may
    lie in, whether all of it passes the landing bound (motioncorrection :574) and whether none of it does"""
    with np.errstate(all="ignore"):
        straddle = ~(np.abs(w2) > ez)      # the sign of w2 is open (or w2 is not a number): c may be anything
        c = wn / w2
        band = (delta + np.abs(c) * ez) / (np.abs(w2) - ez)
        lo, hi = np.floor(c - band), np.floor(c + band)
        lo_bound, hi_bound = rules.land_lo, N - rules.land_hi   # a pixel k lands iff lo_bound < k < hi_bound
        all_in = ~straddle & (lo > lo_bound) & (hi < hi_bound)
        all_out = np.where(straddle, np.abs(wn) - delta > N * (np.abs(w2) + ez), (hi <= lo_bound) | (lo >= hi_bound))
        all_out = all_out | (~straddle & ~np.isfinite(c))
    return c, lo, hi, all_in, all_out, straddle


def warp64(ev, t0, motion, W, H, rules=EXACT, delta=DELTA):
    """float64 restatement of the gate + motioncorrection for the events `ev` of one camera; t0 = the first LEFT
    event's time.  Returns a Warp of per-event arrays: applied (the event passed the time, acceleration and border
    gates, so the warp formula decides its pixel), u, v, w2 (the real warped coordinates and the homogeneous
    coordinate; nan where not applied), x, y (the landing pixel), sure, and for the unsure events `may`: {event index:
    [(x, y), ...]}, the pixels it may be written to.  wild: unsure events whose coordinates are not bounded at all
    (0/0); their `may` holds their own pixel only."""
    om, vsum, (fx, fy, cx, cy), an = motion_inputs(motion)
    n = len(ev)
    ex, ey = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    et = event_times(ev)
    dt = et - t0
    dtb = float(motion["t1"]) - t0
    with np.errstate(all="ignore"):
        ratio = dt / dtb
    in_time = (dtb > 0) & ((ratio <= 1) if rules.time_le else (ratio < 1))
    active = (an >= 5) if rules.accel_ge else (an > 5)
    in_border = (ex > rules.border_lo) & (ex <= W - rules.border_hi) & (ey > rules.border_lo) & (ey <= H - rules.border_hi)
    applied = in_time & active & in_border

    R = rotation64(om[None, :] * dt[:, None])
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Kinv = np.array([[1.0 / fx, 0, -cx / fx], [0, 1.0 / fy, -cy / fy], [0, 0, 1.0]])
    rot_K = K[None] @ (R.transpose(0, 2, 1) if rules.transpose else R) @ Kinv[None]
    kt = (0.5 * dt[:, None] * vsum[None, :]) @ Kinv.T
    e = np.stack([ex, ey, np.ones(n)], 1).astype(np.float64)
    w = (rot_K @ e[:, :, None])[:, :, 0]
    if rules.translation:
        w = w - (rot_K @ kt[:, :, None])[:, :, 0]

    ez = delta / max(W, H)
    u, xlo, xhi, xin, xout, xstr = _axis(w[:, 0], w[:, 2], W, delta, ez, rules)
    v, ylo, yhi, yin, yout, ystr = _axis(w[:, 1], w[:, 2], H, delta, ez, rules)
    one = xin & yin & (xlo == xhi) & (ylo == yhi)
    stays = xout | yout
    sure = ~applied | one | stays
    # the nominal landing pixel: floor(u), floor(v) where they pass the bound
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        lands = applied & (fu > rules.land_lo) & (fu < W - rules.land_hi) & (fv > rules.land_lo) & (fv < H - rules.land_hi)
    x = np.where(lands, fu, ex).astype(np.int64)
    y = np.where(lands, fv, ey).astype(np.int64)
    may, wild = {}, np.zeros(n, bool)
    for i in np.nonzero(~sure)[0]:
        px = {(int(ex[i]), int(ey[i]))}
        if (xstr[i] and not xout[i]) or (ystr[i] and not yout[i]) or xhi[i] - xlo[i] > 2 or yhi[i] - ylo[i] > 2:
            wild[i] = True
        else:
            for a in range(int(xlo[i]), int(xhi[i]) + 1):
                for b in range(int(ylo[i]), int(yhi[i]) + 1):
                    if rules.land_lo < a < W - rules.land_hi and rules.land_lo < b < H - rules.land_hi:
                        px.add((a, b))
        may[int(i)] = sorted(px)
    nan = np.full(n, np.nan)
    return Warp(applied, np.where(applied, u, nan), np.where(applied, v, nan), np.where(applied, w[:, 2], nan), x, y,
                sure, may, wild)


def planes64(W, H, ev, warp, threshold=FILTER_THRESHOLD):
    """the sae_latest_ and sae_ planes (L0, L1, S0, S1, as get_sae orders them) after the batch `ev` is written into
    zeroed planes at warp64's landing pixels, and the mask of pixels an unsure event may have touched.  Unsure events
    are not written: every pixel they may land on is in the mask, every other pixel sees sure events only."""
    Lp = np.zeros((2, H, W))
    Sp = np.zeros((2, H, W))
    unsure = np.zeros((H, W), bool)
    for px in warp.may.values():
        for a, b in px:
            unsure[b, a] = True
    et = event_times(ev).tolist()
    pol = (ev["polarity"] != 0).astype(np.int64).tolist()
    xs, ys, sure = warp.x.tolist(), warp.y.tolist(), warp.sure.tolist()
    for i in range(len(ev)):
        if not sure[i]:
            continue
        p, x, y, t = pol[i], xs[i], ys[i], et[i]
        t_last, t_inv = Lp[p, y, x], Lp[1 - p, y, x]
        if t > t_last + threshold or t_inv > t_last:  # createSAE_left (event_detector.cc:138-143)
            Sp[p, y, x] = t
        Lp[p, y, x] = t
    return [Lp[0], Lp[1], Sp[0], Sp[1]], unsure


def pade_band(ev, t0, motion):
    """per event: the branch of Matrix3f::exp() its skew matrix takes (3, 5 or 7) and the number of squarings, from
    the L1 norm as the float code forms it"""
    om = _f32(motion["omega"])
    fdt = (event_times(ev) - t0).astype(np.float32)
    r = np.abs(om[None, :] * fdt[:, None])
    l1 = np.maximum(np.maximum(r[:, 2] + r[:, 1], r[:, 2] + r[:, 0]), r[:, 1] + r[:, 0])
    band = np.where(l1 < PADE3_BELOW, 3, np.where(l1 < PADE5_BELOW, 5, 7))
    _, e = np.frexp((l1 / PADE7_MAXNORM).astype(np.float32))
    sq = np.where(band == 7, np.maximum(e, 0), 0)
    return band, sq, l1


# ------------------------------------------------------------------ events
def _stamps(rng, n, lo_us, hi_us, base_us):
    return base_us + np.sort(rng.choice(np.arange(lo_us, hi_us), n, replace=False))


def dense(W, H, seed, lo_us=0, hi_us=SPAN_US, base_us=BASE_US):
    """one event on every pixel, pixels shuffled against the (ascending, distinct) stamps, random polarity"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(W * H)
    return make_events(perm % W, perm // W, _stamps(rng, W * H, lo_us, hi_us, base_us), rng.integers(0, 2, W * H))


def _after_first(t_us, pol, ev):
    """`ev` without its event on pixel (0, 0), behind a first event there at t_us (the batch's t0)"""
    ev = ev[(ev["x"] != 0) | (ev["y"] != 0)]
    out = np.zeros(len(ev) + 1, EVENT_DTYPE)
    out[:1] = make_events([0], [0], [t_us], [pol])
    out[1:] = ev
    return out


def _t0(L):
    return float(event_times(L[:1])[0])


def _intrinsics(W, H):
    return dict(fx=0.9 * W, fy=0.9 * W, cx=W / 2.0 + 3.5, cy=H / 2.0 - 2.25)


def _motion(L, W, H, accel=(4.0, 5.0, 3.0), omega=(0.9, -1.4, 2.1), dt_frac=0.8, t1=None, v=(0.8, -0.3, 0.2),
            v_pre=(0.7, -0.25, 0.15), **K):
    """test_motion_compensated_sae's Motion_correction_value (tests/test_parity_gpu.py), at this size"""
    t = event_times(L)
    kw = dict(_intrinsics(W, H))
    kw.update(K)
    return dict(t1=float(t[0] + dt_frac * (t[-1] - t[0])) if t1 is None else float(t1), v=v, v_pre=v_pre, accel=accel,
                omega=omega, **kw)


# the six motions of test_motion_compensated_sae
DENSE_MOTIONS = {
    "default": dict(), "accel_low": dict(accel=(1.0, 2.0, 3.0)), "omega_9": dict(omega=(9.0, -14.0, 21.0)),
    "omega_40": dict(omega=(40.0, 35.0, -60.0)), "t1_late": dict(dt_frac=1.5), "t1_early": dict(dt_frac=-0.5),
}
LEAVES_TILE = ("pade",)  # warped events leave their source tile in every direction (the dense cases' rotations are
#                          dominated by one axis: omega_9 never goes to -x, omega_40 only to -x and +y)
PADE_OMEGA = (2.0, -3.0, 600.0)                    # the norm, 603 dt, crosses every branch up to 3 squarings in 40 ms
FRAME_OMEGA = {"frame_pos": (3.0, -3.0, 0.0), "frame_neg": (-3.0, 3.0, 0.0)}  # +x +y / -x -y, 9-28 px
DIV_F = 128.0                                      # fx = fy of the division cases: K * K^-1 is exact
DIV_US = 15_625                                    # 2^-6 s
DIV_ROWS = 8                                       # rows within this of H/2 carry the stamp t0 + 2^-6 s
MANY_VZ = -50.0                                    # w = 1 + 25 dt: 1.5 ... 2.5 for dt in 20 ... 60 ms


def _size_cases(W, H, k):
    cases = []

    def add(name, L, R, motion):
        cases.append(Case(name, W, H, (Batch(L, R, motion),)))

    L, R = dense(W, H, 100 + k), dense(W, H, 200 + k)
    for name, kw in DENSE_MOTIONS.items():
        add("dense_" + name, L, R, _motion(L, W, H, **kw))
    add("dense_v50", L, R, _motion(L, W, H, omega=(9.0, -14.0, 21.0), v=(40.0, -15.0, 10.0), v_pre=(35.0, -12.5, 7.5)))

    # all three Pade branches and 0 ... 3 squarings inside one batch: the norm grows with the event's dt
    add("pade", L, R, _motion(L, W, H, omega=PADE_OMEGA, dt_frac=1.5))

    # the acceleration gate: |a| > 5 in double, from float components
    for name, a in (("accel_5", (3.0, 4.0, 0.0)), ("accel_5_plus", (3.0, 4.0, 0.01)), ("accel_0", (0.0, 0.0, 0.0))):
        add(name, L, R, _motion(L, W, H, accel=a, omega=(9.0, -14.0, 21.0)))

    # the time gate.  t1 on an event's own stamp (ratio exactly 1: not warped), in both cameras' streams; the right
    # camera's stream starts 10 ms before the first left event (negative dt: warped)
    for name, base in (("gate", BASE_US), ("gate_epoch", EPOCH_US)):
        Lg = dense(W, H, 300 + k, base_us=base)
        Rg = dense(W, H, 400 + k, lo_us=-10_000, hi_us=SPAN_US - 10_000, base_us=base)
        late = _motion(Lg, W, H, omega=(9.0, -14.0, 21.0), dt_frac=2.0)

        def moving(ev, start):  # the first event from `start` on that the warp would move to another pixel for sure
            wp = warp64(ev, _t0(Lg), late, W, H)
            ok = wp.applied & wp.sure & ((wp.x != ev["x"]) | (wp.y != ev["y"]))
            return start + int(np.argmax(ok[start:]))
        i1 = moving(Lg, int(0.6 * len(Lg)))
        at_t1 = Rg.copy()
        at_t1["sec"], at_t1["nsec"] = Lg["sec"][i1], Lg["nsec"][i1]
        j1 = moving(at_t1, int(0.7 * len(Rg)))
        twin = (Rg["sec"] == Lg["sec"][i1]) & (Rg["nsec"] == Lg["nsec"][i1])  # stamps stay distinct: swap
        Rg["sec"][twin], Rg["nsec"][twin] = Rg["sec"][j1], Rg["nsec"][j1]
        Rg["sec"][j1], Rg["nsec"][j1] = Lg["sec"][i1], Lg["nsec"][i1]
        Rg = Rg[np.argsort(event_times(Rg), kind="stable")]
        t1 = float(event_times(Lg[i1:i1 + 1])[0])
        add(name + "_t1_on_event", Lg, Rg, _motion(Lg, W, H, omega=(9.0, -14.0, 21.0), t1=t1))
        add(name + "_t1_eq_t0", Lg, Rg, _motion(Lg, W, H, omega=(9.0, -14.0, 21.0), t1=_t0(Lg)))
        add(name + "_t1_before_t0", Lg, Rg, _motion(Lg, W, H, omega=(9.0, -14.0, 21.0), t1=_t0(Lg) - 0.01))

    # the border band and the landing bound: every pixel, stamped 20 ... 60 ms after the first left event (which sits
    # on pixel (0, 0)), moved 10 ... 19 px along the diagonal: into the image on one side, out of it on the other
    Lf, Rf = dense(W, H, 500 + k, 20_000, 60_000), dense(W, H, 600 + k, 20_000, 60_000)
    Lf = _after_first(BASE_US, 1, Lf)
    for name, om in FRAME_OMEGA.items():
        add(name, Lf, Rf, _motion(Lf, W, H, omega=om, dt_frac=1.5))

    # division by zero and overflow: omega = 0, K * K^-1 = I exactly, the rows around H/2 at dt = 2^-6 s exactly
    Ld, Rd = dense(W, H, 700 + k), dense(W, H, 800 + k)
    for ev in (Ld, Rd):
        t = (event_times(ev) * 1e6).round().astype(np.int64)
        t[np.abs(ev["y"].astype(np.int64) - H // 2) <= DIV_ROWS] = BASE_US + DIV_US
        stamped = make_events(ev["x"], ev["y"], t, ev["polarity"])
        ev["sec"], ev["nsec"] = stamped["sec"], stamped["nsec"]
    Ld = _after_first(BASE_US, 0, Ld)
    KD = dict(fx=DIV_F, fy=DIV_F, cx=float(W // 2), cy=float(H // 2))
    ex0, ey0 = W // 2 + 9, H // 2 - 3  # the pixel whose numerators are 0 too
    zero = dict(omega=(0.0, 0.0, 0.0), t1=_t0(Ld) + 0.1, v_pre=(0.0, 0.0, 0.0), **KD)
    add("div_zero", Ld, Rd, _motion(Ld, W, H, v=(DIV_F * (DIV_F * ex0 + W // 2), DIV_F * (DIV_F * ey0 + H // 2), 128.0), **zero))
    add("div_zero_split", Ld, Rd, _motion(Ld, W, H, **dict(zero, v=(0.0, 0.0, 100.0), v_pre=(0.0, 0.0, 28.0))))
    add("div_negative", Ld, Rd, _motion(Ld, W, H, v=(0.0, 0.0, 130.0), **zero))
    add("div_huge", Ld, Rd, _motion(Ld, W, H, v=(0.0, 0.0, 128.0 - 2.0 ** -10), **zero))

    # many-to-one: the image scales by 1/1.5 ... 1/2.5, about four sources per target; two batches in a row
    batches = []
    for b in range(2):
        base = BASE_US + b * 65_000
        Lm, Rm = (dense(W, H, 900 + 10 * b + k + s, 20_000, 60_000, base_us=base) for s in (0, 50))
        Lm = _after_first(base, 1, Lm)
        batches.append(Batch(Lm, Rm, _motion(Lm, W, H, omega=(0.3, -0.2, 0.5), v=(0.0, 0.0, MANY_VZ),
                                             v_pre=(0.0, 0.0, 0.0), dt_frac=1.5)))
    cases.append(Case("many_to_one", W, H, tuple(batches)))
    return cases


@functools.lru_cache(maxsize=None)
def build():
    """{(W, H): [Case, ...]}; the event arrays are shared and read-only"""
    out = {}
    for k, (W, H) in enumerate(SIZES):
        out[(W, H)] = _size_cases(W, H, k)
        for c in out[(W, H)]:
            for b in c.batches:
                b.L.setflags(write=False)
                b.R.setflags(write=False)
    return out


def case_names():
    return [c.name for c in build()[SIZES[0]]]


def float64_case_names():
    return [n for n in case_names() if n not in ORACLE_ONLY]


def get(W, H, name):
    return next(c for c in build()[(W, H)] if c.name == name)


# ------------------------------------------------------------------ the oracle on a case
def oracle_planes(O, case, upto=None):
    """the oracle's planes [cam][L0, L1, S0, S1] after the case's batches (the first `upto` of them)"""
    det = O.Detector(case.W, case.H)
    for b in case.batches[:upto]:
        m = O.make_motion(**b.motion)
        det.create_sae_mc(0, b.L, b.L[:1], m)
        det.create_sae_mc(1, b.R, b.L[:1], m)
    return [det.get_sae(0), det.get_sae(1)]


def landing_from_planes(ev, planes):
    """where each event of a batch written into zeroed planes landed, read back from the sae_latest_ planes by its
    stamp: (x, y), -1 for an event whose stamp is not unique in the batch or was overwritten on its pixel"""
    et = event_times(ev)
    x = np.full(len(ev), -1, np.int64)
    y = np.full(len(ev), -1, np.int64)
    uniq, idx, cnt = np.unique(et, return_index=True, return_counts=True)
    for pol in (0, 1):
        ys, xs = np.nonzero(planes[pol])
        st = planes[pol][ys, xs]
        k = np.searchsorted(uniq, st)
        ok = (k < len(uniq)) & (uniq[np.minimum(k, len(uniq) - 1)] == st)
        ok &= cnt[np.minimum(k, len(uniq) - 1)] == 1
        i = idx[k[ok]]
        keep = (ev["polarity"][i] != 0) == bool(pol)
        x[i[keep]], y[i[keep]] = xs[ok][keep], ys[ok][keep]
    return x, y


@functools.lru_cache(maxsize=None)
def expected64(W, H, name):
    """per camera (planes, unsure mask, unsure events, warped events) of a case's first batch by warp64 + planes64"""
    b = get(W, H, name).batches[0]
    out = []
    for ev in (b.L, b.R):
        wp = warp64(ev, _t0(b.L), b.motion, W, H)
        planes, unsure = planes64(W, H, ev, wp)
        out.append((planes, unsure, int((~wp.sure).sum()), int(wp.applied.sum())))
    return out


def mismatch64(case, planes, rules=EXACT):
    """the pixels outside the unsure set at which the planes [cam][L0, L1, S0, S1] of the case's first batch are not
    the float64 planes: [(cam, plane name, x, y, got, float64), ...]"""
    b = case.batches[0]
    bad = []
    for cam, ev in ((0, b.L), (1, b.R)):
        if rules == EXACT:
            want, unsure = expected64(case.W, case.H, case.name)[cam][:2]
        else:
            want, unsure = planes64(case.W, case.H, ev, warp64(ev, _t0(b.L), b.motion, case.W, case.H, rules))
        for k, name in enumerate(("L0", "L1", "S0", "S1")):
            ys, xs = np.nonzero((np.asarray(planes[cam][k]) != want[k]) & ~unsure)
            bad += [(cam, name, int(x), int(y), float(planes[cam][k][y, x]), float(want[k][y, x])) for x, y in zip(xs, ys)]
    return bad


def events_landing_on(case, cam, x, y):
    """the events of the case's first batch that warp64 writes to (or may write to) pixel (x, y) of camera cam: what a
    failure report shows next to the pixel"""
    b = case.batches[0]
    ev = (b.L, b.R)[cam]
    wp = warp64(ev, _t0(b.L), b.motion, case.W, case.H)
    hit = (wp.x == x) & (wp.y == y)
    for i, px in wp.may.items():
        hit[i] |= (x, y) in px
    return [dict(i=int(i), src=(int(ev["x"][i]), int(ev["y"][i])), t=float(event_times(ev[i:i + 1])[0]),
                 pol=int(ev["polarity"][i]), u=float(wp.u[i]), v=float(wp.v[i]), sure=bool(wp.sure[i]))
            for i in np.nonzero(hit)[0]]


def tile_exits(case):
    """the directions in which sure, warped events of the case leave their source tile of the tiled update"""
    b = case.batches[0]
    out = set()
    for ev in (b.L, b.R):
        wp = warp64(ev, _t0(b.L), b.motion, case.W, case.H)
        for src, dst, T, names in ((ev["x"], wp.x, TILE[0], ("-x", "+x")), (ev["y"], wp.y, TILE[1], ("-y", "+y"))):
            d = dst[wp.sure] // T - src[wp.sure].astype(np.int64) // T
            out |= {names[0]} if (d < 0).any() else set()
            out |= {names[1]} if (d > 0).any() else set()
    return out


def measure(O, verbose=False, sizes=SIZES):
    """the largest scaled distance to an integer of an event that the oracle and warp64 write to different pixels, over
    every case compared with float64; (measured, events that differ, events compared)"""
    worst, ndiff, ntot = 0.0, 0, 0
    for W, H in sizes:
        for c in build()[(W, H)]:
            if c.name in ORACLE_ONLY:
                continue
            b = c.batches[0]
            planes = oracle_planes(O, c)
            cw, cd = 0.0, 0
            for cam, ev in ((0, b.L), (1, b.R)):
                wp = warp64(ev, _t0(b.L), b.motion, W, H)
                ox, oy = landing_from_planes(ev, planes[cam])
                known = ox >= 0
                dx, dy = known & (ox != wp.x), known & (oy != wp.y)
                ntot += int(known.sum())
                with np.errstate(all="ignore"):
                    sc = (1.0 + np.maximum(np.abs(wp.u) / W, np.abs(wp.v) / H)) / np.abs(wp.w2)
                    du = np.abs(wp.u - np.round(wp.u)) / sc
                    dv = np.abs(wp.v - np.round(wp.v)) / sc
                for i in np.nonzero(dx | dy)[0]:
                    moved_o = (ox[i], oy[i]) != (ev["x"][i], ev["y"][i])
                    moved_f = (wp.x[i], wp.y[i]) != (ev["x"][i], ev["y"][i])
                    if moved_o != moved_f:     # one side refused the landing: the coordinate nearest a bound's integer
                        d = np.nanmin([du[i], dv[i]])
                    else:
                        d = np.nanmax([du[i] if dx[i] else 0.0, dv[i] if dy[i] else 0.0])
                    cw, cd = max(cw, float(d) if np.isfinite(d) else np.inf), cd + 1  # (inf: a gate disagrees)
            if verbose:
                print("%3dx%-3d %-22s differ %3d  farthest %.3e" % (W, H, c.name, cd, cw))
            worst, ndiff = max(worst, cw), ndiff + cd
    return worst, ndiff, ntot


def unsure_share(case):
    """unsure events / warped events of a case's first batch, both cameras"""
    b = case.batches[0]
    applied = unsure = 0
    for ev in (b.L, b.R):
        wp = warp64(ev, _t0(b.L), b.motion, case.W, case.H)
        applied += int(wp.applied.sum())
        unsure += int((~wp.sure).sum())
    return unsure / max(applied, 1), unsure, applied


if __name__ == "__main__":
    from oracle import oracle as O
    O.lib()
    worst, ndiff, ntot = measure(O, verbose=True)
    d = 2.0 ** int(np.ceil(np.log2(4 * worst))) if worst > 0 else 0.0
    print("MEASURED_DISAGREEMENT = %.3e px (%d of %d events differ); DELTA = 4 x, rounded up = 2^%d = %.3e"
          % (worst, ndiff, ntot, int(np.log2(d)) if d else 0, d))
    for (W, H), cases in build().items():
        for c in cases:
            s, u, a = unsure_share(c)
            print("%3dx%-3d %-22s unsure %5d of %6d warped = %.3f %%" % (W, H, c.name, u, a, 100 * s))
