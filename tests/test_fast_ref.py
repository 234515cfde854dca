"""CPU: the FAST stage is pinned to outputs of the reference's own compiled code.

tests/golden/fast_ref_*.npz hold, per image and barrier, what fast::fast_corner_detect_9 / _10,
fast::fast_corner_score_10 and fast::fast_nonmax_3x3 of the reference's vendored library
(dependences/fast_neon-master, plain C++) returned (tests/golden/make_fast_ref.py).  The numpy
restatement tests/fast_ref.py must reproduce them element for element and in order; the GPU tests then
use the restatement on inputs the fixtures do not hold.  Also: the new C ABI symbol is declared and
exported, and refuses bad arguments (no device needed: the checks come before any GPU call)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import fast_ref
from esvio_amd import frontend as FE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "fast_ref_*.npz")))


def fixture_cases(path):
    """(name, img, barrier, d9, d10, s10, nm) of one fixture file"""
    z = np.load(path)
    for name in z["names"]:
        name = str(name)
        img = z[name + "_img"]
        for b in z[name + "_barriers"]:
            k = "%s_b%d_" % (name, int(b))
            yield name, img, int(b), z[k + "d9"], z[k + "d10"], z[k + "s10"], z[k + "nm"]


def test_fixture_set_is_complete():
    names = {os.path.basename(f) for f in FILES}
    assert names == {"fast_ref_ts_346x260.npz", "fast_ref_noise_346x260.npz", "fast_ref_ts_640x480.npz",
                     "fast_ref_eq_640x480.npz", "fast_ref_ts_1280x720.npz", "fast_ref_small.npz"}
    for f in FILES:
        assert os.path.getsize(f) < 712434, f
        assert "g++" in str(np.load(f)["compiler"]) or "gcc" in str(np.load(f)["compiler"]).lower()


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[9:-4] for f in FILES])
def test_restatement_equals_reference_outputs(path):
    n = 0
    maps = {}
    for name, img, b, d9, d10, s10, nm in fixture_cases(path):
        if name not in maps:
            maps[name] = (fast_ref.score_map(img, 9), fast_ref.score_map(img, 10))
        m9, m10 = maps[name]
        xy9, _ = fast_ref.detect(img, 9, b, m9)
        xy10, sc10 = fast_ref.detect(img, 10, b, m10)
        idx = fast_ref.nonmax_3x3(xy10, sc10, img.shape)
        print(name, img.shape, "barrier", b, "n9", len(d9), "n10", len(d10), "nonmax", len(nm))
        assert d9.dtype == np.int16 and s10.dtype == np.int32 and nm.dtype == np.int32
        assert np.array_equal(xy9, d9), (name, b, "detect_9")
        assert np.array_equal(xy10, d10), (name, b, "detect_10")
        assert np.array_equal(sc10, s10), (name, b, "score_10")
        assert np.array_equal(idx, nm), (name, b, "nonmax_3x3")
        # the composed call of the C ABI
        xy, sc, nd = fast_ref.fast_corners(img, 10, b, True)
        assert np.array_equal(xy, d10[nm]) and np.array_equal(sc, s10[nm]) and nd == len(d10)
        n += 1
    assert n >= 2


def test_fixtures_hit_the_edges_of_the_definition():
    z = np.load(os.path.join(GOLDEN, "fast_ref_small.npz"))
    H, W = z["edges_img"].shape
    assert z["edges_b20_d10"].tolist() == [[3, 3], [W - 4, H - 4]]          # first and last pixel visited
    assert len(z["constant_b0_d9"]) == 0                                    # barrier 0 is strict: p > c
    assert len(z["tiny6x9_b0_d9"]) == 0 and z["tiny7x7c_b20_d10"].tolist() == [[3, 3]]
    # equal neighbours suppress each other, unequal ones leave the larger
    d, s, nm = z["plateaus_b20_d10"], z["plateaus_b20_s10"], z["plateaus_b20_nm"]
    kept = {tuple(p) for p in d[nm].tolist()}
    assert (41, 36) in kept and (40, 36) not in kept
    assert not any((x, 10) in kept for x in range(10, 13))
    assert len(nm) < len(d)


def test_abi_symbol_and_argument_checks():
    assert "esvio_fe_fast_corners" in FE.ABI_SYMBOLS
    L = FE.load_library()
    f = L.esvio_fe_fast_corners
    assert f.argtypes is not None and len(f.argtypes) == 12
    n = C.c_int32(-7)
    # a NULL handle is refused before anything touches a device
    assert f(None, 0, None, 0, 10, 20, 1, None, None, 0, C.byref(n), None) == -1  # ESVIO_FE_EINVAL
