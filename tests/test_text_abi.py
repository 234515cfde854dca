"""CPU: the text stage's entry points that need no device, through the library and its Python mirror — the side files
(esvio_fe_text_imu, esvio_fe_text_images: argument checks, return codes, n_out, the mirror's default capacities), the limits
and the kernel table, and the argument checks of the handle's calls on a null handle."""
import ctypes as C

import numpy as np
import pytest

import text_ref as T
from esvio_amd import frontend as FE

IMU = b"# imu\n1.5 0.1 -9.81 1e-05 0 3.25 -0.5\r\n\n2.000000001,1,2,3,4,5,6\n3 inf -inf 0.30000000000000004 1E3 -0.0 7"
IMAGES = b"0.100000000 images/frame_00000000.png\n1.5\timages/frame 1,a.png \r\n% c\n2 x"


def test_text_imu_reads_the_davis_extractors_lines():
    imu = FE.text_imu(IMU)
    assert imu.dtype == FE.IMU_DTYPE and len(imu) == 3
    assert [(int(s), int(n)) for s, n in zip(imu["sec"], imu["nsec"])] == [(1, 500000000), (2, 1), (3, 0)]
    assert imu["acc"][0].tolist() == [0.1, -9.81, 1e-05] and imu["gyr"][0].tolist() == [0.0, 3.25, -0.5]
    assert imu["acc"][1].tolist() == [1.0, 2.0, 3.0] and imu["gyr"][1].tolist() == [4.0, 5.0, 6.0]
    assert imu["acc"][2][0] == np.inf and imu["acc"][2][1] == -np.inf and imu["acc"][2][2] == float("0.30000000000000004")
    assert imu["gyr"][2][0] == 1000.0 and np.signbit(imu["gyr"][2][1]) and imu["gyr"][2][1] == 0.0
    # the offset moves every stamp, in exact integers
    assert [int(s) for s in FE.text_imu(IMU, t_offset_ns=10 ** 9 - 1)["sec"]] == [2, 3, 3]
    assert len(FE.text_imu(b"")) == 0 and len(FE.text_imu(b"# nothing\n\n")) == 0
    # the mirror's default capacity, a sample per 14 bytes, holds the shortest lines there are
    short = b"0 0 0 0 0 0 0\n" * 50
    assert len(FE.text_imu(short)) == 50 and len(FE.text_imu(short[:-1])) == 50


def test_text_imu_refusals_say_where_or_how_many():
    with pytest.raises(FE.FrontendError) as e:
        FE.text_imu(IMU, cap=2)
    assert e.value.n == 3                                     # too small a capacity: the number needed
    with pytest.raises(FE.FrontendError) as e:
        FE.text_imu(IMU, t_offset_ns=-1_600_000_000)          # BAD: the first stamp is 1.5 s
    assert e.value.n == 0
    for bad in (b"2 1 2 3 4 5\n", b"2 1 2 3 4 5 6 7\n", b"2 1 2 3 4 5 +6\n", b"2 1 2 3 4 5 6x\n", b"2. 1 2 3 4 5 6\n", b"2 1 2 3 4 5 0x10\n"):
        with pytest.raises(FE.FrontendError) as e:
            FE.text_imu(b"1 0 0 0 0 0 0\n" + bad + b"3 0 0 0 0 0 0\n")
        assert e.value.n == 1, bad                            # the samples in front of the line that does not read
    L = FE.load_library()
    out, n = np.zeros(4, FE.IMU_DTYPE), C.c_size_t(7)
    assert L.esvio_fe_text_imu(IMU, len(IMU), 0, FE._p(out), 4, None) == -1           # no n_out
    assert L.esvio_fe_text_imu(None, len(IMU), 0, FE._p(out), 4, C.byref(n)) == -1    # bytes null with n > 0
    assert L.esvio_fe_text_imu(IMU, len(IMU), 0, None, 4, C.byref(n)) == -1           # out null with room
    assert L.esvio_fe_text_imu(IMU, len(IMU), (1 << 62) + 1, FE._p(out), 4, C.byref(n)) == -1
    assert L.esvio_fe_text_imu(IMU, len(IMU), -(1 << 62) - 1, FE._p(out), 4, C.byref(n)) == -1
    assert n.value == 7                                       # an argument error touches nothing
    assert L.esvio_fe_text_imu(IMU, len(IMU), 0, None, 0, C.byref(n)) == -1 and n.value == 3   # counting alone
    assert L.esvio_fe_text_imu(None, 0, 0, None, 0, C.byref(n)) == 0 and n.value == 0


def test_text_images_reads_stamps_and_paths():
    stamps, paths = FE.text_images(IMAGES)
    assert stamps.tolist() == [100000000, 1500000000, 2000000000]
    assert paths == [b"images/frame_00000000.png", b"images/frame 1,a.png", b"x"]
    assert FE.text_images(IMAGES, t_offset_ns=5)[0].tolist() == [100000005, 1500000005, 2000000005]
    # the stamp is the event files' SEC_DECIMAL token
    for tok in (b"7", b"7.5", b"4294967295.999999999", b"0.1234567891"):
        cls, rec = T.classify(tok + b" 0 0 0", T.TXYP, T.SEC_DECIMAL)
        assert FE.text_images(tok + b" p\n")[0].tolist() == [rec[5]]
    short = b"0 a\n" * 30  # the mirror's default capacity: an entry per 4 bytes
    assert len(FE.text_images(short)[1]) == 30
    with pytest.raises(FE.FrontendError) as e:
        FE.text_images(IMAGES, cap=1)
    assert e.value.n == 3
    for bad in (b"1.5\n", b"1.5 \n", b".5 p\n", b"1e5 p\n", b"4294967296 p\n"):
        with pytest.raises(FE.FrontendError) as e:
            FE.text_images(b"1 a\n" + bad)
        assert e.value.n == 1, bad
    L = FE.load_library()
    st, off, ln, n = np.zeros(4, np.int64), np.zeros(4, np.uint64), np.zeros(4, np.uint32), C.c_size_t(9)
    args = (FE._p(st), FE._p(off), FE._p(ln))
    assert L.esvio_fe_text_images(IMAGES, len(IMAGES), 0, *args, 4, None) == -1
    assert L.esvio_fe_text_images(None, 5, 0, *args, 4, C.byref(n)) == -1
    for k in range(3):
        a = list(args)
        a[k] = None
        assert L.esvio_fe_text_images(IMAGES, len(IMAGES), 0, *a, 4, C.byref(n)) == -1
    assert L.esvio_fe_text_images(IMAGES, len(IMAGES), (1 << 62) + 1, *args, 4, C.byref(n)) == -1 and n.value == 9
    assert L.esvio_fe_text_images(IMAGES, len(IMAGES), 0, *args, 4, C.byref(n)) == 0 and n.value == 3
    assert [IMAGES[int(o):int(o) + int(m)] for o, m in zip(off[:3], ln[:3])] == paths


def test_text_limits_the_kernel_table_and_null_handles():
    lim = FE.text_limits()
    assert (lim.max_body, lim.max_tail) == (64, 65) and lim.tile_bytes >= 1024 and lim.tile_bytes % 256 == 0
    assert FE.text_bound(0) == 9 and FE.text_bound(8) == 10
    L = FE.load_library()
    assert L.esvio_fe_text_limits(None) == -1
    assert [L.esvio_fe_text_kernel_name(k) for k in range(L.esvio_fe_text_kernel_count())] == [b"k_text_count", b"k_text_place", b"k_text_emit"]
    assert L.esvio_fe_text_kernel_name(-1) == b"" and L.esvio_fe_text_kernel_name(3) == b""
    assert L.esvio_fe_text_kernel_stats(None, 0, None, None, None) == -1
    fmt = FE.TextFormat(FE.TEXT_TXYP, FE.TEXT_SEC_DECIMAL, 0, 0)
    assert L.esvio_fe_decode_text(None, 0, C.byref(fmt), None, 0, FE.HOST, 0, None, 0, FE.HOST, None) == -1
    assert L.esvio_fe_track_text(None, C.byref(fmt), None, 0, None, 0, FE.HOST, 0, 1, None, None, None, None, None) == -1
    assert L.esvio_fe_feed_push_text(None, 0, C.byref(fmt), None, 0, FE.HOST, 0, None) == -1
