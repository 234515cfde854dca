"""CPU: tests/aedat_ref.py — the sequential reading of the AEDAT 3.1 rule — against answers derived by hand from byte
strings written out here, and the every-cut property of the loops themselves."""
import struct

import numpy as np
import pytest

import aedat_ref as A


def hdr(etype, size, overflow, capacity, number, ts_offset=4):
    return struct.pack("<hhiiiiii", etype, 1, size, ts_offset, overflow, capacity, number, 0)


def test_one_polarity_packet_written_out_byte_by_byte():
    # x = 3, y = 2, p = 1, valid: data = 1 | 1<<1 | 2<<2 | 3<<17 = 0x0006000B; ts = 5 us
    data = hdr(1, 8, 0, 1, 1) + bytes([0x0B, 0x00, 0x06, 0x00, 0x05, 0x00, 0x00, 0x00])
    assert A.polarity(3, 2, 1, 5) == data[28:]
    o = A.decode(data)
    assert o["events"] == [(3, 2, 0, 5000, 1)] and o["invalid"] == 0 and o["polarity_packets"] == 1
    # the same event with valid = 0 is dropped, or kept with the flag: what the reference's drivers do
    data = hdr(1, 8, 0, 1, 1) + bytes([0x0A, 0x00, 0x06, 0x00, 0x05, 0x00, 0x00, 0x00])
    assert A.decode(data)["events"] == [] and A.decode(data)["invalid"] == 1
    o = A.decode(data, flags=A.KEEP_INVALID)
    assert o["events"] == [(3, 2, 0, 5000, 1)] and o["invalid"] == 0


def test_overflow_one_with_the_largest_ts():
    # ts64 = 1 << 31 | 0x7FFFFFFF = 2^32 - 1 us = 4294.967295 s
    data = hdr(1, 8, 1, 1, 1) + struct.pack("<Ii", 1, 0x7FFFFFFF)
    assert A.decode(data)["events"] == [(0, 0, 4294, 967295000, 0)]
    assert A.decode(data)["ticks"] == [4294967295000]


def test_the_nsec_carry_of_a_nanosecond_offset():
    # 1 us + 1 999 999 999 ns = 2 000 000 999 ns = 2 s + 999 ns
    data = hdr(1, 8, 0, 1, 1) + struct.pack("<Ii", 1, 1)
    assert A.decode(data, t_offset_ns=1_999_999_999)["events"] == [(0, 0, 2, 999, 0)]
    # a negative offset that the stamp outweighs; one that it does not is BAD
    assert A.decode(data, t_offset_ns=-999)["events"] == [(0, 0, 0, 1, 0)]
    with pytest.raises(A.Bad) as e:
        A.decode(data, t_offset_ns=-1001)
    assert e.value.bad == 1


def test_fifteen_bit_addresses():
    data = hdr(1, 8, 0, 2, 2) + struct.pack("<IiIi", 0xFFFFFFFF, 0, 0x7FFF << 17 | 1, 0)
    assert A.decode(data)["events"] == [(0x7FFF, 0x7FFF, 0, 0, 1), (0x7FFF, 0, 0, 0, 0)]


def test_an_imu6_samples_six_doubles():
    # values exact in binary: ax = 0.5 g -> -0.5 * 9.81; gx = 90 deg/s -> -90 / 180 * pi
    rec = struct.pack("<Ii7f", 1, 2_000_000, 0.5, -0.25, 1.0, 90.0, -45.0, 180.0, 30.0)
    o = A.decode(hdr(3, 36, 0, 1, 1) + rec, mode="side")
    (sec, nsec, acc, gyr), = o["imu"]
    assert (sec, nsec) == (2, 0)
    assert acc == (-0.5 * 9.81, -0.25 * 9.81, -1.0 * 9.81)
    assert gyr == (-90.0 / 180.0 * np.pi, -45.0 / 180.0 * np.pi, -180.0 / 180.0 * np.pi)
    # a value that is not exact in float: the float is widened AFTER the negation, no rounding to double before it
    rec = struct.pack("<Ii7f", 1, 0, 0.1, 0, 0, 0.1, 0, 0, 0)
    (_, _, acc, gyr), = A.decode(hdr(3, 36, 0, 1, 1) + rec, mode="side")["imu"]
    f = float(np.float32(0.1))  # 0.100000001490116...
    assert acc[0] == -f * 9.81 and acc[0] != -0.1 * 9.81 and gyr[0] == -f / 180.0 * np.pi
    # the event walker skips the packet whole, the side walker skips polarity packets
    assert A.decode(hdr(3, 36, 0, 1, 1) + rec)["events"] == [] and A.decode(hdr(3, 36, 0, 1, 1) + rec)["imu_packets"] == 1


def test_a_reset_and_the_three_external_input_types():
    ev = b"".join(struct.pack("<Ii", 1 | t << 1, 10 * t) for t in (1, 2, 3, 4, 5, 0))
    o = A.decode(hdr(0, 8, 0, 6, 6) + ev, mode="side")
    assert o["resets"] == 1 and o["other_specials"] == 2
    assert o["triggers"] == [(0, 20000, 2, 1), (0, 30000, 3, 0), (0, 40000, 4, 1)]


def test_capacity_greater_than_number_is_padding():
    pad = b"\xff" * 16  # (would be two valid events with ts < 0)
    data = hdr(1, 8, 0, 3, 1) + A.polarity(1, 1, 1, 7) + pad + hdr(1, 8, 0, 1, 1) + A.polarity(2, 2, 0, 8)
    o = A.decode(data)
    assert o["events"] == [(1, 1, 0, 7000, 1), (2, 2, 0, 8000, 0)] and o["polarity_packets"] == 2


def test_malformed_headers_and_bad_stamps():
    ok = A.polarity(1, 1, 1, 7)
    for h in (hdr(1, 0, 0, 1, 1), hdr(7, -8, 0, 1, 1), hdr(1, 8, 0, -1, 0), hdr(1, 8, 0, 1, -1), hdr(1, 8, 0, 1, 2),
              hdr(1, 12, 0, 1, 1), hdr(0, 8, 0, 1, 1, ts_offset=0), hdr(3, 8, 0, 1, 1), hdr(3, 36, 0, 1, 1, ts_offset=8)):
        with pytest.raises(A.Malformed):
            A.decode(h + ok)
    A.decode(hdr(9, 12, 0, 2, 1, ts_offset=0) + b"\0" * 24)  # an unknown type may have any size and offset
    for rec, ovf, off in ((A.polarity(0, 0, 0, -1), 0, 0), (ok, -1, 0), (ok, 0, -8000), (ok, 1 << 22, 0), (ok, 0, 2 ** 32 * 10 ** 9 - 7000)):
        with pytest.raises(A.Bad):
            A.decode(hdr(1, 8, ovf, 1, 1) + rec, t_offset_ns=off)
    assert A.decode(hdr(1, 8, 0, 1, 1) + ok, t_offset_ns=2 ** 32 * 10 ** 9 - 7001)["events"] == [(1, 1, 2 ** 32 - 1, 999999999, 1)]
    # a dropped event is never BAD
    assert A.decode(hdr(1, 8, 0, 1, 1) + A.polarity(0, 0, 0, -1, valid=0))["invalid"] == 1


def test_every_cut_of_the_loops_themselves():
    s = A.small_stream()
    for mode in ("events", "side"):
        whole = A.decode(s, 1_000_000_007, mode=mode)
        for cut in range(len(s) + 1):
            w, a = A.Walker(mode).feed(s[:cut], 1_000_000_007)
            w, b = w.feed(s[cut:], 1_000_000_007)
            for k in whole:
                assert a[k] + b[k] == whole[k], (mode, cut, k)
            assert w.payload_left == 0 and w.hdr == b"" and w.rec == b""
    ev, info = A.decode_fast(s, 1_000_000_007)
    whole = A.decode(s, 1_000_000_007)
    assert ev.tobytes() == A.events_array(whole["events"]).tobytes()
    assert (info["events"], info["invalid"], info["polarity_packets"], info["other_packets"]) == (11, 1, 3, 1)
    ev, info = A.decode_fast(s, 0, A.KEEP_INVALID)
    assert ev.tobytes() == A.events_array(A.decode(s, 0, A.KEEP_INVALID)["events"]).tobytes() and info["events"] == 12


def test_the_readings_constants_are_the_front_ends_mirrors():
    from esvio_amd import frontend as FE
    assert A.KEEP_INVALID == FE.AEDAT_KEEP_INVALID
    assert A.IMU_DTYPE == FE.IMU_DTYPE and A.TRIGGER_DTYPE == FE.TRIGGER_DTYPE
    h = b"#!AER-DAT3.1\r\n#!END-HEADER\r\n"
    i = FE.aedat_header(h + A.small_stream())
    assert (i.payload_offset, i.version, i.complete) == (len(h), 31, 1)


def test_decoded_imu_samples_reach_the_nodes_imu_callback():
    from esvio_amd.node import MotionCorrection
    rec = [A.imu6(1000 * k, (0.5, 0.0, 1.0), (90.0, 0.0, -45.0)) for k in (1, 2, 2, 3)]  # (the third is "in disorder": not newer)
    imu = A.imu_array(A.decode(A.packet(A.IMU6, rec), 2_000_000_000, mode="side")["imu"])
    mc = MotionCorrection(200.0, 200.0, 173.0, 130.0)
    mc.imu_samples(imu)
    assert [s[0] for s in mc.imu_buf] == [2.001, 2.002, 2.003]
    assert mc.imu_buf[0][1] == (-90.0 / 180.0 * np.pi, 0.0, 45.0 / 180.0 * np.pi) and mc.imu_buf[0][2] == (-0.5 * 9.81, 0.0, -9.81)
