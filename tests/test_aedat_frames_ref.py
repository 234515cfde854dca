"""CPU: the sequential reading of the "AEDAT 3.1 frames" rule (tests/aedat_frame_ref.py) against answers derived by hand
from the text of include/esvio_fe.h."""
import numpy as np
import pytest

import aedat_frame_ref as F
import aedat_ref as A


def one(pixels, lx, ly, ch, **kw):
    return F.decode(F.frame_packet([F.frame_event(pixels, lx, ly, ch, **kw)]))


def test_the_high_byte_is_the_gray_of_a_mono_frame():
    o = one([0xFFFF, 0x00FF, 0x0100], 3, 1, 1)
    assert o["images"][0].tolist() == [[255, 0, 1]]
    assert F.convert([0xFFFF, 0x00FF, 0x0100], 1, 3, 1).tolist() == [[255, 0, 1]]


def test_a_colour_frame_goes_through_the_15_bit_gray_on_the_high_bytes():
    # (R, G, B) = (0, 0, 250): (250 * 3735 + 16384) >> 15 = 950134 >> 15 = 28 (OpenCV 3's 14-bit constants give 29)
    assert (250 * 3735 + 16384) >> 15 == 28
    o = one([0x00FF, 0x00FF, (250 << 8) | 0xFF, 0xFFFF, 0xFFFF, 0xFFFF], 2, 1, 3)
    assert o["images"][0].tolist() == [[28, 255]]  # (255 * 32768 + 16384) >> 15 = 255
    assert F.gray(255, 0, 0) == (255 * 9798 + 16384) >> 15 == 76 and F.gray(0, 255, 0) == 150 and F.gray(0, 0, 255) == 29
    v = F.test_pixels(7, 5, 3, 3)
    assert np.array_equal(F.convert(v, 5, 7, 3), F.convert_fast(v, 5, 7, 3))
    v = F.test_pixels(7, 5, 1, 4)
    assert np.array_equal(F.convert(v, 5, 7, 1), F.convert_fast(v, 5, 7, 1))


def test_the_stamp_is_the_mid_exposure_stamp_truncated_toward_zero():
    # an odd exposure length: 20 + 11 / 2 = 25 us
    r = one([1], 1, 1, 1, ts=(1, 2, 20, 31))["rows"][0]
    assert (r["stamp_sec"], r["stamp_nsec"], r["exposure_us"]) == (0, 25000, 11)
    # ts_endexposure < ts_startexposure: 31 + (-11) / 2 = 31 - 5 = 26, not 25 (which rounding down would give)
    r = one([1], 1, 1, 1, ts=(1, 2, 31, 20))["rows"][0]
    assert (r["stamp_sec"], r["stamp_nsec"], r["exposure_us"]) == (0, 26000, -11)
    assert F.mid_exposure(-9, 2) == -4 and F.mid_exposure(2, -9) == -3 and F.mid_exposure(-2 ** 31, 2 ** 31 - 1) == -1
    # the four raw stamps are recorded as they are
    assert [r[k] for k in ("ts_startframe", "ts_endframe", "ts_startexposure", "ts_endexposure")] == [1, 2, 31, 20]


def test_an_overflow_of_1_adds_2_to_the_31_microseconds_and_the_offset_is_nanoseconds():
    s = F.frame_packet([F.frame_event([1], 1, 1, 1, ts=(0, 0, 4, 6))], overflow=1)
    r = F.decode(s)["rows"][0]
    assert (r["stamp_sec"], r["stamp_nsec"], r["ts_overflow"]) == ((2 ** 31 + 5) // 10 ** 6, ((2 ** 31 + 5) % 10 ** 6) * 1000, 1)
    assert (r["stamp_sec"], r["stamp_nsec"]) == (2147, 483653000)
    r = F.decode(s, t_offset_ns=10 ** 9 + 7)["rows"][0]
    assert (r["stamp_sec"], r["stamp_nsec"]) == (2148, 483653007)
    with pytest.raises(F.Bad) as e:  # a negative sum
        F.decode(s, t_offset_ns=-(2 ** 31 + 5) * 1000 - 1)
    assert e.value.bad == 1
    with pytest.raises(F.Bad):  # sec >= 2^32
        F.decode(s, t_offset_ns=2 ** 32 * 10 ** 9 - (2 ** 31 + 5) * 1000)
    assert F.decode(s, t_offset_ns=2 ** 32 * 10 ** 9 - (2 ** 31 + 5) * 1000 - 1)["rows"][0]["stamp_sec"] == 2 ** 32 - 1


def test_slot_and_validity_in_both_modes():
    ev = [F.frame_event([k << 8], 1, 1, 1, ts=(0, 0, 10 * k, 10 * k), valid=k != 1) for k in range(3)]
    s = F.frame_packet(ev, capacity=5) + F.frame_packet([F.frame_event([9 << 8], 1, 1, 1, valid=0)])
    o = F.decode(s)
    assert [(r["slot"], r["valid"], r["index"]) for r in o["rows"]] == [(0, 1, 0), (2, 1, 1)] and o["invalid"] == 2
    assert [int(g[0, 0]) for g in o["images"]] == [0, 2] and o["frame_packets"] == 2
    o = F.decode(s, flags=F.KEEP_INVALID)
    assert [(r["slot"], r["valid"], r["index"]) for r in o["rows"]] == [(0, 1, 0), (1, 0, 1), (2, 1, 2), (0, 0, 3)] and o["invalid"] == 0
    # the rows with slot == 0 under KEEP_INVALID are the driver's frames: event 0 of every packet, whatever its valid bit
    assert [int(g[0, 0]) for g, r in zip(o["images"], o["rows"]) if r["slot"] == 0] == [0, 9]
    # a dropped event is not examined further: never BAD, malformed or refused
    junk = F.frame_event([1, 2], -5, 0, 6, ts=(0, 0, -100, -100), valid=0)
    assert F.decode(F.frame_packet([junk]))["invalid"] == 1
    with pytest.raises(F.Malformed):
        F.decode(F.frame_packet([junk]), flags=F.KEEP_INVALID)


def test_the_info_word_and_the_position_are_recorded():
    r = one([1, 2, 3], 1, 1, 3, position=(-7, 9), color_filter=11, roi=100)["rows"][0]
    assert (r["channels"], r["color_filter"], r["roi"], r["position_x"], r["position_y"], r["length_x"], r["length_y"]) == (3, 11, 100, -7, 9, 1, 1)


def test_bytes_behind_the_pixels_are_never_read_and_other_types_are_passed_over():
    ev = F.frame_event([0x0500, 0x0600], 2, 1, 1, size=36 + 4 + 10)
    s = F.frame_packet([ev]) + A.packet(9, [bytes(20)], size=20)
    o = F.decode(A.packet(A.POLARITY, [A.polarity(1, 2, 1, 3)]) + s)
    assert o["images"][0].tolist() == [[5, 6]] and o["pixels"][0] == bytes([0, 5, 0, 6])
    assert (o["frame_packets"], o["other_packets"]) == (1, 1)
    # A.small_stream's type-2 packet has eventSize 12: to the frame walker a malformed header, to the other two another type
    with pytest.raises(F.Malformed):
        F.decode(A.small_stream() + s)
    assert A.decode(A.small_stream() + s)["other_packets"] == 3


@pytest.mark.parametrize("name", sorted(F.bad_streams()))
def test_every_malformed_and_refused_case_by_name(name):
    data, kind, names = F.bad_streams()[name]
    with pytest.raises(kind) as e:
        F.decode(F.small_stream() + data, size=(5, 3))
    assert type(e.value) is kind
    if kind is F.Refused:
        assert e.value.value == names
    # the state is as it was: the walker that met the failure still gives the whole behind the prefix
    w, first = F.FrameWalker((5, 3)).feed(F.small_stream())
    with pytest.raises(kind):
        w.feed(data)
    assert len(w.feed(F.small_stream())[1]["rows"]) == len(first["rows"]) == 4


def test_the_small_stream_whole_cut_and_byte_by_byte():
    s = F.small_stream()
    whole = F.decode(s, size=(5, 3))
    assert [(r["channels"], r["slot"], r["ts_overflow"]) for r in whole["rows"]] == [(1, 0, 0), (3, 0, 0), (1, 0, 1), (3, 1, 1)]
    assert (whole["invalid"], whole["frame_packets"], whole["other_packets"]) == (1, 3, 1)
    for cut in range(len(s) + 1):
        w, a = F.FrameWalker((5, 3)).feed(s[:cut])
        w, b = w.feed(s[cut:])
        assert [g.tobytes() for g in a["images"] + b["images"]] == [g.tobytes() for g in whole["images"]], cut
        assert len(a["rows"]) == sum(e <= cut for e in whole["ends"]), cut  # a frame is emitted by the call that brings its last pixel byte
    w, images = F.FrameWalker((5, 3)), []
    for k in range(len(s)):
        w, o = w.feed(s[k:k + 1])
        images += o["images"]
    assert [g.tobytes() for g in images] == [g.tobytes() for g in whole["images"]]
