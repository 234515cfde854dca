"""CPU: the sequential reading of the "rosbag images" rule (tests/bag_image_ref.py) against answers derived by hand from
the text in include/esvio_fe.h: the gray formula at its rounding edges, the channel orders, the relabelled encodings,
the row stride.  No library code runs here."""
import numpy as np
import pytest

import bag_image_ref as I
import bag_ref as B


def test_the_gray_formula_at_hand_derived_values():
    # (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15, by hand:
    #   255 * 9798 = 2498490, + 16384 = 2514874, / 32768 = 76.7   255 * 19235 = 4904925 -> 4921309 / 32768 = 150.2
    #   255 * 3735 = 952425 -> 968809 / 32768 = 29.6              255 * 32768 + 16384 -> 255.5
    #   1 * 9798 + 16384 = 26182 < 32768;  2 * 9798 + 16384 = 35980 >= 32768
    #   4 * 3735 + 16384 = 31324 < 32768;  5 * 3735 + 16384 = 35059 >= 32768
    for rgb, want in (((255, 0, 0), 76), ((0, 255, 0), 150), ((0, 0, 255), 29), ((255, 255, 255), 255), ((1, 0, 0), 0), ((2, 0, 0), 1),
                      ((0, 0, 4), 0), ((0, 0, 5), 1)):
        assert I.gray(*rgb) == want, rgb
    assert 9798 + 19235 + 3735 == 1 << 15


def test_a_triple_at_which_the_15_bit_and_the_14_bit_constants_differ():
    # brute force over all 2^24 triples, in the order R, G, B ascending, first hit: (0, 0, 250)
    #   15 bit: 250 * 3735 = 933750, + 16384 = 950134, >> 15 = 28 (28 * 32768 = 917504, 29 * 32768 = 950272 > 950134)
    #   14 bit: 250 * 1868 = 467000, +  8192 = 475192, >> 14 = 29 (29 * 16384 = 475136 <= 475192)
    assert (I.gray(0, 0, 250), I.gray14(0, 0, 250)) == (28, 29)
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    first, differ = None, 0
    for r in range(256):
        a = (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
        c = (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14
        assert 0 <= int(a.min()) and int(a.max()) <= 255
        hits = np.argwhere(a != c)
        differ += len(hits)
        if first is None and len(hits):
            first = (r, int(hits[0][0]), int(hits[0][1]))
    assert first == (0, 0, 250) and 0 < differ < (1 << 24) // 10


def test_bgr_is_rgb_with_the_channels_swapped_and_the_relabelled_names_are_their_classes():
    px = I.test_image(4, 6, 3, 5)
    rgb = I.convert(px.tobytes(), 4, 6, 18, "rgb8")
    swapped = px.reshape(4, 6, 3)[:, :, ::-1].reshape(4, 18)
    assert np.array_equal(I.convert(swapped.tobytes(), 4, 6, 18, "bgr8"), rgb)
    assert not np.array_equal(I.convert(px.tobytes(), 4, 6, 18, "bgr8"), rgb)
    assert np.array_equal(I.convert(px.tobytes(), 4, 6, 18, "8UC3"), I.convert(px.tobytes(), 4, 6, 18, "bgr8"))
    mono = I.test_image(4, 6, 1, 6)
    assert np.array_equal(I.convert(mono.tobytes(), 4, 6, 6, "8UC1"), mono)
    assert np.array_equal(I.convert(mono.tobytes(), 4, 6, 6, "mono8"), mono)
    assert rgb[0, 0] == I.gray(int(px[0, 0]), int(px[0, 1]), int(px[0, 2]))
    with pytest.raises(KeyError):
        I.convert(mono.tobytes(), 4, 6, 6, "mono16")


def test_a_3x2_image_with_five_padding_bytes_per_row_ignores_them():
    for cls, name in ((1, "mono8"), (2, "bgr8"), (3, "rgb8")):
        px = I.test_image(2, 3, cls, 9 + cls)
        step = 3 * I.BPP[cls] + 5
        want = I.convert(px.tobytes(), 2, 3, 3 * I.BPP[cls], name)
        for fill in (0x00, 0xEE, 0xFF):
            data = I.rows(px, step, fill)
            assert len(data) == 2 * step and data[3 * I.BPP[cls]] == fill
            assert np.array_equal(I.convert(data, 2, 3, step, name), want), (name, fill)
            assert np.array_equal(I.convert_rows(data, 2, 3, step, cls), want)


def test_the_array_form_equals_the_loops_on_a_seeded_image_per_class():
    for cls, name in ((1, "8UC1"), (2, "8UC3"), (3, "rgb8")):
        px = I.test_image(17, 23, cls, 20 + cls)
        data = I.rows(px, 23 * I.BPP[cls] + 3)
        assert np.array_equal(I.convert_rows(data, 17, 23, 23 * I.BPP[cls] + 3, cls), I.convert(data, 17, 23, 23 * I.BPP[cls] + 3, name))


def test_the_small_bag_read_whole_and_the_walker_as_a_value():
    bag = I.small_bag()
    o = I.decode(bag, size=(5, 3))
    assert [len(v) for v in o["images"]] == [3, 2] and o["table"]["cam"].tolist() == [0, 1, 1, 0, 0]
    assert o["table"]["index"].tolist() == [0, 0, 1, 1, 2] and o["table"]["encoding"].tolist() == [1, 3, 2, 2, 1]
    assert o["table"]["step"].tolist() == [5, 20, 16, 31, 8] and o["table"]["is_bigendian"].tolist() == [1, 1, 0, 0, 1]
    assert (o["chunks"], o["other_messages"]) == (3, 4)  # events of two topics, IMU and odometry are other messages here
    assert np.array_equal(o["images"][0][0], I.test_image(3, 5, 1, 41))
    w = I.ImageWalker(size=(5, 3))
    s = bag[13:]
    w1, a = w.feed(s[:700])
    w2, b = w1.feed(s[700:])
    assert len(a["table"]) + len(b["table"]) == 5 and b["table"]["index"][0] == 0  # the index counts per call
    assert w.history == b"" and w1.feed(s[700:])[1]["table"].tobytes() == b["table"].tobytes()
    for name, (stream, names) in I.bad_streams().items():
        with pytest.raises(B.Malformed) as e:
            I.ImageWalker(size=(5, 3)).feed(stream)
        assert names in str(e.value), name
        assert isinstance(e.value, I.Refused) == (name in ("mono16", "bayer_rggb8", "an empty encoding", "Mono8 in capitals", "another size",
                                                           "width and height swapped")), name
