"""tests/text_ref.py, the sequential reading of include/esvio_fe.h "text event files": hand-derived answers, one case per
line of the rule; its numbers against Python's own decimal.Decimal and int(); round trips through the cited writers'
lines.  No device, no library."""
import decimal

import numpy as np

import text_ref as T

D, U, N = T.SEC_DECIMAL, T.INT_US, T.INT_NS


def ev(body, order=T.TXYP, time=D, off=0):
    cls, rec = T.classify(body, order, time, off)
    return cls if rec is None else rec[:5]


def test_the_line_classes_by_hand():
    assert ev(b"1.5 3 4 1") == (3, 4, 1, 500000000, 1)                    # the davis extractor's line
    assert ev(b"3 4 1 1500000", T.XYPT, U) == (3, 4, 1, 500000000, 1)      # the dvs extractor's, writer.cpp's
    assert ev(b"3,4,1,1500000", T.XYPT, U) == (3, 4, 1, 500000000, 1)      # a Prophesee CSV line
    assert ev(b"3 4 0 1500000123", T.XYPT, N) == (3, 4, 1, 500000123, 0)
    # 1. more than 64 bytes
    body = b"1.5 3 4 1" + b" " * 55
    assert len(body) == 64 and ev(body) == (3, 4, 1, 500000000, 1) and ev(body + b" ") == "malformed"
    assert ev(b"#" + b"x" * 63) == "comment" and ev(b"#" + b"x" * 64) == "malformed"
    # 2. separators stripped; nothing left: blank
    assert ev(b"") == "blank" and ev(b" \t, ,") == "blank" and ev(b" ,\t1.5 3 4 1,, ") == (3, 4, 1, 500000000, 1)
    # 3. comments
    assert ev(b"# t x y p") == "comment" and ev(b"  % 1 2 3 4 5") == "comment" and ev(b"%") == "comment"
    # 4. runs of separators; exactly four tokens
    assert ev(b"1.5 ,\t 3\t\t4,1") == (3, 4, 1, 500000000, 1)
    assert ev(b"1.5 3 4") == "malformed" and ev(b"1.5 3 4 1 0") == "malformed" and ev(b"x") == "malformed"
    # 5. x, y
    assert ev(b"0 65535 65535 0") == (65535, 65535, 0, 0, 0) and ev(b"0 65536 0 0") == "malformed"
    assert ev(b"0 00007 007 0") == (7, 7, 0, 0, 0) and ev(b"0 000007 7 0") == "malformed"
    assert ev(b"0 -1 7 0") == "malformed" and ev(b"0 7 1e2 0") == "malformed" and ev(b"0 7 +1 0") == "malformed"
    # p
    assert ev(b"0 1 2 -1") == (1, 2, 0, 0, 0) and ev(b"0 1 2 1") == (1, 2, 0, 0, 1)
    for p in (b"2", b"+1", b"-0", b"01", b"00", b"-", b"1.0", b"--1"):
        assert ev(b"0 1 2 " + p) == "malformed", p
    # t, SEC_DECIMAL
    assert ev(b"7 1 2 0") == (1, 2, 7, 0, 0) and ev(b"7.1 1 2 0") == (1, 2, 7, 100000000, 0)
    assert ev(b"7.123456789 1 2 0") == (1, 2, 7, 123456789, 0)
    assert ev(b"7.1234567899 1 2 0") == (1, 2, 7, 123456789, 0)   # truncation, not rounding
    assert ev(b"7.999999999999 1 2 0") == (1, 2, 7, 999999999, 0)
    assert ev(b"0000000007.5 1 2 0") == (1, 2, 7, 500000000, 0) and ev(b"00000000007.5 1 2 0") == "malformed"
    for t in (b".5", b"5.", b"1e5", b"1E5", b"+5", b"-5", b"5.5.5", b"5.1234567890x", b"5\x00", b"0x10", b"nan"):
        assert ev(t + b" 1 2 0") == "malformed", t
    # t, integers: 1 to 19 digits
    assert ev(b"1 2 0 0000000000000000042", T.XYPT, U) == (1, 2, 0, 42000, 0)
    assert ev(b"1 2 0 00000000000000000042", T.XYPT, U) == "malformed"       # 20 digits
    assert ev(b"1 2 0 4.2", T.XYPT, U) == "malformed" and ev(b"1 2 0 4.2", T.XYPT, N) == "malformed"
    # the order decides which token is which
    assert ev(b"65536 1 2 0") == (1, 2, 65536, 0, 0) and ev(b"65536 1 0 2", T.XYPT, U) == "malformed"
    # a malformed token wins over a BAD stamp
    assert ev(b"4294967296.0 1 2 2") == "malformed" and ev(b"4294967296.0 1 2 1") == "bad"


def test_stamps_and_bad_by_hand():
    assert ev(b"4294967295.999999999 1 2 0") == (1, 2, 4294967295, 999999999, 0)
    assert ev(b"4294967296 1 2 0") == "bad" and ev(b"9999999999.9 1 2 0") == "bad"
    assert ev(b"1 2 0 4294967295999999", T.XYPT, U) == (1, 2, 4294967295, 999999000, 0)
    assert ev(b"1 2 0 4294967296000000", T.XYPT, U) == "bad"
    assert ev(b"1 2 0 9999999999999999999", T.XYPT, U) == "bad"      # 19 digits: never wraps
    assert ev(b"1 2 0 9999999999999999999", T.XYPT, N) == "bad"
    assert ev(b"1 2 0 9999999999999999999", T.XYPT, N, -(1 << 62)) == "bad"
    assert ev(b"1 2 0 4611686018427387904", T.XYPT, N, -(1 << 62)) == (1, 2, 0, 0, 0)
    assert ev(b"1 2 0 4611686018427387903", T.XYPT, N, -(1 << 62)) == "bad"   # ticks == -1
    assert ev(b"0.000000005 1 2 0", off=-6) == "bad" and ev(b"0.000000005 1 2 0", off=-5) == (1, 2, 0, 0, 0)
    assert ev(b"4294967295.999999999 1 2 0", off=1) == "bad"
    assert ev(b"0 1 2 0", off=(1 << 62)) == "bad"
    assert ev(b"0 1 2 0", off=T.TICK_LIMIT - 1) == (1, 2, 4294967295, 999999999, 0)


def rd(data, order=T.TXYP, time=D, flags=0, state=None, off=0, cap=None):
    return T.read(state or T.fresh(), order, time, flags, data, off, cap)


def test_lines_terminators_and_the_state_by_hand():
    recs, info, ok, st = rd(b"1.5 3 4 1\r\n# c\n\n \r\n2 3 4 0\nx\n3 1 1 1")
    assert not ok and info["malformed"] == 1 and info["first_malformed"] == 27 and st == T.fresh()
    recs, info, ok, st = rd(b"1.5 3 4 1\r\n# c\n\n \r\n2 3 4 0\nx\n3 1 1 1", flags=T.SKIP_MALFORMED)
    assert ok and recs == [(3, 4, 1, 500000000, 1), (3, 4, 2, 0, 0)]
    assert {k: info[k] for k in ("events", "lines", "comments", "blank", "malformed", "bad", "first_malformed", "carried")} == \
        dict(events=2, lines=6, comments=1, blank=2, malformed=1, bad=0, first_malformed=27, carried=7)
    assert info["first_t_ns"] == 1500000000 and info["last_t_ns"] == 2000000000 and st["tail"] == b"3 1 1 1"
    # the tail is a line of the call that holds its terminator; first_malformed is negative for a line begun in the tail
    recs, info, ok, st2 = rd(b"\n", state=st)
    assert ok and recs == [(1, 1, 3, 0, 1)] and info["carried"] == 0
    recs, info, ok, st2 = rd(b"x\n", state=st)
    assert not ok and info["first_malformed"] == -7 and st2 == st
    # END: a non-empty tail is a line; a '\r' without '\n' is a byte of the body
    recs, info, ok, st2 = rd(b"", state=st, flags=T.END)
    assert ok and recs == [(1, 1, 3, 0, 1)] and st2 == T.fresh() and info["lines"] == 1
    assert not rd(b"3 1 1 1\r", flags=T.END)[2] and rd(b"3 1 1 1\r")[3]["tail"] == b"3 1 1 1\r"
    # '\r' and '\n' in different calls
    recs, info, ok, st2 = rd(b"\n", state=rd(b"3 1 1 1\r")[3])
    assert ok and recs == [(1, 1, 3, 0, 1)]
    # 64 bytes of body and a '\r' wait as a tail; one more byte and the line is being discarded
    body = b"3 1 1 1" + b" " * 57
    st = rd(body + b"\r")[3]
    assert len(st["tail"]) == 65 and not st["skip"] and rd(b"\n", state=st)[0] == [(1, 1, 3, 0, 1)]
    st = rd(body + b" ")[3]
    assert st == {"tail": b"", "skip": True, "skip_len": 65}
    st = rd(b"abc", state=st)[3]
    assert st["skip_len"] == 68
    recs, info, ok, st2 = rd(b"def\n4 1 1 1\n", state=st, flags=T.SKIP_MALFORMED)
    assert ok and recs == [(1, 1, 4, 0, 1)] and info["malformed"] == 1 and info["first_malformed"] == -68 and info["lines"] == 2
    recs, info, ok, st2 = rd(b"", state=st, flags=T.END | T.SKIP_MALFORMED)
    assert ok and info["malformed"] == 1 and info["first_malformed"] == -68 and st2 == T.fresh()
    # failures leave the state; BAD and lack of room count exactly
    recs, info, ok, st2 = rd(b"4294967296 1 1 1\n1 1 1 1\n5", state=None)
    assert not ok and info["bad"] == 1 and info["events"] == 2 and st2 == T.fresh()
    recs, info, ok, st2 = rd(b"1 1 1 1\n2 1 1 1\n", cap=1)
    assert not ok and info["events"] == 2
    assert rd(b"1 1 1 1\n2 1 1 1\n", cap=2)[2]


def test_sec_decimal_tokens_equal_decimal_decimal():
    rng = np.random.default_rng(3)
    q = decimal.Decimal(1).scaleb(-9)
    ctx = decimal.Context(prec=60, rounding=decimal.ROUND_DOWN)
    tokens = ["0", "0.0", "4294967295.999999999", "1.000000001", "1.0000000019", "9.99999999999999", "0000000001.5"]
    for _ in range(3000):
        whole = str(int(rng.integers(0, 1 << 32))) if rng.random() < 0.8 else "0" * int(rng.integers(0, 4)) + str(int(rng.integers(0, 1000)))
        nf = int(rng.integers(0, 15))
        tokens.append(whole + ("." + "".join(str(int(d)) for d in rng.integers(0, 10, nf)) if nf else ""))
    for tok in tokens:
        if len(tok.split(".")[0]) > 10:
            continue
        cls, rec = T.classify(tok.encode() + b" 1 2 0", T.TXYP, D)
        want = decimal.Decimal(tok).quantize(q, context=ctx)
        assert cls == "event" and decimal.Decimal(rec[2]) + decimal.Decimal(rec[3]) * q == want, tok
        assert 0 <= rec[3] < 10 ** 9


def test_integer_tokens_equal_int():
    rng = np.random.default_rng(4)
    for _ in range(3000):
        nd = int(rng.integers(1, 20))
        tok = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        for time, mul in ((U, 1000), (N, 1)):
            cls, rec = T.classify(b"1 2 1 " + tok.encode(), T.XYPT, time)
            ns = int(tok) * mul
            if ns >= T.TICK_LIMIT:
                assert cls == "bad", tok
            else:
                assert cls == "event" and rec[2] * 10 ** 9 + rec[3] == ns, tok


def _events(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, 1 << 62, n) % T.TICK_LIMIT)
    return [(int(x), int(y), int(tt // 10 ** 9), int(tt % 10 ** 9), int(p))
            for x, y, tt, p in zip(rng.integers(0, 65536, n), rng.integers(0, 65536, n), t, rng.integers(0, 2, n))]


def test_round_trip_of_the_davis_writer_is_exact():
    events = _events(2000, 5) + [(0, 0, 0, 0, 0), (65535, 65535, 4294967295, 999999999, 1), (1, 2, 3, 4, 1)]
    recs, info, ok, st = rd(T.write_davis(events))
    assert ok and recs == events and info["events"] == info["lines"] == len(events) and st == T.fresh()


def test_round_trip_of_the_dvs_writers_floors_to_microseconds():
    events = _events(2000, 6) + [(0, 0, 0, 999, 0), (65535, 65535, 4294967295, 999999999, 1)]
    floored = [(x, y, s, ns // 1000 * 1000, p) for x, y, s, ns, p in events]
    for write in (T.write_dvs, T.write_cpp, T.write_csv):
        recs, info, ok, st = rd(write(events), T.XYPT, U)
        assert ok and recs == floored and info["events"] == len(events)


def test_reading_in_pieces_equals_reading_whole():
    data = (b"# header\r\n1.5 3 4 1\n\n2.25,5,6,0\r\n" + b"7" * 70 + b"\n3 1 1 1\nbad line\n" + b" " * 64 + b"\r\n4 1 1 -1")
    whole = rd(data, flags=T.END | T.SKIP_MALFORMED)
    assert whole[2] and whole[1]["malformed"] == 2 and whole[1]["events"] == 4
    for cut in range(len(data) + 1):
        a = rd(data[:cut], flags=T.SKIP_MALFORMED)
        b = rd(data[cut:], flags=T.END | T.SKIP_MALFORMED, state=a[3])
        assert a[2] and b[2] and a[0] + b[0] == whole[0], cut
        for k in ("events", "lines", "comments", "blank", "malformed", "bad"):
            assert a[1][k] + b[1][k] == whole[1][k], (cut, k)
