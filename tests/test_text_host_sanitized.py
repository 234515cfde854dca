"""CPU: the host side of the text event files (esvio_amd/csrc/fe_text.h: the carry step, the sequential decode around it,
the two side parsers) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program with its own main:
g++ -fsanitize=address,undefined, run directly, exit 0.  Every chunk handed over is a heap block of exactly its length,
so a read outside the n bytes is a report.  Nothing here is loaded into Python.  What the program expects — records,
counts, the tail behind every cut — is what tests/text_ref.py says."""
import os
import re
import shutil
import subprocess

import pytest

import text_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every line class; an overlong line (it spans three chunks of 40 bytes); CRLF; a 64-byte body; no terminator at the end
STREAM = (b"# t x y p\r\n1.5 3 4 1\n\n , \r\n2.25,5,6,0\r\n" + b"7" * 97 + b"\n3.000000001\t65535\t0\t-1\nbad line\n4294967295.999999999 1 1 1\n" +
          b"5 1 1 1" + b" " * 57 + b"\r\n" + b"9" * 64 + b"\n6 2 2 0")
IMU = b"# imu\n1.5 0.1 -9.81 1e-05 0 3.25 -0.5\r\n\n2.000000001,1,2,3,4,5,6\n3 inf -inf 0.30000000000000004 1E3 -0.0 7"
IMAGES = b"0.100000000 images/frame_00000000.png\n1.5\timages/frame 1,a.png \r\n% c\n2 x"

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fe_text.h"
using namespace esvio::text;
static const uint8_t kStream[] = {%(stream)s};
static const size_t kLen = sizeof kStream;
static const Event kWant[] = {%(records)s};
static const size_t kWantN = sizeof kWant / sizeof kWant[0];
static const uint64_t kCounts[6] = {%(counts)s};   // events, lines, comments, blank, malformed, bad
static const long long kFirstMalformed = %(first_malformed)s;
static const uint32_t kCarried[] = {%(carried)s};  // the tail behind the first `cut` bytes
static const uint8_t kSkip[] = {%(skip)s};         // ... or inside an overlong line
static const uint8_t kImu[] = {%(imu)s};
static const ImuSample kImuWant[] = {%(imu_want)s};
static const uint8_t kImages[] = {%(images)s};
static const long long kImgStamp[] = {%(img_stamp)s};
static const uint64_t kImgOff[] = {%(img_off)s};
static const uint32_t kImgLen[] = {%(img_len)s};
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %%d: %%s\n", __LINE__, #c); fails++; } } while (0)

struct Totals {
  std::vector<Event> ev;
  uint64_t v[6] = {0, 0, 0, 0, 0, 0};
};
// one chunk as a heap block of exactly n bytes, dst with exactly the room the bound promises
static bool feed(State* st, uint32_t flags, const uint8_t* p, size_t n, Totals* t, Counts* out = nullptr) {
  uint8_t* blk = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(blk, p, n);
  const size_t cap = (n + kMaxTail) / 8 + 1;
  std::vector<Event> dst(cap);
  const Format f{kTxyp, kSecDecimal, flags};
  const State before = *st;
  Counts c;
  const int rc = decode_chunk(st, f, blk, n, 0, dst.data(), cap, &c);
  if (rc == 0) {
    CHECK(c.events <= cap && c.lines == c.events + c.comments + c.blank + c.malformed && c.carried == st->len);
    t->ev.insert(t->ev.end(), dst.begin(), dst.begin() + c.events);
    const uint64_t add[6] = {c.events, c.lines, c.comments, c.blank, c.malformed, c.bad};
    for (int k = 0; k < 6; k++) t->v[k] += add[k];
    if (!(flags & kEnd)) {  // the carry step alone leaves the same state
      State s2 = before;
      carry(&s2, blk, n);
      CHECK(s2.len == st->len && s2.skip == st->skip && s2.skip_len == st->skip_len && memcmp(s2.tail, st->tail, st->len) == 0);
    }
  } else {
    CHECK(memcmp(st, &before, sizeof before) == 0);
  }
  if (out) *out = c;
  free(blk);
  return rc == 0;
}
static bool whole(const Totals& t) {
  return t.ev.size() == kWantN && memcmp(t.ev.data(), kWant, sizeof kWant) == 0 && memcmp(t.v, kCounts, sizeof kCounts) == 0;
}

int main() {
  {
    Totals t;
    State st;
    Counts c;
    CHECK(feed(&st, kEnd | kSkipMalformed, kStream, kLen, &t, &c) && whole(t));
    CHECK(c.first_malformed == kFirstMalformed && st.len == 0 && !st.skip);
    State st2;
    Totals t2;
    CHECK(!feed(&st2, kEnd, kStream, kLen, &t2, &c));  // a malformed line without SKIP_MALFORMED: refused, counts exact
    CHECK(c.malformed == kCounts[4] && c.events == kCounts[0] && c.first_malformed == kFirstMalformed);
  }
  for (size_t cut = 0; cut <= kLen; cut++) {  // cut in two at every byte
    Totals t;
    State st;
    CHECK(feed(&st, kSkipMalformed, kStream, cut, &t));
    CHECK(st.len == kCarried[cut] && st.skip == kSkip[cut]);
    CHECK(feed(&st, kEnd | kSkipMalformed, kStream + cut, kLen - cut, &t) && whole(t));
  }
  for (size_t step = 1; step <= 40; step += 39) {  // one byte per call; 40 bytes per call: the overlong line spans three chunks
    Totals t;
    State st;
    for (size_t at = 0; at < kLen; at += step) {
      CHECK(feed(&st, kSkipMalformed, kStream + at, kLen - at < step ? kLen - at : step, &t));
      const size_t end = at + step < kLen ? at + step : kLen;
      CHECK(st.len == kCarried[end] && st.skip == kSkip[end]);
    }
    CHECK(feed(&st, kEnd | kSkipMalformed, nullptr, 0, &t) && whole(t));
  }
  {  // a first malformed line that began in the tail, and one that began calls ago
    Totals t;
    State st;
    Counts c;
    CHECK(feed(&st, 0, (const uint8_t*)"1 1 1 1\nab", 10, &t));
    CHECK(!feed(&st, 0, (const uint8_t*)"c\n", 2, &t, &c) && c.first_malformed == -2 && st.len == 2);
    State s2;
    std::vector<uint8_t> longline(100, 'x');
    CHECK(feed(&s2, 0, longline.data(), 100, &t) && s2.skip && s2.skip_len == 100);
    CHECK(feed(&s2, 0, longline.data(), 7, &t) && s2.skip_len == 107);
    CHECK(!feed(&s2, 0, (const uint8_t*)"\n", 1, &t, &c) && c.first_malformed == -107 && c.malformed == 1);
    CHECK(feed(&s2, kSkipMalformed, (const uint8_t*)"\n", 1, &t, &c) && !s2.skip && s2.len == 0);
  }
  // the side files: whole, as heap blocks of exactly their length; then every prefix (any outcome, no bad read)
  {
    const size_t n = sizeof kImu, want = sizeof kImuWant / sizeof kImuWant[0];
    for (size_t len = 0; len <= n; len++) {
      uint8_t* blk = (uint8_t*)malloc(len ? len : 1);
      memcpy(blk, kImu, len);
      std::vector<ImuSample> out(want);
      size_t got = 0;
      const int rc = parse_imu(blk, len, 0, out.data(), want, &got);
      CHECK(rc == 0 || rc == -1);
      if (len == n) {
        CHECK(rc == 0 && got == want);
        for (size_t k = 0; k < want && rc == 0; k++) {
          CHECK(out[k].sec == kImuWant[k].sec && out[k].nsec == kImuWant[k].nsec);
          CHECK(memcmp(out[k].acc, kImuWant[k].acc, sizeof out[k].acc) == 0 && memcmp(out[k].gyr, kImuWant[k].gyr, sizeof out[k].gyr) == 0);
        }
        CHECK(parse_imu(blk, len, 0, out.data(), 1, &got) == -2 && got == want);
        CHECK(parse_imu(blk, len, -1600000000, out.data(), want, &got) == -1 && got == 0);  // BAD: the first stamp is 1.5 s
      }
      free(blk);
    }
  }
  {
    const size_t n = sizeof kImages, want = sizeof kImgStamp / sizeof kImgStamp[0];
    for (size_t len = 0; len <= n; len++) {
      uint8_t* blk = (uint8_t*)malloc(len ? len : 1);
      memcpy(blk, kImages, len);
      std::vector<int64_t> st(want);
      std::vector<uint64_t> off(want);
      std::vector<uint32_t> ln(want);
      size_t got = 0;
      const int rc = parse_images(blk, len, 0, st.data(), off.data(), ln.data(), want, &got);
      CHECK(rc == 0 || rc == -1);
      for (size_t k = 0; k < got && k < want; k++) CHECK(off[k] + ln[k] <= len);
      if (len == n) {
        CHECK(rc == 0 && got == want);
        for (size_t k = 0; k < want && rc == 0; k++) CHECK(st[k] == kImgStamp[k] && off[k] == kImgOff[k] && ln[k] == kImgLen[k]);
      }
      free(blk);
    }
    size_t got = 9;
    CHECK(parse_images((const uint8_t*)"1.5\n", 4, 0, nullptr, nullptr, nullptr, 0, &got) == -1 && got == 0);  // no path
    CHECK(parse_imu((const uint8_t*)"1.5 1 2 3 4 5\n", 14, 0, nullptr, 0, &got) == -1);                       // six columns
    CHECK(parse_imu((const uint8_t*)"1.5 1 2 3 4 5 +6\n", 17, 0, nullptr, 0, &got) == -1);
    CHECK(parse_imu((const uint8_t*)"1.5 1 2 3 4 5 6 7\n", 18, 0, nullptr, 0, &got) == -1);
  }
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def expectations():
    recs, info, ok, st = T.read(T.fresh(), T.TXYP, T.SEC_DECIMAL, T.END | T.SKIP_MALFORMED, STREAM)
    assert ok and info["events"] == 6 and info["comments"] == 1 and info["blank"] == 2 and info["malformed"] == 3
    states = [T.read(T.fresh(), T.TXYP, T.SEC_DECIMAL, T.SKIP_MALFORMED, STREAM[:cut])[3] for cut in range(len(STREAM) + 1)]
    assert any(s["skip"] for s in states) and max(len(s["tail"]) for s in states) == 65
    return recs, info, states


def imu_expectations():
    out = []
    for line in IMU.replace(b"\r", b"").split(b"\n"):
        tok = line.replace(b",", b" ").split()
        if not tok or tok[0].startswith(b"#"):
            continue
        cls, rec = T.classify(tok[0] + b" 0 0 0", T.TXYP, T.SEC_DECIMAL)
        out.append((rec[2], rec[3], [float(v) for v in tok[1:7]]))
    return out


def image_expectations():
    out, pos = [], 0
    for line in IMAGES.split(b"\n"):
        body = line.rstrip(b"\r").rstrip(b" \t,")
        if body and body[:1] not in (b"#", b"%"):
            stamp = re.split(rb"[ \t]", body, maxsplit=1)[0]
            path = body[len(stamp):].lstrip(b" \t")
            cls, rec = T.classify(stamp + b" 0 0 0", T.TXYP, T.SEC_DECIMAL)
            out.append((rec[5], pos + len(body) - len(path), len(path), path))
        pos += len(line) + 1
    return out


def test_the_expectations_hold_every_case():
    recs, info, states = expectations()
    assert recs[2] == (65535, 0, 3, 1, 0) and recs[3] == (1, 1, 4294967295, 999999999, 1)
    imu = imu_expectations()
    assert len(imu) == 3 and imu[0][:2] == (1, 500000000) and imu[0][2][2] == 1e-05 and imu[2][2][0] == float("inf")
    img = image_expectations()
    assert [i[3] for i in img] == [b"images/frame_00000000.png", b"images/frame 1,a.png", b"x"] and img[1][0] == 1500000000
    assert all(IMAGES[o:o + n] == p for _, o, n, p in img)


def _c_double(v):
    return "INFINITY" if v == float("inf") else "-INFINITY" if v == float("-inf") else v.hex()


def test_the_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    recs, info, states = expectations()
    blist = lambda b: ", ".join(str(x) for x in b)  # noqa: E731
    src, exe = tmp_path / "text_host.cpp", tmp_path / "text_host"
    src.write_text(PROGRAM % {
        "stream": blist(STREAM),
        "records": ", ".join("{%d, %d, %du, %du, %d, {0, 0, 0}}" % r for r in recs),
        "counts": ", ".join(str(info[k]) for k in ("events", "lines", "comments", "blank", "malformed", "bad")),
        "first_malformed": info["first_malformed"],
        "carried": ", ".join(str(len(s["tail"])) for s in states), "skip": ", ".join(str(int(s["skip"])) for s in states),
        "imu": blist(IMU),
        "imu_want": ", ".join("{%du, %du, {%s}, {%s}}" % (s, ns, ", ".join(_c_double(v) for v in vals[:3]), ", ".join(_c_double(v) for v in vals[3:]))
                              for s, ns, vals in imu_expectations()),
        "images": blist(IMAGES),
        "img_stamp": ", ".join("%dLL" % i[0] for i in image_expectations()),
        "img_off": ", ".join(str(i[1]) for i in image_expectations()), "img_len": ", ".join(str(i[2]) for i in image_expectations())})
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "esvio_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures"
