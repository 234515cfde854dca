"""CPU: the rosbag host walk (esvio_amd/csrc/fe_bag.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program with its own main: g++ -fsanitize=address,undefined, run directly, exit 0.  Every chunk handed to the
walk is a heap block of exactly its length, so a read outside the n bytes is a report.  Nothing here is loaded into Python.
The edge-value streams are built by tests/bag_ref.py's writer, and what the program expects of each — refused, or walked —
is what the sequential reading says."""
import os
import shutil
import struct
import subprocess

import pytest

import bag_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = (0, 1, 4095, 4096, 4097, 0xFFFFFFFF)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fe_bag.h"
using namespace esvio::bag;
static const uint8_t kBag[] = {%(bag)s};
static const size_t kLen = sizeof kBag;
static const uint8_t kEdge[] = {%(edge)s};          // the edge-value streams, one behind the other
static const uint32_t kEdgeLen[] = {%(edge_len)s};
static const int kEdgeOk[] = {%(edge_ok)s};         // what the sequential reading says: 1 walked, 0 refused
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %%d: %%s\n", __LINE__, #c); fails++; } } while (0)

static Topics topics;
struct Totals {
  uint64_t v[10];
  std::vector<uint8_t> pay[2];
  std::vector<esvio_fe_bag_message> msgs;
  std::vector<esvio_fe_imu_sample> imu;
};
// one chunk, as a heap block of exactly n bytes; outputs sized exactly by a counting walk first
static bool feed(Walk* w, Mode mode, const uint8_t* p, size_t n, Totals* t) {
  uint8_t* blk = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(blk, p, n);
  Walk probe = *w;
  const Walk before = *w;
  Out cnt;
  const bool ok = walk(&probe, topics, mode, n ? blk : nullptr, n, &cnt);
  if (ok) {
    Out o;
    std::vector<uint8_t> pay[2] = {std::vector<uint8_t>(cnt.n_events[0] * 13), std::vector<uint8_t>(cnt.n_events[1] * 13)};
    std::vector<esvio_fe_bag_message> msgs(cnt.n_msgs);
    std::vector<esvio_fe_imu_sample> imu(cnt.n_imu);
    for (int c = 0; c < 2; c++) o.payload[c] = pay[c].data(), o.events_cap[c] = cnt.n_events[c];
    o.msgs = msgs.data(), o.msgs_cap = cnt.n_msgs, o.imu = imu.data(), o.imu_cap = cnt.n_imu;
    Walk st = *w;
    CHECK(walk(&st, topics, mode, n ? blk : nullptr, n, &o));
    CHECK(memcmp(&st, &probe, sizeof st) == 0);
    CHECK(o.n_events[0] == cnt.n_events[0] && o.n_events[1] == cnt.n_events[1] && o.n_msgs == cnt.n_msgs && o.n_imu == cnt.n_imu);
    *w = st;
    const uint64_t add[10] = {o.n_events[0], o.n_events[1], o.n_cam_msgs[0], o.n_cam_msgs[1], o.n_imu, o.bad, o.other_messages, o.other_records,
                              o.chunks, o.connections};
    for (int k = 0; k < 10; k++) t->v[k] += add[k];
    for (int c = 0; c < 2; c++) t->pay[c].insert(t->pay[c].end(), pay[c].begin(), pay[c].end());
    t->msgs.insert(t->msgs.end(), msgs.begin(), msgs.end());
    t->imu.insert(t->imu.end(), imu.begin(), imu.end());
  } else {
    CHECK(cnt.why != nullptr && memcmp(w, &before, sizeof before) == 0);
  }
  free(blk);
  return ok;
}
static bool same(const Totals& a, const Totals& b) {
  return memcmp(a.v, b.v, sizeof a.v) == 0 && a.pay[0] == b.pay[0] && a.pay[1] == b.pay[1] && a.msgs.size() == b.msgs.size() &&
         (a.msgs.empty() || memcmp(a.msgs.data(), b.msgs.data(), a.msgs.size() * sizeof(esvio_fe_bag_message)) == 0) &&
         a.imu.size() == b.imu.size() && (a.imu.empty() || memcmp(a.imu.data(), b.imu.data(), a.imu.size() * sizeof(esvio_fe_imu_sample)) == 0);
}

static uint32_t rs = 12345u;
static uint32_t rnd() { return rs = rs * 1664525u + 1013904223u; }

int main() {
  const esvio_fe_bag_topics names = {"%(left)s", "%(right)s", "%(imu)s"};
  const char* why = nullptr;
  CHECK(set_topics(&names, &topics, &why));
  for (int mode = 0; mode < 2; mode++) {
    Totals whole{};
    Walk w{};
    CHECK(feed(&w, (Mode)mode, kBag, kLen, &whole));
    if (mode == kEvents) CHECK(whole.v[0] == 5 && whole.v[1] == 4 && whole.v[2] == 3 && whole.v[3] == 2 && whole.msgs.size() == 5);
    if (mode == kSide) CHECK(whole.v[4] == 2 && whole.v[5] == 0 && whole.imu.size() == 2);
    CHECK(whole.v[6] == 1 && whole.v[7] == 0 && whole.v[8] == 2 && whole.v[9] == 8);
    for (size_t cut = 0; cut <= kLen; cut++) {  // the bag cut in two at every byte
      Totals t{};
      Walk c{};
      CHECK(feed(&c, (Mode)mode, kBag, cut, &t) && feed(&c, (Mode)mode, kBag + cut, kLen - cut, &t));
      CHECK(same(t, whole));
      CHECK(c.phase == P_HLEN && c.have == 0 && !c.in_chunk);
    }
    for (size_t n = 0; n <= kLen; n += 3) {  // truncated bags, byte by byte behind them
      Totals t{};
      Walk c{};
      CHECK(feed(&c, (Mode)mode, kBag, n, &t));
      for (size_t i = n; i < kLen; i++) CHECK(feed(&c, (Mode)mode, kBag + i, 1, &t));
      CHECK(same(t, whole));
    }
    // edge values in header_len, field_len, data_len, size, n and L: refused with the state as it was, or walked
    size_t at = 0;
    for (size_t k = 0; k < sizeof kEdgeLen / sizeof kEdgeLen[0]; at += kEdgeLen[k], k++) {
      Totals t{};
      Walk c{};
      const bool ok = feed(&c, (Mode)mode, kEdge + at, kEdgeLen[k], &t);
      if (ok != (kEdgeOk[k] != 0)) fprintf(stderr, "edge stream %%zu, mode %%d: walked %%d\n", k, mode, (int)ok), fails++;
      Totals u{};
      Walk d{};
      bool ok1 = true;
      for (size_t i = 0; i < kEdgeLen[k] && ok1; i++) ok1 = feed(&d, (Mode)mode, kEdge + at + i, 1, &u);
      CHECK(ok1 == ok);
      if (ok) CHECK(same(t, u) && memcmp(&c, &d, offsetof(Walk, buf)) == 0);
    }
  }
  // 10 000 seeded random byte strings, half of them behind a valid prefix, cut at a random place
  for (int it = 0; it < 10000; it++) {
    std::vector<uint8_t> s;
    if (it & 1) s.assign(kBag, kBag + rnd() %% (kLen + 1));
    const size_t n = rnd() %% 200;
    for (size_t i = 0; i < n; i++) s.push_back((uint8_t)((it & 2) && (rnd() & 3) ? 0 : rnd() >> 24));
    const size_t cut = s.empty() ? 0 : rnd() %% (s.size() + 1);
    for (int mode = 0; mode < 2; mode++) {
      Totals t{};
      Walk c{};
      if (feed(&c, (Mode)mode, s.data(), cut, &t)) feed(&c, (Mode)mode, s.data() + cut, s.size() - cut, &t);
    }
    esvio_fe_bag_header_info hi;
    uint8_t* blk = (uint8_t*)malloc(s.size() + 13);
    memcpy(blk, kMagic, 13);
    if (!s.empty()) memcpy(blk + 13, s.data(), s.size());
    const size_t len = (it & 4) ? s.size() + 13 : rnd() %% (s.size() + 14);
    uint8_t* exact = (uint8_t*)malloc(len ? len : 1);
    memcpy(exact, blk, len);
    const int rc = file_header(exact, len, &hi);
    CHECK(rc == 0 || rc == ESVIO_FE_EINVAL);
    CHECK(hi.payload_offset <= len);
    free(exact);
    free(blk);
  }
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def edge_streams():
    """per place and edge value a stream that holds the value there, cut off after at most 5000 bytes"""
    lconn = B.connection_record(0, B.LEFT, B.EVENT_TYPE, B.EVENT_MD5)
    iconn = B.connection_record(1, B.IMU, B.IMU_TYPE, B.IMU_MD5)
    one = B.wire_events([1], [2], [3], [4], [1])
    out = []
    for v in EDGES:
        w = struct.pack("<I", v)
        room = b"x=" + b"y" * 5000
        # header_len: an op field and one that fills the rest of the header
        fill = max(v - 8 - 4 - 2, 0)
        out.append(w + B.field("op", b"\x09") + struct.pack("<I", fill + 2) + room[:fill + 2] + struct.pack("<I", 0))
        # field_len of a header's second field
        out.append(struct.pack("<I", 8 + 4 + min(v, 4200)) + B.field("op", b"\x09") + w + room[:min(v, 4200)] + struct.pack("<I", 0))
        # field_len in a role's connection data
        out.append(B.record([("conn", b"\0" * 4), ("topic", B.LEFT.encode()), ("op", b"\x07")],
                            B.field("type", B.EVENT_TYPE) + B.field("md5sum", B.EVENT_MD5) + w + room[:min(v, 4200)]))
        # data_len of a message nobody reads, of a left message, and of a chunk
        out.append(B.record([("conn", b"\0\0\0\x07"), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + w + b"z" * min(v, 4200))
        out.append(lconn + B.record([("conn", b"\0" * 4), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + w + (B.event_array(1, (1, 1), one) + b"z" * 5000)[:min(v, 4200)])
        out.append(B.record([("compression", b"none"), ("size", w), ("op", b"\x05")], b"")[:-4] + w + (lconn + iconn)[:min(v, 4200)])
        # size against a data_len of 4096
        out.append(B.record([("compression", b"none"), ("size", w), ("op", b"\x05")], b"")[:-4] + struct.pack("<I", 4096))
        # n of an EventArray whose data_len is right for n events, and for one
        for dl in (28 + 3 + 13 * v, 28 + 3 + 13):
            out.append(lconn + B.record([("conn", b"\0" * 4), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + struct.pack("<I", dl & 0xFFFFFFFF) +
                       (B.event_array(1, (1, 1), one * 400, n=v))[:min(dl, 4200)])
        # L of an EventArray and of an Imu message, data_len right for it where 32 bits can say so
        out.append(lconn + B.record([("conn", b"\0" * 4), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + struct.pack("<I", (28 + v + 13) & 0xFFFFFFFF) +
                   (struct.pack("<IIII", 1, 1, 1, v) + b"f" * min(v, 4200) + struct.pack("<III", 2, 2, 1) + one)[:4300])
        out.append(iconn + B.record([("conn", b"\x01\0\0\0"), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + struct.pack("<I", (16 + v + 296) & 0xFFFFFFFF) +
                   (struct.pack("<IIII", 1, 1, 1, v) + b"f" * min(v, 4200) + b"\0" * 296)[:4600])
    return out


def loop_walks(stream, mode):
    try:
        B.Walker(mode).feed(stream)
        return True
    except B.Malformed:
        return False
    except B.Bad:
        return True  # (a BAD stamp is not the walk's business)


def test_the_edge_streams_cover_both_outcomes():
    ok = [loop_walks(s, "events") for s in edge_streams()]
    assert 20 < sum(ok) < len(ok) - 20
    assert all(loop_walks(s, "side") == o for s, o in zip(edge_streams(), ok))


def test_the_walk_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    edges = edge_streams()
    src, exe = tmp_path / "bag_walk.cpp", tmp_path / "bag_walk"
    src.write_text(PROGRAM % {"bag": ", ".join(str(b) for b in B.small_bag()[13:]), "edge": ", ".join(str(b) for s in edges for b in s),
                              "edge_len": ", ".join(str(len(s)) for s in edges), "edge_ok": ", ".join(str(int(loop_walks(s, "events"))) for s in edges),
                              "left": B.LEFT, "right": B.RIGHT, "imu": B.IMU})
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "esvio_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures"
