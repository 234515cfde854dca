"""CPU: the rosbag host walk in its image mode (esvio_amd/csrc/fe_bag.h) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program with its own main: g++ -fsanitize=address,undefined, run directly,
exit 0.  Every chunk handed to the walk is a heap block of exactly its length and every output is sized exactly by a
counting walk, so a read or a write outside them is a report.  Nothing here is loaded into Python.  The streams are built
by tests/bag_image_ref.py's writer, and what the program expects of each — refused, or walked, and the bytes gathered — is
what the sequential reading says."""
import os
import shutil
import struct
import subprocess

import pytest

import bag_image_ref as I
import bag_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = (0, 1, 32, 33, 4096, 0xFFFFFFFF)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fe_bag.h"
using namespace esvio::bag;
static const uint8_t kBag[] = {%(bag)s};
static const size_t kLen = sizeof kBag;
static const uint8_t kWant[] = {%(want)s};          // the payloads the sequential reading gathers, one behind the other
static const uint8_t kEdge[] = {%(edge)s};          // the bad and the edge-value streams, one behind the other
static const uint32_t kEdgeLen[] = {%(edge_len)s};
static const int kEdgeOk[] = {%(edge_ok)s};         // what the sequential reading says: 1 walked, 0 refused
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %%d: %%s\n", __LINE__, #c); fails++; } } while (0)

static Topics topics;
struct Totals {
  uint64_t v[7];
  std::vector<uint8_t> pay;  // the payloads without their padding
  std::vector<esvio_fe_bag_image> imgs;
};
struct Walker {
  Walk w{};
  Carry carry;
};
// one chunk, as a heap block of exactly n bytes; outputs sized exactly by a counting walk first, as the library's call does
static bool feed(Walker* k, const uint8_t* p, size_t n, Totals* t) {
  uint8_t* blk = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(blk, p, n);
  Walk probe = k->w;
  const Walk before = k->w;
  const std::vector<uint8_t> waiting(k->carry.buf[before.carry_buf & 1u].begin(), k->carry.buf[before.carry_buf & 1u].begin() + (size_t)before.carry_len);
  Out cnt;
  cnt.want_w = 5, cnt.want_h = 3;
  const bool ok = walk(&probe, topics, kImages, n ? blk : nullptr, n, &cnt);
  if (ok) {
    Out o;
    o.want_w = 5, o.want_h = 3, o.carry = &k->carry;
    std::vector<uint8_t> pix(cnt.n_pix_bytes);
    std::vector<esvio_fe_bag_image> imgs(cnt.n_imgs);
    o.pix = pix.data(), o.pix_cap = pix.size(), o.imgs = imgs.data(), o.imgs_cap = imgs.size();
    Walk st = k->w;
    CHECK(walk(&st, topics, kImages, n ? blk : nullptr, n, &o));
    CHECK(memcmp(&st, &probe, sizeof st) == 0);
    CHECK(o.n_imgs == cnt.n_imgs && o.n_pix_bytes == cnt.n_pix_bytes);
    // what waited at the call's start is where it was: a call that failed behind its gathering walk would go back to it
    CHECK(k->carry.buf[before.carry_buf & 1u].size() >= waiting.size() &&
          (waiting.empty() || memcmp(k->carry.buf[before.carry_buf & 1u].data(), waiting.data(), waiting.size()) == 0));
    k->w = st;
    const uint64_t add[7] = {o.n_imgs, o.n_cam_imgs[0], o.n_cam_imgs[1], o.other_messages, o.other_records, o.chunks, o.connections};
    for (int i = 0; i < 7; i++) t->v[i] += add[i];
    size_t at = 0;
    for (const esvio_fe_bag_image& m : imgs) {
      const size_t d = (size_t)m.step * m.height;
      t->pay.insert(t->pay.end(), pix.begin() + at, pix.begin() + at + d);
      at += (d + 15) & ~(size_t)15;
    }
    CHECK(at == pix.size());
    t->imgs.insert(t->imgs.end(), imgs.begin(), imgs.end());
  } else {
    CHECK(cnt.why != nullptr && memcmp(&k->w, &before, sizeof before) == 0);
  }
  free(blk);
  return ok;
}
static bool same_but_index(const Totals& a, const Totals& b) {
  if (memcmp(a.v, b.v, sizeof a.v) != 0 || a.pay != b.pay || a.imgs.size() != b.imgs.size()) return false;
  for (size_t k = 0; k < a.imgs.size(); k++)  // (the index counts per call)
    if (memcmp(&a.imgs[k], &b.imgs[k], offsetof(esvio_fe_bag_image, index)) != 0) return false;
  return true;
}

static uint32_t rs = 4321u;
static uint32_t rnd() { return rs = rs * 1664525u + 1013904223u; }

int main() {
  const esvio_fe_bag_topics names = {"%(ev_left)s", "%(ev_right)s", "%(imu)s"};
  const char* why = nullptr;
  CHECK(set_topics(&names, &topics, &why));
  // the topic rules: the string rules, and no image topic may be one that has a role from set_topics
  CHECK(!set_image_topics("%(ev_left)s", nullptr, &topics, &why) && why != nullptr);
  CHECK(!set_image_topics("/a", "%(imu)s", &topics, &why));
  CHECK(!set_image_topics("/a", "/a", &topics, &why) && !set_image_topics("", nullptr, &topics, &why));
  CHECK(topics.len[3] == 0 && topics.len[4] == 0);  // (a refused call leaves the topics as they were)
  CHECK(set_image_topics("%(left)s", "%(right)s", &topics, &why));
  CHECK(set_topics(&names, &topics, &why) && topics.len[3] != 0);  // (the event topics' call keeps the image topics)

  Totals whole{};
  {
    Walker k;
    CHECK(feed(&k, kBag, kLen, &whole));
    CHECK(whole.v[0] == 5 && whole.v[1] == 3 && whole.v[2] == 2 && whole.v[3] == 4 && whole.v[5] == 3);
    CHECK(whole.pay.size() == sizeof kWant && memcmp(whole.pay.data(), kWant, sizeof kWant) == 0);
    CHECK(whole.imgs[3].index == 1 && whole.imgs[3].step == 31 && whole.imgs[3].encoding == kEncBgr);
  }
  for (size_t cut = 0; cut <= kLen; cut++) {  // the bag cut in two at every byte: the carry across the calls
    Totals t{};
    Walker k;
    CHECK(feed(&k, kBag, cut, &t) && feed(&k, kBag + cut, kLen - cut, &t));
    CHECK(same_but_index(t, whole));
    CHECK(k.w.phase == P_HLEN && k.w.have == 0 && !k.w.in_chunk && k.w.carry_len == 0);
  }
  for (size_t n = 0; n <= kLen; n += 3) {  // truncated bags, byte by byte behind them: a payload that grows a byte per call
    Totals t{};
    Walker k;
    CHECK(feed(&k, kBag, n, &t));
    for (size_t i = n; i < kLen; i++) CHECK(feed(&k, kBag + i, 1, &t));
    CHECK(same_but_index(t, whole));
  }
  // a failed call behind every cut: refused with state and carry as they were, and the right bytes behind it give the whole
  const uint8_t junk[4] = {0x01, 0x10, 0x00, 0x00};  // header_len 4097
  for (size_t cut = 0; cut <= kLen; cut += 7) {
    Totals t{}, u{};
    Walker k;
    CHECK(feed(&k, kBag, cut, &t));
    std::vector<uint8_t> bad(kBag + cut, kBag + kLen);
    bad.insert(bad.end(), junk, junk + 4);  // (behind the bag's last record: refused whatever else the chunk holds)
    CHECK(!feed(&k, bad.data(), bad.size(), &u));
    CHECK(feed(&k, kBag + cut, kLen - cut, &t));
    CHECK(same_but_index(t, whole));
  }
  // the bad streams and the edge values in L, Le, height, width, step and D: refused with the state as it was, or walked
  size_t at = 0;
  for (size_t e = 0; e < sizeof kEdgeLen / sizeof kEdgeLen[0]; at += kEdgeLen[e], e++) {
    Totals t{};
    Walker k;
    const bool ok = feed(&k, kEdge + at, kEdgeLen[e], &t);
    if (ok != (kEdgeOk[e] != 0)) fprintf(stderr, "edge stream %%zu: walked %%d\n", e, (int)ok), fails++;
    Totals u{};
    Walker d;
    bool ok1 = true;
    for (size_t i = 0; i < kEdgeLen[e] && ok1; i++) ok1 = feed(&d, kEdge + at + i, 1, &u);
    CHECK(ok1 == ok);
    if (ok) CHECK(same_but_index(t, u) && memcmp(&k.w, &d.w, offsetof(Walk, carry_buf)) == 0 && k.w.carry_len == d.w.carry_len);
  }
  // 10 000 seeded random byte strings, half of them behind a valid prefix, cut at a random place
  for (int it = 0; it < 10000; it++) {
    std::vector<uint8_t> s;
    if (it & 1) s.assign(kBag, kBag + rnd() %% (kLen + 1));
    const size_t n = rnd() %% 200;
    for (size_t i = 0; i < n; i++) s.push_back((uint8_t)((it & 2) && (rnd() & 3) ? 0 : rnd() >> 24));
    const size_t cut = s.empty() ? 0 : rnd() %% (s.size() + 1);
    Totals t{};
    Walker k;
    if (feed(&k, s.data(), cut, &t)) feed(&k, s.data() + cut, s.size() - cut, &t);
  }
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def edge_streams():
    """the bad streams of the reading, and per place and edge value a stream that holds the value there"""
    out = [data for data, _ in I.bad_streams().values()]
    conn = B.connection_record(0, I.LEFT_IMAGE, I.IMAGE_TYPE, I.IMAGE_MD5)
    head = lambda dl: conn + B.record([("conn", b"\0" * 4), ("time", b"\0" * 8), ("op", b"\x02")], b"")[:-4] + struct.pack("<I", dl & 0xFFFFFFFF)
    for v in EDGES:
        m = min(v, 4200)
        # L, with a data_len that is right for it where 32 bits can say so
        out.append(head(37 + v + 5 + 15) + (struct.pack("<IIII", 1, 1, 1, v) + b"f" * m + struct.pack("<III", 3, 5, 5) + b"mono8" +
                                                 struct.pack("<BII", 0, 5, 15) + bytes(15))[:4300])
        # Le
        out.append(head(37 + v + 15) + (B.ros_header(1, (1, 1), b"") + struct.pack("<III", 3, 5, v) + (b"mono8" + b"e" * 5000)[:m] +
                                            struct.pack("<BII", 0, 5, 15) + bytes(15))[:4300])
        # height and width, with step and D right for them where 32 bits can say so
        out.append(head(37 + 5 + 5 * v) + (B.ros_header(1, (1, 1), b"") + struct.pack("<III", v, 5, 5) + b"mono8" +
                                               struct.pack("<BII", 0, 5, (5 * v) & 0xFFFFFFFF) + bytes(min(5 * v, 4200))))
        out.append(head(37 + 5 + 3 * v) + (B.ros_header(1, (1, 1), b"") + struct.pack("<III", 3, v, 5) + b"mono8" +
                                               struct.pack("<BII", 0, v, (3 * v) & 0xFFFFFFFF) + bytes(min(3 * v, 4200))))
        # step, D right for it; and D alone
        out.append(head(37 + 5 + 3 * v) + (B.ros_header(1, (1, 1), b"") + struct.pack("<III", 3, 5, 5) + b"mono8" +
                                               struct.pack("<BII", 0, v, (3 * v) & 0xFFFFFFFF) + bytes(min(3 * v, 4200))))
        out.append(head(37 + 5 + v) + (B.ros_header(1, (1, 1), b"") + struct.pack("<III", 3, 5, 5) + b"mono8" + struct.pack("<BII", 0, 5, v) + bytes(m)))
    return out


def loop_walks(stream):
    try:
        I.ImageWalker(size=(5, 3)).feed(stream)
        return True
    except B.Malformed:
        return False


def test_the_edge_streams_cover_both_outcomes():
    ok = [loop_walks(s) for s in edge_streams()]
    assert 5 < sum(ok) < len(ok) - 20


def test_the_image_walk_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    edges = edge_streams()
    bag = I.small_bag()
    want = b"".join(I.decode(bag, size=(5, 3))["payloads"])
    src, exe = tmp_path / "bag_image_walk.cpp", tmp_path / "bag_image_walk"
    src.write_text(PROGRAM % {"bag": ", ".join(str(b) for b in bag[13:]), "want": ", ".join(str(b) for b in want),
                              "edge": ", ".join(str(b) for s in edges for b in s), "edge_len": ", ".join(str(len(s)) for s in edges),
                              "edge_ok": ", ".join(str(int(loop_walks(s))) for s in edges), "left": I.LEFT_IMAGE, "right": I.RIGHT_IMAGE,
                              "ev_left": B.LEFT, "ev_right": B.RIGHT, "imu": B.IMU})
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "esvio_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures"
