"""CPU: the AEDAT host walk in its frame mode (esvio_amd/csrc/fe_aedat.h) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program with its own main: g++ -fsanitize=address,undefined, run directly,
exit 0.  Every chunk handed to the walk is a heap block of exactly its length and every output is sized exactly by a
counting walk, so a read or a write outside them is a report.  Nothing here is loaded into Python.  The streams are built
by tests/aedat_frame_ref.py's writer, and what the program expects of each — refused, or walked, and the bytes gathered —
is what the sequential reading says."""
import os
import shutil
import subprocess

import pytest

import aedat_frame_ref as F
import aedat_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = (0, 1, 35, 36, 37, 2 ** 31 - 1, -1, -2 ** 31)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fe_aedat.h"
using namespace esvio::aedat;
static const uint8_t kStream[] = {%(stream)s};
static const size_t kLen = sizeof kStream;
static const uint8_t kWant[] = {%(want)s};          // the pixel bytes the sequential reading gathers, one frame behind the other
static const uint8_t kEdge[] = {%(edge)s};          // the bad and the edge-value streams, one behind the other
static const uint32_t kEdgeLen[] = {%(edge_len)s};
static const int kEdgeOk[] = {%(edge_ok)s};         // what the sequential reading says: 1 walked, 0 refused
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %%d: %%s\n", __LINE__, #c); fails++; } } while (0)

struct Totals {
  uint64_t v[5];
  std::vector<uint8_t> pix;  // the frames' pixel bytes without their padding
  std::vector<esvio_fe_aedat_frame> rows;
};
struct Walker {
  Walk w{};
  Carry carry;
};
// one chunk, as a heap block of exactly n bytes; outputs sized exactly by a counting walk first, as the library's call does
static bool feed(Walker* k, const uint8_t* p, size_t n, Totals* t, uint32_t flags = 0, uint32_t want_w = 5, uint32_t want_h = 3) {
  uint8_t* blk = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(blk, p, n);
  Walk probe = k->w;
  const Walk before = k->w;
  const std::vector<uint8_t> waiting(k->carry.buf[before.carry_buf & 1u].begin(), k->carry.buf[before.carry_buf & 1u].begin() + (size_t)before.carry_len);
  Out cnt;
  cnt.want_w = want_w, cnt.want_h = want_h;
  bool ok = walk(&probe, kFrames, n ? blk : nullptr, n, 0, flags, &cnt);
  if (!ok) CHECK(cnt.why != nullptr);
  if (ok && cnt.bad) ok = false;  // a BAD stamp fails the call
  if (ok) {
    Out o;
    o.want_w = want_w, o.want_h = want_h, o.carry = &k->carry;
    std::vector<uint8_t> pix(cnt.n_pix_bytes);
    std::vector<esvio_fe_aedat_frame> rows(cnt.n_frames);
    o.pix = pix.data(), o.pix_cap = pix.size(), o.frames = rows.data(), o.frames_cap = rows.size();
    Walk st = k->w;
    CHECK(walk(&st, kFrames, n ? blk : nullptr, n, 0, flags, &o));
    CHECK(memcmp(&st, &probe, sizeof st) == 0);
    CHECK(o.n_frames == cnt.n_frames && o.n_pix_bytes == cnt.n_pix_bytes);
    // what waited at the call's start is where it was: a call that failed behind its gathering walk would go back to it
    CHECK(k->carry.buf[before.carry_buf & 1u].size() >= waiting.size() &&
          (waiting.empty() || memcmp(k->carry.buf[before.carry_buf & 1u].data(), waiting.data(), waiting.size()) == 0));
    k->w = st;
    const uint64_t add[5] = {o.n_frames, o.invalid, o.frame_packets, o.other_packets, o.polarity_packets + o.special_packets + o.imu_packets};
    for (int i = 0; i < 5; i++) t->v[i] += add[i];
    size_t at = 0;
    for (const esvio_fe_aedat_frame& m : rows) {
      const size_t d = (size_t)m.length_x * m.length_y * m.channels * 2;
      t->pix.insert(t->pix.end(), pix.begin() + at, pix.begin() + at + d);
      at += (d + 15) & ~(size_t)15;
    }
    CHECK(at == pix.size());
    t->rows.insert(t->rows.end(), rows.begin(), rows.end());
  } else {
    CHECK(memcmp(&k->w, &before, sizeof before) == 0);
  }
  free(blk);
  return ok;
}
static bool same_but_index(const Totals& a, const Totals& b) {
  if (memcmp(a.v, b.v, sizeof a.v) != 0 || a.pix != b.pix || a.rows.size() != b.rows.size()) return false;
  for (size_t k = 0; k < a.rows.size(); k++)  // (the index counts per call)
    if (memcmp(&a.rows[k], &b.rows[k], offsetof(esvio_fe_aedat_frame, index)) != 0) return false;
  return true;
}

static uint32_t rs = 4321u;
static uint32_t rnd() { return rs = rs * 1664525u + 1013904223u; }

int main() {
  Totals whole{};
  {
    Walker k;
    CHECK(feed(&k, kStream, kLen, &whole));
    CHECK(whole.v[0] == 4 && whole.v[1] == 1 && whole.v[2] == 3 && whole.v[3] == 1 && whole.v[4] == 4);
    CHECK(whole.pix.size() == sizeof kWant && memcmp(whole.pix.data(), kWant, sizeof kWant) == 0);
    CHECK(whole.rows[3].slot == 1 && whole.rows[3].channels == 3 && whole.rows[3].ts_overflow == 1 && whole.rows[1].roi == 5);
    Totals keep{};
    Walker k2;
    CHECK(feed(&k2, kStream, kLen, &keep, ESVIO_FE_AEDAT_KEEP_INVALID) && keep.v[0] == 5 && keep.v[1] == 0 && keep.rows[2].valid == 0);
  }
  for (size_t cut = 0; cut <= kLen; cut++) {  // the stream cut in two at every byte: the carry across the calls
    Totals t{};
    Walker k;
    CHECK(feed(&k, kStream, cut, &t) && feed(&k, kStream + cut, kLen - cut, &t));
    CHECK(same_but_index(t, whole));
    CHECK(k.w.payload_left == 0 && k.w.hdr_have == 0 && k.w.carry_len == 0 && k.w.ev_off == 0);
  }
  for (size_t n = 0; n <= kLen; n += 3) {  // truncated streams, byte by byte behind them: a frame that grows a byte per call
    Totals t{};
    Walker k;
    CHECK(feed(&k, kStream, n, &t));
    for (size_t i = n; i < kLen; i++) CHECK(feed(&k, kStream + i, 1, &t));
    CHECK(same_but_index(t, whole));
  }
  // a failed call behind every cut: refused with state and carry as they were, and the right bytes behind it give the whole
  uint8_t junk[28] = {2, 0, 1, 0, 35, 0, 0, 0, 12, 0, 0, 0};  // a type-2 header with eventSize 35
  for (size_t cut = 0; cut <= kLen; cut += 7) {
    Totals t{}, u{};
    Walker k;
    CHECK(feed(&k, kStream, cut, &t));
    std::vector<uint8_t> bad(kStream + cut, kStream + kLen);
    bad.insert(bad.end(), junk, junk + 28);  // (behind the stream's last packet: refused whatever else the chunk holds)
    CHECK(!feed(&k, bad.data(), bad.size(), &u));
    CHECK(feed(&k, kStream + cut, kLen - cut, &t));
    CHECK(same_but_index(t, whole));
  }
  // the bad streams and the edge values in eventSize, lengthX, lengthY and the channel bits: refused with the state as it
  // was, or walked; whole and byte by byte alike
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
  // 10 000 seeded random byte strings, half of them behind a valid prefix, cut at a random place; every other one with any
  // size taken, so that a random head's pixels are gathered
  for (int it = 0; it < 10000; it++) {
    std::vector<uint8_t> s;
    if (it & 1) s.assign(kStream, kStream + rnd() %% (kLen + 1));
    const size_t n = rnd() %% 200;
    for (size_t i = 0; i < n; i++) s.push_back((uint8_t)((it & 2) && (rnd() & 3) ? (rnd() & 1 ? 0 : 2) : rnd() >> 24));
    const size_t cut = s.empty() ? 0 : rnd() %% (s.size() + 1);
    const uint32_t flags = it & 4 ? ESVIO_FE_AEDAT_KEEP_INVALID : 0, ww = it & 8 ? 0 : 5;
    Totals t{};
    Walker k;
    if (feed(&k, s.data(), cut, &t, flags, ww, 3)) feed(&k, s.data() + cut, s.size() - cut, &t, flags, ww, 3);
  }
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def edge_streams():
    """the bad streams of the reading, and per place and edge value a stream that holds the value there"""
    out = [data for data, _, _ in F.bad_streams().values()]
    px = F.test_pixels(5, 3, 3, 21).tobytes()
    for v in EDGES:
        # eventSize, with one event's worth of bytes behind the header where that is not gigabytes
        out.append(A.HEADER.pack(F.FRAME, 1, v, 12, 0, 1, 1, 1) + F.frame_event(px[:30], 5, 3, 1)[:max(min(v, 200), 0)])
        # lengthX and lengthY
        for valid in (1, 0):  # (an event with valid == 0 is dropped and not examined further)
            out.append(F.frame_packet([F.frame_event(px, v, 3, 1, valid=valid)]))
            out.append(F.frame_packet([F.frame_event(px, 5, v, 1, valid=valid)]))
            out.append(F.frame_packet([F.frame_event(px, v, v, 3, valid=valid)]))
    for ch in range(8):  # the channel bits
        out.append(F.frame_packet([F.frame_event(px, 5, 3, ch)]))
        out.append(F.frame_packet([F.frame_event(px, 1, 1, ch, valid=0)]))
    return out


def reading_walks(stream):
    try:
        F.FrameWalker((5, 3)).feed(stream)
        return True
    except (F.Malformed, F.Bad):
        return False


def test_the_edge_streams_cover_both_outcomes():
    ok = [reading_walks(s) for s in edge_streams()]
    assert 3 < sum(ok) < len(ok) - 20


def test_the_frame_walk_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    edges = edge_streams()
    stream = F.small_stream()
    want = b"".join(F.decode(stream, size=(5, 3))["pixels"])
    src, exe = tmp_path / "aedat_frame_walk.cpp", tmp_path / "aedat_frame_walk"
    src.write_text(PROGRAM % {"stream": ", ".join(str(b) for b in stream), "want": ", ".join(str(b) for b in want),
                              "edge": ", ".join(str(b) for s in edges for b in s), "edge_len": ", ".join(str(len(s)) for s in edges),
                              "edge_ok": ", ".join(str(int(reading_walks(s))) for s in edges)})
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "esvio_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures"
