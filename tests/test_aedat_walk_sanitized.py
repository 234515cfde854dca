"""CPU: the AEDAT host walk (esvio_amd/csrc/fe_aedat.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program with its own main: g++ -fsanitize=address,undefined, run directly, exit 0.  Every chunk handed to the
walk is a heap block of exactly its length, so a read outside the n bytes is a report.  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import aedat_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fe_aedat.h"
using namespace esvio::aedat;
static const uint8_t kStream[] = {%(stream)s};
static const size_t kLen = sizeof kStream;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %%d: %%s\n", __LINE__, #c); fails++; } } while (0)

struct Totals { uint64_t v[12]; std::vector<uint8_t> pay; };
// one chunk, as a heap block of exactly n bytes; outputs sized exactly by a counting walk first
static bool feed(Walk* w, Mode mode, const uint8_t* p, size_t n, uint32_t flags, Totals* t) {
  uint8_t* blk = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(blk, p, n);
  Walk probe = *w;
  Out cnt;
  const bool ok = walk(&probe, mode, n ? blk : nullptr, n, 1000000007, flags, &cnt);
  if (ok) {
    Out o;
    std::vector<uint8_t> pay(cnt.n_events * 8);
    std::vector<Run> runs(cnt.n_runs);
    std::vector<esvio_fe_imu_sample> imu(cnt.n_imu);
    std::vector<esvio_fe_trigger> trig(cnt.n_trig);
    o.payload = pay.data(), o.events_cap = cnt.n_events, o.runs = runs.data(), o.runs_cap = cnt.n_runs;
    o.imu = imu.data(), o.imu_cap = cnt.n_imu, o.trig = trig.data(), o.trig_cap = cnt.n_trig;
    Walk st = *w;
    CHECK(walk(&st, mode, n ? blk : nullptr, n, 1000000007, flags, &o));
    CHECK(memcmp(&st, &probe, sizeof st) == 0);
    CHECK(o.n_events == cnt.n_events && o.n_runs == cnt.n_runs && o.n_imu == cnt.n_imu && o.n_trig == cnt.n_trig);
    *w = st;
    const uint64_t add[12] = {o.n_events, o.polarity_packets, o.other_packets, o.n_imu, o.n_trig, o.resets, o.other_specials,
                              o.invalid, o.bad, o.special_packets, o.imu_packets, 0};
    for (int k = 0; k < 12; k++) t->v[k] += add[k];
    for (size_t i = 0; i < runs.size(); i++) CHECK(runs[i].first < cnt.n_events && (i == 0 ? runs[i].first == 0 : runs[i].first > runs[i - 1].first));
    t->pay.insert(t->pay.end(), pay.begin(), pay.end());
  }
  free(blk);
  return ok;
}

static uint32_t rs = 12345u;
static uint32_t rnd() { return rs = rs * 1664525u + 1013904223u; }
static void put32(uint8_t* p, int32_t v) { for (int k = 0; k < 4; k++) p[k] = (uint8_t)((uint32_t)v >> (8 * k)); }

int main() {
  for (int mode = 0; mode < 2; mode++)
    for (uint32_t flags = 0; flags < 2; flags++) {
      Totals whole{};
      Walk w{};
      CHECK(feed(&w, (Mode)mode, kStream, kLen, flags, &whole));
      if (mode == kEvents) CHECK(whole.v[0] == 12 && whole.v[1] == 3 && whole.v[2] == 1);
      if (mode == kSide) CHECK(whole.v[3] == 1 && whole.v[4] == 1 && whole.v[5] == 1 && whole.v[8] == 0);
      for (size_t cut = 0; cut <= kLen; cut++) {  // the stream cut in two at every byte
        Totals t{};
        Walk c{};
        CHECK(feed(&c, (Mode)mode, kStream, cut, flags, &t) && feed(&c, (Mode)mode, kStream + cut, kLen - cut, flags, &t));
        CHECK(memcmp(t.v, whole.v, sizeof t.v) == 0 && t.pay == whole.pay);
        CHECK(c.payload_left == 0 && c.hdr_have == 0 && c.rec_have == 0);
      }
      for (size_t n = 0; n <= kLen; n++) {  // truncated streams, byte by byte behind them
        Totals t{};
        Walk c{};
        CHECK(feed(&c, (Mode)mode, kStream, n, flags, &t));
        for (size_t i = n; i < kLen; i++) CHECK(feed(&c, (Mode)mode, kStream + i, 1, flags, &t));
        CHECK(memcmp(t.v, whole.v, sizeof t.v) == 0 && t.pay == whole.pay);
      }
    }
  // headers with INT32_MAX / negative fields: refused, or walked without reading what is not there
  const int32_t edge[] = {0, 1, -1, 8, 36, INT32_MAX, INT32_MIN, 4};
  for (int type = -1; type <= 4; type++)
    for (int32_t size : edge)
      for (int32_t cap : edge)
        for (int32_t num : edge)
          for (int32_t tso : {4, 0, INT32_MIN}) {
            uint8_t h[28 + 40] = {0};
            h[0] = (uint8_t)type, h[1] = (uint8_t)(type < 0 ? 0xff : 0);
            put32(h + 4, size), put32(h + 8, tso), put32(h + 12, INT32_MAX), put32(h + 16, cap), put32(h + 20, num);
            for (int k = 28; k < 68; k++) h[k] = (uint8_t)rnd();
            const bool known = type == 0 || type == 1 || type == 3;
            const bool malformed = size <= 0 || cap < 0 || num < 0 || num > cap || (known && (size != (type == 3 ? 36 : 8) || tso != 4));
            for (int mode = 0; mode < 2; mode++) {
              Totals t{};
              Walk c{}, before{};
              // (the payload bytes this packet owns and no more: what follows them would be read as the next header)
              const uint64_t own = malformed ? 40 : (uint64_t)cap * (uint64_t)size;
              const bool ok = feed(&c, (Mode)mode, h, 28 + (size_t)(own < 40 ? own : 40), 0, &t);
              CHECK(ok == !malformed);
              if (!ok) CHECK(memcmp(&c, &before, sizeof c) == 0);
            }
          }
  // 10 000 seeded random byte strings, some of them behind a valid prefix, cut at a random place
  for (int it = 0; it < 10000; it++) {
    std::vector<uint8_t> s;
    if (it & 1) s.assign(kStream, kStream + rnd() %% (kLen + 1));
    const size_t n = rnd() %% 200;
    for (size_t i = 0; i < n; i++) s.push_back((uint8_t)((it & 2) && (rnd() & 3) ? 0 : rnd() >> 24));
    const size_t cut = s.empty() ? 0 : rnd() %% (s.size() + 1);
    for (int mode = 0; mode < 2; mode++) {
      Totals t{};
      Walk c{};
      if (feed(&c, (Mode)mode, s.data(), cut, it & 4 ? 1u : 0u, &t)) feed(&c, (Mode)mode, s.data() + cut, s.size() - cut, it & 4 ? 1u : 0u, &t);
    }
    esvio_fe_aedat_header_info hi;
    uint8_t* blk = (uint8_t*)malloc(s.size() ? s.size() : 1);
    if (!s.empty()) memcpy(blk, s.data(), s.size());
    if (it & 8) blk[0] = '#';
    CHECK(file_header(blk, s.size(), &hi) == 0 && hi.payload_offset <= s.size());
    free(blk);
  }
  printf("%%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_the_walk_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "aedat_walk.cpp", tmp_path / "aedat_walk"
    src.write_text(PROGRAM % {"stream": ", ".join(str(b) for b in A.small_stream())})
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "esvio_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures"
