// The sequential decoder esvio_fe_decode_raw replaces: the rule of include/esvio_fe.h as one plain loop on one CPU
// core, words in, 16-byte event records out (what a host would then still have to upload).  The project's own.
//   g++ -O2 -std=c++17 tools/raw_seq_decode.cpp -o tools/_bin/raw_seq_decode
//   raw_seq_decode <3|2> <file of little-endian words> [t_offset_us] [repeats]
// prints one line: events, untimed, other, bad, wraps, and the median / min / max time of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Event {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity, pad[3];
};
struct State {
  uint32_t seen = 0, th = 0, tl = 0, y = 0, bx = 0, bp = 0;
  uint64_t wraps = 0;
};
struct Counts {
  uint64_t events = 0, untimed = 0, other = 0, bad = 0;
};

static inline void emit(std::vector<Event>& out, Counts& c, const State& s, uint32_t x, uint32_t y, uint32_t p, uint64_t t, int64_t off) {
  if (!s.seen) {
    c.untimed++;
    return;
  }
  const int64_t ticks = (int64_t)t + off;
  Event e{(uint16_t)x, (uint16_t)y, 0, 0, (uint8_t)p, {0, 0, 0}};
  if (ticks < 0 || ticks >= (int64_t)4294967296 * 1000000) {
    c.bad++;
  } else {
    e.sec = (uint32_t)(ticks / 1000000);
    e.nsec = (uint32_t)(ticks % 1000000) * 1000u;
  }
  out.push_back(e);
  c.events++;
}

static void decode_evt3(const uint16_t* w, size_t n, State& s, int64_t off, std::vector<Event>& out, Counts& c) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t v = w[i];
    const uint64_t t = (s.wraps << 24) + ((uint64_t)s.th << 12) + s.tl;
    switch (v >> 12) {
      case 0x0: s.y = v & 0x7ff; break;
      case 0x2: emit(out, c, s, v & 0x7ff, s.y, (v >> 11) & 1, t, off); break;
      case 0x3: s.bx = v & 0x7ff, s.bp = (v >> 11) & 1; break;
      case 0x4:
      case 0x5: {
        const uint32_t bits = (v >> 12) == 4 ? 12 : 8;
        for (uint32_t k = 0; k < bits; k++)
          if (v >> k & 1) emit(out, c, s, (s.bx + k) & 0xffff, s.y, s.bp, t, off);
        s.bx = (s.bx + bits) & 0xffff;
        break;
      }
      case 0x6: s.tl = v & 0xfff; break;
      case 0x8: {
        const uint32_t h = v & 0xfff;
        if (s.seen && h < s.th && s.th - h >= 2048) s.wraps++;
        s.th = h, s.seen = 1;
        break;
      }
      default: c.other++; break;
    }
  }
}

static void decode_evt2(const uint32_t* w, size_t n, State& s, int64_t off, std::vector<Event>& out, Counts& c) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t v = w[i], type = v >> 28;
    if (type <= 1) {
      emit(out, c, s, (v >> 11) & 0x7ff, v & 0x7ff, type, (s.wraps << 34) + ((uint64_t)s.th << 6) + ((v >> 22) & 0x3f), off);
    } else if (type == 8) {
      const uint32_t h = v & 0x0fffffff;
      if (s.seen && h < s.th && s.th - h >= (1u << 27)) s.wraps++;
      s.th = h, s.seen = 1;
    } else {
      c.other++;
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <3|2> <words file> [t_offset_us] [repeats]\n", argv[0]);
    return 2;
  }
  const int format = atoi(argv[1]);
  const int64_t off = argc > 3 ? atoll(argv[3]) : 0;
  const int repeats = argc > 4 ? atoi(argv[4]) : 5;
  FILE* f = fopen(argv[2], "rb");
  if (!f || (format != 2 && format != 3)) return 2;
  std::vector<uint8_t> bytes;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
  fclose(f);
  std::vector<double> us;
  Counts c;
  State s;
  std::vector<Event> out;
  for (int r = 0; r < repeats; r++) {
    c = Counts(), s = State();
    out.clear();  // (keeps its capacity: from the second repeat on no allocation is timed)
    const auto t0 = std::chrono::steady_clock::now();
    if (format == 3)
      decode_evt3((const uint16_t*)bytes.data(), bytes.size() / 2, s, off, out, c);
    else
      decode_evt2((const uint32_t*)bytes.data(), bytes.size() / 4, s, off, out, c);
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::vector<double> rest(us.begin() + (us.size() > 1 ? 1 : 0), us.end());
  std::sort(rest.begin(), rest.end());
  printf("events %llu untimed %llu other %llu bad %llu wraps %llu us_median %.1f us_min %.1f us_max %.1f\n", (unsigned long long)c.events,
         (unsigned long long)c.untimed, (unsigned long long)c.other, (unsigned long long)c.bad, (unsigned long long)s.wraps,
         rest[rest.size() / 2], rest.front(), rest.back());
  return 0;
}
