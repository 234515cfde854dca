// The bridge esvio_fe_decode_aedat replaces: a libcaer / AEDAT 3.1 packet stream walked and decoded by one plain loop on
// one CPU core — the drivers' loop (davis_ros_driver/src/driver.cpp:664-694) over the rule of include/esvio_fe.h —, bytes
// in, 16-byte event records out (what a host would then still have to upload).  The project's own.
//   g++ -O2 -std=c++17 tools/aedat_seq_decode.cpp -o tools/_bin/aedat_seq_decode
//   aedat_seq_decode <file of packets> [t_offset_ns] [repeats] [keep_invalid]
// prints one line: events, invalid, bad, the packets, and the median / min / max time of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Event {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity, pad[3];
};
struct Counts {
  uint64_t events = 0, invalid = 0, bad = 0, polarity_packets = 0, other_packets = 0, malformed = 0;
};

static inline int32_t i32(const uint8_t* p) {
  int32_t v;
  memcpy(&v, p, 4);
  return v;
}

static void decode(const uint8_t* b, size_t n, int64_t off, bool keep, std::vector<Event>& out, Counts& c) {
  size_t pos = 0;
  while (pos + 28 <= n) {
    int16_t type;
    memcpy(&type, b + pos, 2);
    const int32_t size = i32(b + pos + 4), ts_off = i32(b + pos + 8), overflow = i32(b + pos + 12), capacity = i32(b + pos + 16),
                  number = i32(b + pos + 20);
    const bool known = type == 0 || type == 1 || type == 3;
    if (size <= 0 || capacity < 0 || number < 0 || number > capacity || (known && (size != (type == 3 ? 36 : 8) || ts_off != 4))) {
      c.malformed++;
      return;
    }
    pos += 28;
    if (type == 1) {
      c.polarity_packets++;
      const uint8_t* p = b + pos;
      for (int32_t j = 0; j < number && pos + 8 * (size_t)(j + 1) <= n; j++, p += 8) {
        const uint32_t data = (uint32_t)i32(p);
        const int32_t ts = i32(p + 4);
        if (!(data & 1u) && !keep) {
          c.invalid++;
          continue;
        }
        Event e{(uint16_t)((data >> 17) & 0x7fff), (uint16_t)((data >> 2) & 0x7fff), 0, 0, (uint8_t)((data >> 1) & 1), {0, 0, 0}};
        const __int128 ticks = (((__int128)overflow << 31) | (uint32_t)ts) * 1000 + off;
        if (ts < 0 || overflow < 0 || ticks < 0 || ticks >= (__int128)4294967296 * 1000000000) {
          c.bad++;
        } else {
          e.sec = (uint32_t)((uint64_t)ticks / 1000000000u);
          e.nsec = (uint32_t)((uint64_t)ticks % 1000000000u);
        }
        out.push_back(e);
        c.events++;
      }
    } else if (!known) {
      c.other_packets++;
    }
    const uint64_t payload = (uint64_t)capacity * (uint64_t)size;
    if (payload > n - pos) break;
    pos += (size_t)payload;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <packet file> [t_offset_ns] [repeats] [keep_invalid]\n", argv[0]);
    return 2;
  }
  const int64_t off = argc > 2 ? atoll(argv[2]) : 0;
  const int repeats = argc > 3 ? atoi(argv[3]) : 5;
  const bool keep = argc > 4 && atoi(argv[4]) != 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> bytes;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
  fclose(f);
  std::vector<double> us;
  Counts c;
  std::vector<Event> out;
  for (int r = 0; r < repeats; r++) {
    c = Counts();
    out.clear();  // (keeps its capacity: from the second repeat on no allocation is timed)
    const auto t0 = std::chrono::steady_clock::now();
    decode(bytes.data(), bytes.size(), off, keep, out, c);
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::vector<double> rest(us.begin() + (us.size() > 1 ? 1 : 0), us.end());
  std::sort(rest.begin(), rest.end());
  printf("events %llu invalid %llu bad %llu polarity_packets %llu other_packets %llu malformed %llu us_median %.1f us_min %.1f us_max %.1f\n",
         (unsigned long long)c.events, (unsigned long long)c.invalid, (unsigned long long)c.bad, (unsigned long long)c.polarity_packets,
         (unsigned long long)c.other_packets, (unsigned long long)c.malformed, rest[rest.size() / 2], rest.front(), rest.back());
  return 0;
}
