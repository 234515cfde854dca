// The bridge esvio_fe_decode_bag replaces: a rosbag v2.0 record stream walked by the project's own host walk
// (esvio_amd/csrc/fe_bag.h) and deserialized event by event on one CPU core — 13 wire bytes in, a 16-byte event record
// out, the loop a ROS deserializer plus make_events runs — per camera (what a host would then still have to upload).
//   g++ -O2 -std=c++17 -Iesvio_amd/csrc tools/bag_seq_decode.cpp -o tools/_bin/bag_seq_decode
//   bag_seq_decode <file: a bag behind its 13-byte magic> <left topic> <right topic> [repeats]
// prints one line: the events per camera, bad, messages, and the median / min / max time of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_bag.h"

struct Event {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity, pad[3];
};

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <bag bytes behind the magic> <left topic> <right topic> [repeats]\n", argv[0]);
    return 2;
  }
  const int repeats = argc > 4 ? atoi(argv[4]) : 5;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> bytes;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
  fclose(f);
  namespace bg = esvio::bag;
  const esvio_fe_bag_topics names = {argv[2], argv[3], nullptr};
  bg::Topics topics;
  const char* why = nullptr;
  if (!bg::set_topics(&names, &topics, &why)) return 2;
  std::vector<double> us;
  std::vector<uint8_t> wire[2];
  std::vector<Event> out[2];
  uint64_t n[2] = {0, 0}, bad = 0, msgs = 0;
  for (int r = 0; r < repeats; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    bg::Walk w{};
    bg::Out cnt;
    if (!bg::walk(&w, topics, bg::kEvents, bytes.data(), bytes.size(), &cnt)) {
      fprintf(stderr, "malformed: %s\n", cnt.why);
      return 1;
    }
    bg::Out o;
    for (int cam = 0; cam < 2; cam++) {
      wire[cam].resize(cnt.n_events[cam] * 13);  // (keeps its capacity: from the second repeat on no allocation is timed)
      out[cam].resize(cnt.n_events[cam]);
      o.payload[cam] = wire[cam].data(), o.events_cap[cam] = cnt.n_events[cam];
    }
    w = bg::Walk{};
    bg::walk(&w, topics, bg::kEvents, bytes.data(), bytes.size(), &o);
    bad = 0;
    for (int cam = 0; cam < 2; cam++) {
      const uint8_t* p = wire[cam].data();
      Event* e = out[cam].data();
      for (uint64_t i = 0; i < cnt.n_events[cam]; i++, p += 13) {
        memset(&e[i], 0, sizeof(Event));
        memcpy(&e[i].x, p, 2), memcpy(&e[i].y, p + 2, 2), memcpy(&e[i].sec, p + 4, 4), memcpy(&e[i].nsec, p + 8, 4);
        e[i].polarity = p[12] ? 1 : 0;
        bad += e[i].nsec >= 1000000000u;
      }
      n[cam] = cnt.n_events[cam];
    }
    msgs = cnt.n_msgs;
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::vector<double> rest(us.begin() + (us.size() > 1 ? 1 : 0), us.end());
  std::sort(rest.begin(), rest.end());
  printf("left %llu right %llu bad %llu messages %llu us_median %.1f us_min %.1f us_max %.1f\n", (unsigned long long)n[0],
         (unsigned long long)n[1], (unsigned long long)bad, (unsigned long long)msgs, rest[rest.size() / 2], rest.front(), rest.back());
  if (argc > 5) {  // the records, left then right, for a caller that wants to compare them
    FILE* g = fopen(argv[5], "wb");
    if (!g) return 2;
    for (int cam = 0; cam < 2; cam++) fwrite(out[cam].data(), sizeof(Event), out[cam].size(), g);
    fclose(g);
  }
  return 0;
}
