// The sequential loop esvio_fe_slice_events replaces: the rule of include/esvio_fe.h as one plain loop on one CPU core over
// 16-byte event records in host memory (what a host holds after a download) — the boundary chain computed as it goes,
// one comparison per event in the common case, a fresh camera whose origin is the first record.  The project's own.
//   g++ -O2 -std=c++17 -ffp-contract=off tools/slice_seq_cut.cpp -o tools/_bin/slice_seq_cut
//   slice_seq_cut <file of records> <frequency> [repeats]
// prints one line: events, windows closed, the sum of the cut entries (a check value), and the median / min / max time
// of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Event {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity, pad[3];
};
static inline double to_sec(uint64_t sec, uint32_t nsec) { return (double)sec + 1e-9 * (double)nsec; }
static inline double next_boundary(double from, double period) {  // toSec(Time(from + period)), ros::Time::fromSec restated
  const double d = from + period, fl = std::floor(d);
  uint64_t sec = (uint64_t)fl, nsec = (uint64_t)std::round((d - fl) * 1e9);
  if (nsec >= 1000000000ull) sec += 1, nsec -= 1000000000ull;
  return to_sec(sec, (uint32_t)nsec);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<Event> ev;
  Event buf[4096];
  for (size_t k; (k = fread(buf, sizeof(Event), 4096, f)) > 0;) ev.insert(ev.end(), buf, buf + k);
  fclose(f);
  const double period = 1.0 / atof(argv[2]);
  const int reps = argc > 3 ? atoi(argv[3]) : 5;
  std::vector<uint64_t> cuts;
  std::vector<double> us;
  for (int r = 0; r < reps; r++) {
    cuts.clear();
    const auto t0 = std::chrono::steady_clock::now();
    if (!ev.empty()) {
      double end = next_boundary(to_sec(ev[0].sec, ev[0].nsec), period);  // toSec(E_m) of the open window
      for (size_t i = 0; i < ev.size(); i++) {
        const double ts = to_sec(ev[i].sec, ev[i].nsec);
        while (end <= ts) {  // the event lies at or behind the boundary: the window closes (a gap: each window in turn)
          cuts.push_back(i);
          end = next_boundary(end, period);
        }
      }
    }
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::sort(us.begin(), us.end());
  uint64_t sum = 0;
  for (uint64_t c : cuts) sum += c;
  printf("%zu %zu %llu %.1f %.1f %.1f\n", ev.size(), cuts.size(), (unsigned long long)sum, us[us.size() / 2], us.front(), us.back());
  return 0;
}
