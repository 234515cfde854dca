// The bridge esvio_fe_decode_text replaces, on one core: a text event file read line by line with a digit loop of
// strtoull's class (esvio_amd/csrc/fe_text.h: decode_chunk, the rule's sequential reading) into event records.  The
// upload of the records is measured beside it by tools/text_microbench.py (esvio_fe_mem_upload).
//   text_seq_decode <file> <order: 1 txyp, 2 xypt> <time: 1 sec_decimal, 2 int_us, 3 int_ns> [blocks]
// prints: events N lines N us_median T us_min T us_max T   (per pass over the file; `blocks` passes behind a warm-up one)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_text.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <file> <order> <time> [blocks]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> data;
  uint8_t buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  const esvio::text::Format fmt{atoi(argv[2]), atoi(argv[3]), esvio::text::kEnd};
  const int blocks = argc > 4 ? atoi(argv[4]) : 5;
  std::vector<esvio::text::Event> dst((data.size() + esvio::text::kMaxTail) / 8 + 1);
  std::vector<double> us;
  esvio::text::Counts c;
  for (int b = 0; b <= blocks; b++) {
    esvio::text::State st;
    const auto t0 = std::chrono::steady_clock::now();
    if (esvio::text::decode_chunk(&st, fmt, data.data(), data.size(), 0, dst.data(), dst.size(), &c) != 0) {
      fprintf(stderr, "the file does not read: %llu malformed, %llu BAD\n", (unsigned long long)c.malformed, (unsigned long long)c.bad);
      return 1;
    }
    const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (b) us.push_back(dt);
  }
  std::sort(us.begin(), us.end());
  printf("events %llu lines %llu us_median %.1f us_min %.1f us_max %.1f\n", (unsigned long long)c.events, (unsigned long long)c.lines,
         us[us.size() / 2], us.front(), us.back());
  return 0;
}
