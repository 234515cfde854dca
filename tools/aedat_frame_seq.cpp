// The bridge esvio_fe_decode_aedat_frames replaces: an AEDAT 3.1 packet stream walked by the project's own host walk in its
// frame mode (esvio_amd/csrc/fe_aedat.h) and every frame event converted pixel by pixel on one CPU core — the driver's
// loop, davis_ros_driver/src/driver.cpp:807-814: one push_back(value >> 8) per 16-bit value, and for a colour frame
// getImageFromMsg's gray behind it — into dense width x height images (what a host would then still have to upload).
//   g++ -O2 -std=c++17 -Iesvio_amd/csrc tools/aedat_frame_seq.cpp -o tools/_bin/aedat_frame_seq
//   aedat_frame_seq <file: packets, no text header> [repeats] [out file]
// prints one line: the frames and the median / min / max time of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_aedat.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <packet bytes> [repeats] [out file]\n", argv[0]);
    return 2;
  }
  const int repeats = argc > 2 ? atoi(argv[2]) : 5;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> bytes;
  uint8_t buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
  fclose(f);
  namespace ae = esvio::aedat;
  std::vector<double> us;
  std::vector<uint8_t> pix, gray;
  std::vector<esvio_fe_aedat_frame> table;
  uint64_t n = 0;
  for (int r = 0; r < repeats; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    ae::Walk w{};
    ae::Carry carry;
    ae::Out cnt;
    if (!ae::walk(&w, ae::kFrames, bytes.data(), bytes.size(), 0, ESVIO_FE_AEDAT_KEEP_INVALID, &cnt) || cnt.bad) {
      fprintf(stderr, "malformed: %s\n", cnt.why ? cnt.why : "a BAD stamp");
      return 1;
    }
    ae::Out o;
    pix.resize(cnt.n_pix_bytes);  // (keeps its capacity: from the second repeat on no allocation is timed)
    table.resize(cnt.n_frames);
    o.carry = &carry, o.pix = pix.data(), o.pix_cap = pix.size(), o.frames = table.data(), o.frames_cap = table.size();
    w = ae::Walk{};
    ae::walk(&w, ae::kFrames, bytes.data(), bytes.size(), 0, ESVIO_FE_AEDAT_KEEP_INVALID, &o);
    size_t at = 0;
    gray.clear();  // (keeps its capacity)
    std::vector<uint8_t> data;  // the driver's msg.data: filled by push_back, as there
    for (const esvio_fe_aedat_frame& m : table) {
      const size_t wh = (size_t)m.length_x * m.length_y, vals = wh * m.channels;
      const uint8_t* s = pix.data() + at;
      data.clear();
      for (size_t i = 0; i < vals; i++) data.push_back((uint8_t)(((uint32_t)s[2 * i] | (uint32_t)s[2 * i + 1] << 8) >> 8));
      if (m.channels == 1) {
        gray.insert(gray.end(), data.begin(), data.end());
      } else {
        for (size_t p = 0; p < wh; p++)
          gray.push_back((uint8_t)((data[3 * p] * 9798u + data[3 * p + 1] * 19235u + data[3 * p + 2] * 3735u + (1u << 14)) >> 15));
      }
      at += (vals * 2 + 15) & ~(size_t)15;
    }
    n = cnt.n_frames;
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::vector<double> rest(us.begin() + (us.size() > 1 ? 1 : 0), us.end());
  std::sort(rest.begin(), rest.end());
  printf("frames %llu us_median %.1f us_min %.1f us_max %.1f\n", (unsigned long long)n, rest[rest.size() / 2], rest.front(), rest.back());
  if (argc > 3) {  // the gray images, one behind the other, for a caller that wants to compare them
    FILE* g = fopen(argv[3], "wb");
    if (!g) return 2;
    fwrite(gray.data(), 1, gray.size(), g);
    fclose(g);
  }
  return 0;
}
