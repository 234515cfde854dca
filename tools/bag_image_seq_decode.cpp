// The bridge esvio_fe_decode_bag_images replaces: a rosbag v2.0 record stream walked by the project's own host walk in its
// image mode (esvio_amd/csrc/fe_bag.h) and every sensor_msgs/Image message converted pixel by pixel on one CPU core —
// getImageFromMsg's loop: the rows de-pitched, the colour classes turned to gray — into dense width x height images per
// camera (what a host would then still have to upload).
//   g++ -O2 -std=c++17 -Iesvio_amd/csrc tools/bag_image_seq_decode.cpp -o tools/_bin/bag_image_seq_decode
//   bag_image_seq_decode <file: a bag behind its 13-byte magic> <left topic> <right topic> [repeats] [out file]
// prints one line: the images per camera and the median / min / max time of the repeats in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_bag.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s <bag bytes behind the magic> <left topic> <right topic> [repeats] [out file]\n", argv[0]);
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
  bg::Topics topics;
  const char* why = nullptr;
  if (!bg::set_image_topics(argv[2], argv[3], &topics, &why)) return 2;
  std::vector<double> us;
  std::vector<uint8_t> pix, gray[2];
  std::vector<esvio_fe_bag_image> table;
  uint64_t n[2] = {0, 0};
  for (int r = 0; r < repeats; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    bg::Walk w{};
    bg::Carry carry;
    bg::Out cnt;
    if (!bg::walk(&w, topics, bg::kImages, bytes.data(), bytes.size(), &cnt)) {
      fprintf(stderr, "malformed: %s\n", cnt.why);
      return 1;
    }
    bg::Out o;
    pix.resize(cnt.n_pix_bytes);  // (keeps its capacity: from the second repeat on no allocation is timed)
    table.resize(cnt.n_imgs);
    o.carry = &carry, o.pix = pix.data(), o.pix_cap = pix.size(), o.imgs = table.data(), o.imgs_cap = table.size();
    w = bg::Walk{};
    bg::walk(&w, topics, bg::kImages, bytes.data(), bytes.size(), &o);
    size_t at = 0, used[2] = {0, 0};
    for (const esvio_fe_bag_image& m : table) {
      const size_t wh = (size_t)m.width * m.height;
      std::vector<uint8_t>& g = gray[m.cam];
      if (g.size() < used[m.cam] + wh) g.resize(used[m.cam] + wh);
      uint8_t* d = g.data() + used[m.cam];
      for (uint32_t y = 0; y < m.height; y++) {
        const uint8_t* s = pix.data() + at + (size_t)y * m.step;
        if (m.encoding == bg::kEncMono) {
          for (uint32_t x = 0; x < m.width; x++) d[(size_t)y * m.width + x] = s[x];
        } else {
          const int ri = m.encoding == bg::kEncBgr ? 2 : 0;
          for (uint32_t x = 0; x < m.width; x++, s += 3)
            d[(size_t)y * m.width + x] = (uint8_t)((s[ri] * 9798u + s[1] * 19235u + s[2 - ri] * 3735u + (1u << 14)) >> 15);
        }
      }
      used[m.cam] += wh;
      at += ((size_t)m.step * m.height + 15) & ~(size_t)15;
    }
    n[0] = cnt.n_cam_imgs[0], n[1] = cnt.n_cam_imgs[1];
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
  std::vector<double> rest(us.begin() + (us.size() > 1 ? 1 : 0), us.end());
  std::sort(rest.begin(), rest.end());
  printf("left %llu right %llu us_median %.1f us_min %.1f us_max %.1f\n", (unsigned long long)n[0], (unsigned long long)n[1], rest[rest.size() / 2],
         rest.front(), rest.back());
  if (argc > 5) {  // the gray images, left then right, for a caller that wants to compare them
    FILE* g = fopen(argv[5], "wb");
    if (!g) return 2;
    for (int cam = 0; cam < 2; cam++) fwrite(gray[cam].data(), 1, (size_t)n[cam] * (table.empty() ? 0 : (size_t)table[0].width * table[0].height), g);
    fclose(g);
  }
  return 0;
}
