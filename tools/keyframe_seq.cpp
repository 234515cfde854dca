// keyframe_seq.cpp — the keyframe rules of include/esvio_fe.h ("keyframes": B, F, D, M) as plain scalar loops on one
// core: the bridge esvio_fe_kf_describe / esvio_fe_kf_match replace for a host that has no OpenCV build at hand, and the
// figure tools/keyframe_microbench.py prints beside the library's.  (A scalar restatement: OpenCV's own blur and FAST
// are vectorised and faster than this; nobody has measured them here.)
//
//   keyframe_seq <input> : int32 {W, H, n_window, nq, nt, reps}, the image (W*H bytes), n_window (x, y) float pairs,
//   the pattern (x1 | y1 | x2 | y2, 256 int32 each), nq + nt descriptors of 8 words.
//   Prints: describe_us <per rep> n_kp <count> desc_xor <xor of all descriptor words> match_us <per rep> match_sum
//   <sum of idx + dist + status>.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
const int kTaps[9] = {7, 17, 32, 46, 52, 46, 32, 17, 7};
const int kDx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
const int kDy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

int reflect101(int p, int n) {
  if (p < 0) p = -p;
  return p >= n ? 2 * n - 2 - p : p;
}

void blur(const uint8_t* img, int W, int H, std::vector<uint16_t>& rows, uint8_t* out) {
  rows.resize((size_t)W * H);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      int s = 0;
      for (int i = 0; i < 9; i++) s += kTaps[i] * img[(size_t)y * W + reflect101(x + i - 4, W)];
      rows[(size_t)y * W + x] = (uint16_t)s;
    }
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      uint32_t s = 0;
      for (int j = 0; j < 9; j++) s += (uint32_t)kTaps[j] * rows[(size_t)reflect101(y + j - 4, H) * W + x];
      out[(size_t)y * W + x] = (uint8_t)((s + 32768u) >> 16);
    }
}

// score + 1 where the pixel is a corner at barrier t, else 0
void fast_map(const uint8_t* img, int W, int H, int t, std::vector<uint8_t>& m) {
  m.assign((size_t)W * H, 0);
  for (int y = 3; y < H - 3; y++)
    for (int x = 3; x < W - 3; x++) {
      const int c = img[(size_t)y * W + x];
      int d[16];
      uint32_t mb = 0, md = 0;
      for (int k = 0; k < 16; k++) {
        d[k] = (int)img[(size_t)(y + kDy[k]) * W + x + kDx[k]] - c;
        mb |= (uint32_t)(d[k] > t) << k;
        md |= (uint32_t)(d[k] < -t) << k;
      }
      if (!mb && !md) continue;
      int best = 0;
      for (int s = 0; s < 16; s++) {
        int lo = 256, hi = -256;
        for (int k = 0; k < 9; k++) {
          const int v = d[(s + k) & 15];
          lo = v < lo ? v : lo;
          hi = v > hi ? v : hi;
        }
        const int a = lo > -hi ? lo : -hi;  // the arc's min |difference| where all lie on one side
        best = a > best ? a : best;
      }
      if (best > t) m[(size_t)y * W + x] = (uint8_t)best;
    }
}

void fast_keep(const std::vector<uint8_t>& m, int W, int H, std::vector<float>& xy) {
  xy.clear();
  for (int y = 3; y < H - 3; y++)
    for (int x = 3; x < W - 3; x++) {
      const int v = m[(size_t)y * W + x];
      if (v < 2) continue;  // (no corner, or a score of 0)
      bool keep = true;
      for (int dy = -1; dy <= 1 && keep; dy++)
        for (int dx = -1; dx <= 1; dx++)
          if ((dx || dy) && m[(size_t)(y + dy) * W + x + dx] >= v) {
            keep = false;
            break;
          }
      if (keep) xy.push_back((float)x), xy.push_back((float)y);
    }
}

void brief(const uint8_t* b, int W, int H, const int32_t* pat, const float* pts, size_t n, uint32_t* desc) {
  for (size_t p = 0; p < n; p++) {
    uint32_t* d = desc + p * 8;
    memset(d, 0, 32);
    const float px = pts[2 * p], py = pts[2 * p + 1];
    if (!(std::fabs(px) < 32768.f) || !(std::fabs(py) < 32768.f)) continue;
    for (int i = 0; i < 256; i++) {
      const int x1 = (int)(px + (float)pat[i]), y1 = (int)(py + (float)pat[256 + i]);
      const int x2 = (int)(px + (float)pat[512 + i]), y2 = (int)(py + (float)pat[768 + i]);
      if (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H && x2 >= 0 && x2 < W && y2 >= 0 && y2 < H)
        if (b[(size_t)y1 * W + x1] < b[(size_t)y2 * W + x2]) d[i >> 5] |= 1u << (i & 31);
    }
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[6];
  if (fread(hd, 4, 6, f) != 6) return 2;
  const int W = hd[0], H = hd[1], nw = hd[2], nq = hd[3], nt = hd[4], reps = hd[5];
  std::vector<uint8_t> img((size_t)W * H);
  std::vector<float> win((size_t)nw * 2);
  std::vector<int32_t> pat(1024);
  std::vector<uint32_t> Q((size_t)nq * 8), T((size_t)nt * 8);
  if (fread(img.data(), 1, img.size(), f) != img.size() || fread(win.data(), 8, nw, f) != (size_t)nw || fread(pat.data(), 4, 1024, f) != 1024 ||
      fread(Q.data(), 32, nq, f) != (size_t)nq || fread(T.data(), 32, nt, f) != (size_t)nt)
    return 2;
  fclose(f);
  using clk = std::chrono::steady_clock;
  std::vector<uint16_t> rows;
  std::vector<uint8_t> blurred((size_t)W * H), m;
  std::vector<float> kp;
  std::vector<uint32_t> wd((size_t)nw * 8), kd;
  uint32_t x = 0;
  const auto t0 = clk::now();
  for (int r = 0; r < reps; r++) {
    blur(img.data(), W, H, rows, blurred.data());
    fast_map(img.data(), W, H, 20, m);
    fast_keep(m, W, H, kp);
    kd.resize(kp.size() * 4);
    brief(blurred.data(), W, H, pat.data(), win.data(), (size_t)nw, wd.data());
    brief(blurred.data(), W, H, pat.data(), kp.data(), kp.size() / 2, kd.data());
  }
  const double describe_us = std::chrono::duration<double, std::micro>(clk::now() - t0).count() / reps;
  for (uint32_t v : wd) x ^= v;
  for (uint32_t v : kd) x ^= v;
  long long sum = 0;
  const auto t1 = clk::now();
  for (int r = 0; r < reps; r++) {
    sum = 0;
    for (int q = 0; q < nq; q++) {
      int best = 128, idx = -1;
      for (int i = 0; i < nt; i++) {
        int d = 0;
        for (int k = 0; k < 8; k++) d += __builtin_popcount(Q[(size_t)q * 8 + k] ^ T[(size_t)i * 8 + k]);
        if (d < best) best = d, idx = i;
      }
      sum += idx + best + (idx != -1 && best < 80);
    }
  }
  const double match_us = std::chrono::duration<double, std::micro>(clk::now() - t1).count() / reps;
  printf("describe_us %.1f n_kp %zu desc_xor %08x match_us %.1f match_sum %lld\n", describe_us, kp.size() / 2, x, match_us, sum);
  return 0;
}
