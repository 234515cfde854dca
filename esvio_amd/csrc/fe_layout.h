// fe_layout.h — where everything lies inside the blocks the LK kernels read and write in place: the result block
// (d_res on the device, h_pin pinned and device-visible) and the two speculative / chained blocks of h_spec.  The
// only place that computes an offset into them; no HIP here, so that a host-only test can check it alone
// (tests/test_layout.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace esvio {
namespace fe {

struct P2f {  // (float2's layout)
  float x, y;
};

// where one forward / backward LK pair puts its results
struct LkOut {
  P2f *fwd, *back;
  uint8_t *st_fwd, *st_back;
};

inline size_t layout_points(int max_cnt) { return max_cnt > 1 ? (size_t)max_cnt : 1; }  // M of every layout below
inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// Result block: set 1 = temporal LK, then stereo LK of the temporal survivors (twice: a frame works in one copy
// while the previous frame's stereo LK may still write the other), each copy with the LK's input points A behind it;
// 16 counters; news = [kept points (as uploaded) | newly selected corners]; set 2 = stereo LK of the new corners.
struct ResLayout {
  size_t B1[2], C1[2], SA1[2], SB1[2], A[2], CNT, NEW, B2, C2, SA2, SB2, total;
  size_t mask;  // total rounded up to 256: h_pin's upload area for a selection mask (d_res ends at total)
};
inline ResLayout res_layout(int max_cnt) {
  const size_t M = layout_points(max_cnt), stM = round_up(M, 64);
  ResLayout L;
  size_t o = 0;
  for (int s = 0; s < 2; s++) {
    L.B1[s] = o;  o += M * 8;
    L.C1[s] = o;  o += M * 8;
    L.SA1[s] = o; o += stM;
    L.SB1[s] = o; o += stM;
    L.A[s] = o;   o += M * 8;
  }
  L.CNT = o; o += 64;
  L.NEW = o; o += M * 8;
  L.B2 = o;  o += M * 8;
  L.C2 = o;  o += M * 8;
  L.SA2 = o; o += stM;
  L.SB2 = o; o += stM;
  L.total = o;
  L.mask = round_up(o, 256);
  return L;
}
// h_pin: the result block + a mask of height x ceil(width / 32) words
inline size_t pin_bytes(int max_cnt, int width, int height) {
  return res_layout(max_cnt).mask + (size_t)height * ((width + 31) / 32) * 4 + 256;
}

// One block of h_spec (there are two: 0 the speculative temporal launch's, 1 the chained launch's):
// [ptsB | ptsC | stA | stB | the launch's "a device-side wait expired" flag], padded to 256.
struct SpecLayout {
  size_t B, C, SA, SB, expired, bytes;
};
inline SpecLayout spec_layout(int max_cnt) {
  const size_t M = layout_points(max_cnt), stM = round_up(M, 64);
  SpecLayout L;
  L.B = 0;
  L.C = M * 8;
  L.SA = M * 16;
  L.SB = L.SA + stM;
  L.expired = L.SB + stM;
  L.bytes = round_up(L.expired + 64, 256);
  return L;
}
constexpr int kSpecBlocks = 2;

// The views: the same builder on a block's host, device-visible or device base address.
struct ResView {
  LkOut s1;         // set 1, the copy asked for ...
  P2f* A;           // ... and its LK input points
  LkOut s2;         // set 2
  P2f* news;
  int* counts;      // [16]: [0] n_out (select), [1] n_total (kept + new: the LK kernels' n_ptr), [3] a spin expired
  uint32_t* mask;   // h_pin only
};
inline ResView res_view(uint8_t* b, int max_cnt, int set) {
  const ResLayout L = res_layout(max_cnt);
  ResView v;
  v.s1 = LkOut{(P2f*)(b + L.B1[set]), (P2f*)(b + L.C1[set]), b + L.SA1[set], b + L.SB1[set]};
  v.A = (P2f*)(b + L.A[set]);
  v.s2 = LkOut{(P2f*)(b + L.B2), (P2f*)(b + L.C2), b + L.SA2, b + L.SB2};
  v.news = (P2f*)(b + L.NEW);
  v.counts = (int*)(b + L.CNT);
  v.mask = (uint32_t*)(b + L.mask);
  return v;
}

struct SpecView {
  LkOut out;
  int* expired;
};
inline SpecView spec_view(uint8_t* b, int max_cnt, int block) {
  const SpecLayout L = spec_layout(max_cnt);
  b += (size_t)block * L.bytes;
  return SpecView{LkOut{(P2f*)(b + L.B), (P2f*)(b + L.C), b + L.SA, b + L.SB}, (int*)(b + L.expired)};
}

}  // namespace fe
}  // namespace esvio
