// tests/test_layout.py: fe_layout.h alone, with the host compiler.  For each max_cnt on the command line every
// region of the result block (both copies of set 1) and of the two speculative blocks must lie inside its block,
// overlap no other region, be aligned for what it holds, and the block sizes must be the ones esvio_fe_create
// allocates.  Prints "layout ok: <n> sizes" or one line per violation (exit 1).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_layout.h"

using namespace esvio::fe;

struct Region {
  const char* name;
  size_t off, len, align;
};
static int bad = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      bad++;                                   \
      printf("max_cnt %d: ", max_cnt);         \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

static void check_regions(int max_cnt, const char* block, const std::vector<Region>& r, size_t block_bytes) {
  for (size_t i = 0; i < r.size(); i++) {
    CHECK(r[i].off + r[i].len <= block_bytes, "%s.%s [%zu, +%zu) leaves the block of %zu", block, r[i].name, r[i].off,
          r[i].len, block_bytes);
    CHECK(r[i].off % r[i].align == 0, "%s.%s at %zu is not %zu-byte aligned", block, r[i].name, r[i].off, r[i].align);
    for (size_t j = i + 1; j < r.size(); j++)
      CHECK(r[i].off + r[i].len <= r[j].off || r[j].off + r[j].len <= r[i].off, "%s.%s and %s.%s overlap", block,
            r[i].name, block, r[j].name);
  }
}

static void lk_out(std::vector<Region>& r, const uint8_t* base, const LkOut& o, size_t n, const char* const names[4]) {
  r.push_back({names[0], (size_t)((const uint8_t*)o.fwd - base), n * 8, 8});
  r.push_back({names[1], (size_t)((const uint8_t*)o.back - base), n * 8, 8});
  r.push_back({names[2], (size_t)(o.st_fwd - base), n, 1});
  r.push_back({names[3], (size_t)(o.st_back - base), n, 1});
}

int main(int argc, char** argv) {
  const int W = 346, H = 260;
  for (int a = 1; a < argc; a++) {
    const int max_cnt = atoi(argv[a]);
    const size_t n = max_cnt > 1 ? (size_t)max_cnt : 1;  // points a launch may write
    // the views are built on a base that is not null, so that a wrong offset cannot hide in pointer arithmetic on 0
    alignas(256) static uint8_t origin[256];
    uint8_t* base = origin;
    {
      const ResLayout L = res_layout(max_cnt);
      const size_t mask_bytes = (size_t)H * ((W + 31) / 32) * 4;
      const size_t bytes = pin_bytes(max_cnt, W, H);  // h_pin; d_res is L.total
      const ResView v[2] = {res_view(base, max_cnt, 0), res_view(base, max_cnt, 1)};
      std::vector<Region> r;
      static const char* const n1[2][4] = {{"ptsB[0]", "ptsC[0]", "stA[0]", "stB[0]"}, {"ptsB[1]", "ptsC[1]", "stA[1]", "stB[1]"}};
      static const char* const n2[4] = {"ptsB2", "ptsC2", "stA2", "stB2"};
      for (int s = 0; s < 2; s++) {
        lk_out(r, base, v[s].s1, n, n1[s]);
        r.push_back({s ? "A[1]" : "A[0]", (size_t)((uint8_t*)v[s].A - base), n * 8, 8});
        CHECK(v[s].news == v[0].news && v[s].counts == v[0].counts && v[s].mask == v[0].mask && v[s].s2.fwd == v[0].s2.fwd &&
                  v[s].s2.back == v[0].s2.back && v[s].s2.st_fwd == v[0].s2.st_fwd && v[s].s2.st_back == v[0].s2.st_back,
              "copy %d of set 1 moves what the copies share", s);
      }
      lk_out(r, base, v[0].s2, n, n2);
      r.push_back({"news", (size_t)((uint8_t*)v[0].news - base), n * 8, 8});
      r.push_back({"counts", (size_t)((uint8_t*)v[0].counts - base), 64, 4});
      check_regions(max_cnt, "d_res", r, L.total);  // (everything but the mask: the device block ends here)
      r.push_back({"mask", (size_t)((uint8_t*)v[0].mask - base), mask_bytes, 4});
      check_regions(max_cnt, "h_pin", r, bytes);
      CHECK(L.mask >= L.total && L.mask % 256 == 0 && (size_t)((uint8_t*)v[0].mask - base) == L.mask,
            "mask area at %zu, layout ends at %zu", L.mask, L.total);
      CHECK(bytes == L.mask + mask_bytes + 256, "pin_bytes %zu", bytes);
    }
    {
      const SpecLayout L = spec_layout(max_cnt);
      CHECK(L.bytes % 256 == 0, "speculative block of %zu bytes", L.bytes);
      std::vector<Region> all;
      static const char* const nb[2][5] = {{"spec.ptsB", "spec.ptsC", "spec.stA", "spec.stB", "spec.expired"},
                                           {"chain.ptsB", "chain.ptsC", "chain.stA", "chain.stB", "chain.expired"}};
      for (int b = 0; b < kSpecBlocks; b++) {
        const SpecView v = spec_view(base, max_cnt, b);
        std::vector<Region> r;
        lk_out(r, base + b * L.bytes, v.out, n, nb[b]);
        r.push_back({nb[b][4], (size_t)((uint8_t*)v.expired - (base + b * L.bytes)), 4, 4});
        check_regions(max_cnt, b ? "h_spec[1]" : "h_spec[0]", r, L.bytes);  // each inside its own block
        for (Region& x : r) x.off += b * L.bytes;
        all.insert(all.end(), r.begin(), r.end());
      }
      check_regions(max_cnt, "h_spec", all, kSpecBlocks * L.bytes);  // ... and the two blocks apart: what create allocates
    }
  }
  if (!bad) printf("layout ok: %d sizes\n", argc - 1);
  return bad ? 1 : 0;
}
