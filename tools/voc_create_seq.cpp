// voc_create_seq — rule C of include/esvio_fe.h ("creating a vocabulary") as scalar loops on one core: the figure
// tools/voc_create_microbench.py times beside esvio_fe_bow_create_vocabulary, and a second reading of the rule whose
// file image the microbenchmark compares with the library's byte for byte.  The project's own text; no device code.
//
//   voc_create_seq DESC.u32 N DOCS.i64 N_DOCS K L WEIGHTING SEED OUT.bin   ->  one line: ms nodes words passes
//
// DESC.u32: N x 8 little-endian uint32; DOCS.i64: N_DOCS + 1 int64 offsets.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
struct Desc {
  uint64_t w[4];
};
struct Node {
  int parent;
  Desc d;
  std::vector<int> children;
  double weight;
};

int K, L, g_passes = 0;
std::vector<Node> nodes;

inline int dist(const Desc& a, const Desc& b) {
  return __builtin_popcountll(a.w[0] ^ b.w[0]) + __builtin_popcountll(a.w[1] ^ b.w[1]) + __builtin_popcountll(a.w[2] ^ b.w[2]) +
         __builtin_popcountll(a.w[3] ^ b.w[3]);
}
uint64_t mix(uint64_t z) {  // C5
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t draw(uint64_t key, uint32_t j) { return (uint32_t)(mix(key ^ ((uint64_t)(j + 1) << 32)) >> 33); }

// C3 for every cluster of a node in one sweep over its features
void means(const std::vector<const Desc*>& f, const std::vector<int>& assign, std::vector<Desc>& centres) {
  std::vector<int> cnt(centres.size() * 257, 0);
  for (size_t i = 0; i < f.size(); i++) {
    int* c = &cnt[(size_t)assign[i] * 257];
    c[256]++;
    for (int q = 0; q < 4; q++)
      for (uint64_t v = f[i]->w[q]; v; v &= v - 1) c[q * 64 + __builtin_ctzll(v)]++;
  }
  for (size_t k = 0; k < centres.size(); k++) {
    const int* c = &cnt[k * 257];
    Desc out = {{0, 0, 0, 0}};
    for (int b = 0; b < 256; b++)
      if (c[b] > c[256] / 2) out.w[b >> 6] |= 1ull << (b & 63);
    centres[k] = out;
  }
}

void step(int id, const std::vector<const Desc*>& f, int level, uint64_t key) {  // C1
  const int m = (int)f.size();
  std::vector<Desc> centres;
  std::vector<int> assign(m);
  if (m <= K) {
    for (int i = 0; i < m; i++) centres.push_back(*f[i]), assign[i] = i;
  } else {
    uint32_t j = 0;  // C2
    centres.push_back(*f[(int)(((double)draw(key, j++) / 2147483648.0) * (double)m)]);
    std::vector<int> md(m);
    for (int i = 0; i < m; i++) md[i] = dist(*f[i], centres[0]);
    while ((int)centres.size() < K) {
      uint64_t sum = 0;
      for (int i = 0; i < m; i++) {
        if (md[i] > 0) {
          const int d = dist(*f[i], centres.back());
          if (d < md[i]) md[i] = d;
        }
        sum += (uint64_t)md[i];
      }
      if (!sum) break;
      double cut;
      do cut = ((double)draw(key, j++) / 2147483647.0) * (double)sum;
      while (cut == 0.0);
      int pick = m - 1;
      uint64_t run = 0;
      for (int i = 0; i < m; i++) {
        run += (uint64_t)md[i];
        if ((double)run >= cut) {
          pick = i;
          break;
        }
      }
      centres.push_back(*f[pick]);
    }
    std::vector<int> last;
    for (int pass = 1;; pass++) {
      if (pass > 1) means(f, last, centres);
      for (int i = 0; i < m; i++) {
        int best = 0, bd = dist(*f[i], centres[0]);
        for (size_t c = 1; c < centres.size(); c++) {
          const int d = dist(*f[i], centres[c]);
          if (d < bd) bd = d, best = (int)c;
        }
        assign[i] = best;
      }
      if (pass > 1 && assign == last) {
        if (pass > g_passes) g_passes = pass;
        break;
      }
      last = assign;
    }
  }
  std::vector<int> kids;
  for (const Desc& c : centres) {
    kids.push_back((int)nodes.size());
    nodes[id].children.push_back(kids.back());
    nodes.push_back(Node{id, c, {}, 0.0});
  }
  if (level >= L) return;
  for (size_t c = 0; c < centres.size(); c++) {
    std::vector<const Desc*> g;
    for (int i = 0; i < m; i++)
      if (assign[i] == (int)c) g.push_back(f[i]);
    if (g.size() > 1) step(kids[c], g, level + 1, mix(key ^ (uint64_t)(c + 1)));
  }
}

template <class T>
std::vector<T> read_all(const char* path, size_t count) {
  std::vector<T> v(count);
  FILE* fp = fopen(path, "rb");
  if (!fp || fread(v.data(), sizeof(T), count, fp) != count) {
    fprintf(stderr, "voc_create_seq: cannot read %zu items from %s\n", count, path);
    exit(2);
  }
  fclose(fp);
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: voc_create_seq DESC.u32 N DOCS.i64 N_DOCS K L WEIGHTING SEED OUT.bin\n");
    return 2;
  }
  const size_t n = strtoull(argv[2], nullptr, 10), n_docs = strtoull(argv[4], nullptr, 10);
  K = atoi(argv[5]), L = atoi(argv[6]);
  const int weighting = atoi(argv[7]);
  const uint64_t seed = strtoull(argv[8], nullptr, 10);
  const std::vector<Desc> desc = read_all<Desc>(argv[1], n);
  const std::vector<int64_t> docs = read_all<int64_t>(argv[3], n_docs + 1);
  const auto t0 = std::chrono::steady_clock::now();
  nodes.push_back(Node{-1, {{0, 0, 0, 0}}, {}, 0.0});
  std::vector<const Desc*> all(n);
  for (size_t i = 0; i < n; i++) all[i] = &desc[i];
  step(0, all, 1, mix(seed));
  std::vector<int> leaves, word_of(nodes.size(), -1);  // C4
  for (size_t i = 1; i < nodes.size(); i++)
    if (nodes[i].children.empty()) word_of[i] = (int)leaves.size(), leaves.push_back((int)i);
  if (weighting == 1 || weighting == 3) {
    for (int id : leaves) nodes[id].weight = 1.0;
  } else {
    std::vector<uint32_t> ni(leaves.size(), 0);
    std::vector<int64_t> seen(leaves.size(), -1);
    for (size_t d = 0; d < n_docs; d++)
      for (int64_t i = docs[d]; i < docs[d + 1]; i++) {
        int at = 0;
        while (!nodes[at].children.empty()) {
          int best = -1, bd = 1 << 30;
          for (int ch : nodes[at].children) {
            const int dd = dist(desc[i], nodes[ch].d);
            if (dd < bd) bd = dd, best = ch;
          }
          at = best;
        }
        const int w = word_of[at];
        if (seen[w] != (int64_t)d) seen[w] = (int64_t)d, ni[w]++;
      }
    for (size_t w = 0; w < leaves.size(); w++)
      if (ni[w]) nodes[leaves[w]].weight = log((double)n_docs / (double)ni[w]);
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FILE* out = fopen(argv[9], "wb");  // C6
  if (!out) return 2;
  const int32_t head[6] = {K, L, 0, weighting, (int32_t)nodes.size() - 1, (int32_t)leaves.size()};
  fwrite(head, 4, 6, out);
  for (size_t i = 1; i < nodes.size(); i++) {
    const int32_t ids[2] = {(int32_t)i, nodes[i].parent};
    fwrite(ids, 4, 2, out), fwrite(&nodes[i].weight, 8, 1, out), fwrite(nodes[i].d.w, 8, 4, out);
  }
  for (size_t w = 0; w < leaves.size(); w++) {
    const int32_t rec[2] = {leaves[w], (int32_t)w};
    fwrite(rec, 4, 2, out);
  }
  fclose(out);
  printf("%.3f %zu %zu %d\n", ms, nodes.size() - 1, leaves.size(), g_passes);
  return 0;
}
