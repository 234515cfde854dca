// bow_seq — the rules of include/esvio_fe.h "loop detection" as scalar loops on one core: the bridge
// tools/bow_microbench.py sets beside the device figures.  This repository's own restatement, NOT DBoW2's code (which
// needs OpenCV and boost and was not measured): a tree of child lists, std::map vectors, an inverted file.
//   bow_seq <file>   file: int32 {voc_bytes, n_desc, n_entries, reps}, the vocabulary file image, n_entries x n_desc
//                    descriptors (8 words each) for the database, n_desc descriptors for the query
//   prints: transform_us query_us words_xor result_ids
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
#include <algorithm>

struct Node {
  std::vector<int> children;
  double weight = 0;
  int word = -1;
  uint64_t d[4] = {0, 0, 0, 0};
};
typedef std::map<uint32_t, double> Vec;
static std::vector<Node> nodes;
static int weighting;

static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void transform(const uint32_t* desc, int n, Vec& v) {
  v.clear();
  for (int i = 0; i < n; i++) {
    uint64_t q[4];
    memcpy(q, desc + 8 * i, 32);
    int at = 0;
    while (!nodes[at].children.empty()) {
      int best = -1, best_d = 0;
      for (int c : nodes[at].children) {
        int d = 0;
        for (int j = 0; j < 4; j++) d += __builtin_popcountll(q[j] ^ nodes[c].d[j]);
        if (best < 0 || d < best_d) best = c, best_d = d;
      }
      at = best;
    }
    const double w = nodes[at].weight;
    if (!(w > 0)) continue;
    Vec::iterator it = v.lower_bound((uint32_t)nodes[at].word);
    if (it != v.end() && it->first == (uint32_t)nodes[at].word) {
      if (weighting <= 1) it->second += w;
    } else {
      v.insert(it, Vec::value_type((uint32_t)nodes[at].word, w));
    }
  }
  double norm = 0.0;
  for (Vec::iterator it = v.begin(); it != v.end(); ++it) norm += fabs(it->second);
  if (norm > 0.0)
    for (Vec::iterator it = v.begin(); it != v.end(); ++it) it->second /= norm;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4) return 4;
  const int voc_bytes = hdr[0], n_desc = hdr[1], n_entries = hdr[2], reps = hdr[3];
  std::vector<uint8_t> voc(voc_bytes);
  std::vector<uint32_t> db_desc((size_t)n_entries * n_desc * 8), q_desc((size_t)n_desc * 8);
  if (fread(voc.data(), 1, voc.size(), f) != voc.size() || fread(db_desc.data(), 4, db_desc.size(), f) != db_desc.size() ||
      fread(q_desc.data(), 4, q_desc.size(), f) != q_desc.size())
    return 4;
  fclose(f);
  int32_t vh[6];
  memcpy(vh, voc.data(), 24);
  weighting = vh[3];
  const int n_nodes = vh[4], n_words = vh[5];
  nodes.resize((size_t)n_nodes + 1);
  for (int r = 0; r < n_nodes; r++) {
    const uint8_t* rec = voc.data() + 24 + (size_t)r * 48;
    int32_t id, pid;
    memcpy(&id, rec, 4), memcpy(&pid, rec + 4, 4);
    memcpy(&nodes[id].weight, rec + 8, 8), memcpy(nodes[id].d, rec + 16, 32);
    nodes[pid].children.push_back(id);
  }
  for (int r = 0; r < n_words; r++) {
    int32_t nid, wid;
    memcpy(&nid, voc.data() + 24 + (size_t)n_nodes * 48 + (size_t)r * 8, 4);
    memcpy(&wid, voc.data() + 24 + (size_t)n_nodes * 48 + (size_t)r * 8 + 4, 4);
    nodes[nid].word = wid;
  }
  // the database: an inverted file, rows in ascending entry id
  std::vector<std::vector<std::pair<int, double>>> ifile((size_t)n_words);
  Vec v;
  for (int e = 0; e < n_entries; e++) {
    transform(db_desc.data() + (size_t)e * n_desc * 8, n_desc, v);
    for (Vec::iterator it = v.begin(); it != v.end(); ++it) ifile[it->first].push_back(std::make_pair(e, it->second));
  }
  double t_transform = 0, t_query = 0;
  uint32_t words_xor = 0;
  std::vector<std::pair<double, int>> ret;
  for (int r = 0; r < reps; r++) {
    double t0 = now_us();
    transform(q_desc.data(), n_desc, v);
    double t1 = now_us();
    std::map<int, double> pairs;
    for (Vec::iterator it = v.begin(); it != v.end(); ++it)
      for (const std::pair<int, double>& row : ifile[it->first]) {
        const double value = fabs(it->second - row.second) - fabs(it->second) - fabs(row.second);
        std::map<int, double>::iterator p = pairs.lower_bound(row.first);
        if (p != pairs.end() && p->first == row.first) p->second += value;
        else pairs.insert(p, std::make_pair(row.first, value));
      }
    ret.clear();
    for (std::map<int, double>::iterator p = pairs.begin(); p != pairs.end(); ++p) ret.push_back(std::make_pair(p->second, p->first));
    std::sort(ret.begin(), ret.end());
    if (ret.size() > 4) ret.resize(4);
    double t2 = now_us();
    t_transform += t1 - t0, t_query += t2 - t0;
  }
  for (Vec::iterator it = v.begin(); it != v.end(); ++it) words_xor ^= it->first;
  printf("transform_us %.1f query_us %.1f words_xor %u ids", t_transform / reps, t_query / reps, words_xor);
  for (size_t i = 0; i < ret.size(); i++) printf(" %d", ret[i].second);
  printf("\n");
  return 0;
}
