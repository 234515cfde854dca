// fe_voc.h — the host side of esvio_fe_bow_create_vocabulary: DBoW2's TemplatedVocabulary::create a level at a time
// (pose_graph/src/ThirdParty/DBoW/TemplatedVocabulary.h:639-995).  include/esvio_fe.h "C, creating a vocabulary" holds
// the rule, fe_kernels.h the kernels and a level's layout, esvio_fe_ctx::Voc the state.  Included by fe_api.cpp alone,
// behind fe_bow.h, whose file check, tree layout and walk it uses.
#pragma once
#include "fe_internal.h"

namespace {
using Voc = esvio_fe_ctx::Voc;
constexpr int64_t kVocMaxDesc = (int64_t)1 << 24;

// the tree as it grows: breadth first, node 0 the root, a node's children contiguous in cluster order
struct VocNode {
  int32_t parent;
  uint32_t first_child, n_child;
  int32_t depth;
  uint32_t desc[8];
};
// a node of the level that is split: its positions, its place in the tree, C5's key
struct VocSeg {
  uint32_t off, m;
  int32_t node;
  uint64_t key;
};

int voc_refuse(esvio_fe_ctx* c, esvio_fe_bow_create_info* info, int code, const char* fmt, ...) {
  char buf[188];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (info) memcpy(info->message, buf, sizeof buf);
  return fail(c, code, "bow_create_vocabulary: %s", buf);
}

template <class T>
int voc_upload(esvio_fe_ctx* c, DevBuf<T>& buf, const std::vector<T>& v) {
  if (int rc = buf.grow(c, v.size())) return rc;
  if (!v.empty()) HIPCHK(c, hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, cur_stream(c)));
  return 0;
}

// run[] of min_dist[0..n)
int voc_scan(esvio_fe_ctx* c, const uint32_t* min_dist, uint32_t n, uint64_t* tile_sum, uint64_t* run) {
  hipStream_t s = cur_stream(c);
  {
    ScopedKernel k(c, K_VOC_SCAN_REDUCE, (uint64_t)n * 4 + (uint64_t)voc_tiles(n) * 8);
    launch_voc_scan_reduce(s, min_dist, n, tile_sum);
  }
  {
    ScopedKernel k(c, K_VOC_SCAN_TOP, (uint64_t)voc_tiles(n) * 16);
    launch_voc_scan_top(s, tile_sum, voc_tiles(n));
  }
  ScopedKernel k(c, K_VOC_SCAN_DOWN, (uint64_t)n * 12 + (uint64_t)voc_tiles(n) * 8);
  launch_voc_scan_down(s, min_dist, n, tile_sum, run);
  return 0;
}

// the stable sort of (keys[src], vals[src]) by the low `passes` digits; the histograms are in the scratch already.
// Returns the buffer that holds the result in *out.
int voc_sort(esvio_fe_ctx* c, uint32_t n, int passes, int src, int* out) {
  Voc& V = c->voc;
  hipStream_t s = cur_stream(c);
  const SortScratch sc = sort_scratch(V.sort);
  const size_t pass_words = (size_t)radix_blocks(n) << kRadixMaxBits;
  int cur = src;
  for (int p = 0; p < passes; p++) {
    ScopedKernel k(c, K_RADIX_PASS, (uint64_t)n * 16);
    launch_radix_pass(s, V.keys[cur], V.vals[cur], n, p * kRadixMaxBits, kRadixMaxBits, sc.ghist + ((size_t)p << kRadixMaxBits),
                      sc.lookback + p * pass_words, sc.tickets + p, V.keys[cur ^ 1], V.vals[cur ^ 1], V.err, c->lim.lookback);
    cur ^= 1;
  }
  *out = cur;
  return 0;
}
int voc_sort_clear(esvio_fe_ctx* c, uint32_t n, int passes) {
  Voc& V = c->voc;
  const size_t pass_words = (size_t)radix_blocks(n) << kRadixMaxBits;
  HIPCHK(c, hipMemsetAsync(V.sort, 0, (kSortHeadWords + (size_t)passes * pass_words) * 4, cur_stream(c)));
  HIPCHK(c, hipMemsetAsync(V.err, 0, 4, cur_stream(c)));
  return 0;
}
int voc_key_passes(uint64_t max_key) {
  int passes = 1;
  while (passes < kRadixMaxPasses && (max_key >> (passes * kRadixMaxBits))) passes++;
  return passes;
}

void voc_put_i32(std::vector<uint8_t>& b, size_t at, int32_t v) { memcpy(b.data() + at, &v, 4); }

// C1..C6 for the descriptors at d (device) / h (the same on the host)
int voc_create_run(esvio_fe_ctx* c, const uint32_t* d, const uint32_t* h, uint32_t n, const int64_t* doc_offsets, int32_t n_docs,
                   const esvio_fe_bow_create_params& P, esvio_fe_bow_create_info* info) {
  Voc& V = c->voc;
  hipStream_t s = cur_stream(c);
  const int k = P.k, L = P.L, max_passes = P.max_passes ? P.max_passes : 100;
  for (int b = 0; b < 2; b++) {
    if (int rc = V.keys[b].grow(c, n)) return rc;
    if (int rc = V.vals[b].grow(c, n)) return rc;
  }
  if (int rc = V.min_dist.grow(c, n)) return rc;
  if (int rc = V.assign.grow(c, n)) return rc;
  if (int rc = V.run.grow(c, n)) return rc;
  if (int rc = V.tile_sum.grow(c, voc_tiles(n))) return rc;
  if (int rc = V.sort.grow(c, sort_scratch_words(n))) return rc;
  if (!V.err)
    if (int rc = V.err.alloc(c, 1)) return rc;

  std::vector<VocNode> nodes(1, VocNode{-1, 0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}});
  std::vector<VocSeg> segs(1, VocSeg{0, n, 0, voc_mix(P.seed)});
  std::vector<uint32_t> h_perm(n);
  for (uint32_t i = 0; i < n; i++) h_perm[i] = i;
  int cur = 0;
  uint32_t na = n;
  HIPCHK(c, hipMemcpyAsync(V.vals[0], h_perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(V.keys[0], 0, (size_t)n * 4, s));
  HIPCHK(c, hipStreamSynchronize(s));

  for (int level = 1; level <= L && !segs.empty(); level++) {
    const uint32_t S = (uint32_t)segs.size();
    std::vector<uint32_t> seg_off(S + 1), seg_slot(S), km_start, km_end, big_km;
    std::vector<int32_t> seg_km(S), km_big;
    std::vector<uint64_t> km_key;
    uint32_t slots = 0;
    bool any_small = false;
    for (uint32_t i = 0; i < S; i++) {
      const VocSeg& g = segs[i];
      seg_off[i] = g.off, seg_slot[i] = slots;
      if (g.m > (uint32_t)k) {
        seg_km[i] = (int32_t)km_start.size();
        km_start.push_back(g.off), km_end.push_back(g.off + g.m), km_key.push_back(g.key);
        km_big.push_back(g.m >= kVocBigNode ? (int32_t)big_km.size() : -1);
        if (g.m >= kVocBigNode) big_km.push_back((uint32_t)seg_km[i]);
        slots += (uint32_t)k;
      } else {
        seg_km[i] = -1, any_small = true;
        slots += g.m;
      }
    }
    seg_off[S] = na;
    const uint32_t K = (uint32_t)km_start.size(), B = (uint32_t)big_km.size();
    if (int rc = voc_upload(c, V.seg_off, seg_off)) return rc;
    if (int rc = voc_upload(c, V.seg_slot, seg_slot)) return rc;
    if (int rc = voc_upload(c, V.seg_km, seg_km)) return rc;
    if (int rc = voc_upload(c, V.km_start, km_start)) return rc;
    if (int rc = voc_upload(c, V.km_end, km_end)) return rc;
    if (int rc = voc_upload(c, V.km_key, km_key)) return rc;
    if (int rc = voc_upload(c, V.km_big, km_big)) return rc;
    if (int rc = voc_upload(c, V.big_km, big_km)) return rc;
    if (int rc = V.ncent.grow(c, K)) return rc;
    if (int rc = V.draws.grow(c, K)) return rc;
    if (int rc = V.stopped.grow(c, K)) return rc;
    if (int rc = V.changed.grow(c, K)) return rc;
    if (int rc = V.cut_d.grow(c, K)) return rc;
    if (int rc = V.pick.grow(c, K)) return rc;
    if (int rc = V.centres.grow(c, (size_t)K * k * 8)) return rc;
    if (int rc = V.counts.grow(c, (size_t)B * k * 257)) return rc;
    if (int rc = V.slot_size.grow(c, slots)) return rc;
    if (int rc = V.slot_map.grow(c, slots)) return rc;
    VocArgs a = {};
    a.desc = d, a.na = na, a.n_seg = S, a.n_km = K, a.n_big = B, a.k = k;
    a.perm = V.vals[cur], a.segof = V.keys[cur], a.seg_off = V.seg_off, a.seg_km = V.seg_km, a.seg_slot = V.seg_slot;
    a.km_start = V.km_start, a.km_end = V.km_end, a.km_key = V.km_key, a.km_big = V.km_big, a.big_km = V.big_km;
    a.ncent = V.ncent, a.draws = V.draws, a.stopped = V.stopped, a.changed = V.changed, a.centres = V.centres;
    a.cut_d = V.cut_d, a.pick = V.pick, a.min_dist = V.min_dist, a.run = V.run, a.tile_sum = V.tile_sum;
    a.assign = V.assign, a.counts = V.counts, a.slot_size = V.slot_size;

    // C2
    if (K) {
      {
        ScopedKernel t(c, K_VOC_FIRST, (uint64_t)K * (32 + 32 + 28));
        launch_voc_first(s, a);
      }
      {
        ScopedKernel t(c, K_VOC_MINDIST, (uint64_t)na * (4 + 4 + 32 + 4));
        launch_voc_mindist(s, a, 1);
      }
      for (int r = 1; r < k; r++) {
        if (r > 1) {  // (against the first centre the distances stand already: TemplatedVocabulary.h:870-879 changes nothing then)
          ScopedKernel t(c, K_VOC_MINDIST, (uint64_t)na * (4 + 4 + 32 + 8));
          launch_voc_mindist(s, a, 0);
        }
        if (int rc = voc_scan(c, V.min_dist, na, V.tile_sum, V.run)) return rc;
        {
          ScopedKernel t(c, K_VOC_DRAW, (uint64_t)K * (8 + 16 + 8 + 12));
          launch_voc_draw(s, a);
        }
        ScopedKernel t(c, K_VOC_PICK, (uint64_t)K * (8 + 8 + 4 + 8 * 24 + 64));
        launch_voc_pick(s, V.run, V.km_start, V.km_end, V.cut_d, K, V.pick, a, 1);
      }
    }
    // C1's passes
    {
      ScopedKernel t(c, K_VOC_ASSIGN, (uint64_t)na * (4 + 4 + 32 + 4) + (uint64_t)K * k * 32);
      launch_voc_assign(s, a, 1);
    }
    if (K) {
      std::vector<int32_t> settled(K, 0);
      std::vector<uint32_t> changed(K);
      uint32_t open = K;
      for (int p = 2; p <= max_passes && open; p++) {
        if (B) {
          HIPCHK(c, hipMemsetAsync(V.counts, 0, (size_t)B * k * 257 * 4, s));
          {
            ScopedKernel t(c, K_VOC_COUNT_BIG, (uint64_t)na * (4 + 4 + 32 + 4));
            launch_voc_count_big(s, a);
          }
          ScopedKernel t(c, K_VOC_MEAN_BIG, (uint64_t)B * k * (257 * 4 + 32));
          launch_voc_mean_big(s, a);
        }
        {
          ScopedKernel t(c, K_VOC_MEAN_SMALL, (uint64_t)na * (4 + 4 + 32) + (uint64_t)K * k * 32);
          launch_voc_mean_small(s, a);
        }
        HIPCHK(c, hipMemsetAsync(V.changed, 0, (size_t)K * 4, s));
        {
          ScopedKernel t(c, K_VOC_ASSIGN, (uint64_t)na * (4 + 4 + 32 + 8) + (uint64_t)K * k * 32);
          launch_voc_assign(s, a, 0);
        }
        HIPCHK(c, hipMemcpyAsync(changed.data(), V.changed, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (uint32_t x = 0; x < K; x++)  // (a settled node is a fixed point: it stays unchanged in every later pass)
          if (!settled[x] && !changed[x]) settled[x] = p, open--, info->passes = std::max(info->passes, p);
      }
      HIPCHK(c, hipGetLastError());
      if (open)
        return voc_refuse(c, info, ESVIO_FE_EINVAL, "%u k-means nodes of level %d have not settled after %d passes (max_passes)", open, level, max_passes);
      info->kmeans_nodes += (int32_t)K;
    }
    // the level's children
    std::vector<uint32_t> ncent(K), stopped(K), centres((size_t)K * k * 8), slot_size(slots), slot_map(slots, 0);
    if (K) {
      HIPCHK(c, hipMemcpyAsync(ncent.data(), V.ncent, (size_t)K * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(stopped.data(), V.stopped, (size_t)K * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(c, hipMemcpyAsync(centres.data(), V.centres, (size_t)K * k * 32, hipMemcpyDeviceToHost, s));
    }
    if (any_small) HIPCHK(c, hipMemcpyAsync(h_perm.data(), V.vals[cur], (size_t)na * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemsetAsync(V.slot_size, 0, (size_t)slots * 4, s));
    {
      ScopedKernel t(c, K_VOC_CHILD_COUNT, (uint64_t)na * 16);
      launch_voc_child_count(s, a);
    }
    HIPCHK(c, hipMemcpyAsync(slot_size.data(), V.slot_size, (size_t)slots * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    std::vector<VocSeg> next;
    uint32_t next_na = 0;
    for (uint32_t i = 0; i < S; i++) {
      const VocSeg g = segs[i];
      const int32_t x = seg_km[i];
      const uint32_t nc = x >= 0 ? ncent[x] : g.m;
      if (nc < 1 || nc > (uint32_t)k) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: a node with %u clusters", nc);
      if (x >= 0) info->short_seedings += (int32_t)(stopped[x] != 0);
      nodes[g.node].first_child = (uint32_t)nodes.size(), nodes[g.node].n_child = nc;
      for (uint32_t cl = 0; cl < nc; cl++) {
        VocNode ch{g.node, 0, 0, level, {}};
        if (x >= 0) memcpy(ch.desc, &centres[((size_t)x * k + cl) * 8], 32);
        else {
          const uint32_t f = h_perm[g.off + cl];
          if (f >= n) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: feature %u of %u", f, n);
          memcpy(ch.desc, h + (size_t)f * 8, 32);
        }
        const uint32_t size = slot_size[seg_slot[i] + cl];
        if (x >= 0 && !size) info->empty_clusters++;
        if (level < L && size > 1) {  // TemplatedVocabulary.h:793-815
          slot_map[seg_slot[i] + cl] = (uint32_t)next.size();
          next.push_back(VocSeg{next_na, size, (int32_t)nodes.size(), voc_mix(g.key ^ (uint64_t)(cl + 1))});
          next_na += size;
        } else {
          slot_map[seg_slot[i] + cl] = 0xffffffffu;
        }
        nodes.push_back(ch);
      }
    }
    if (next.empty() || next_na > na) {
      if (next_na > na) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: %u positions from %u", next_na, na);
      break;
    }
    // the next level's positions: a stable sort by the child's segment, the children that are not split behind them
    const uint32_t dead = (uint32_t)next.size();
    for (uint32_t& m : slot_map)
      if (m == 0xffffffffu) m = dead;
    const int passes = voc_key_passes(dead);
    HIPCHK(c, hipMemcpyAsync(V.slot_map, slot_map.data(), (size_t)slots * 4, hipMemcpyHostToDevice, s));
    if (int rc = voc_sort_clear(c, na, passes)) return rc;
    {
      ScopedKernel t(c, K_VOC_REGROUP_KEYS, (uint64_t)na * 28);
      launch_voc_regroup_keys(s, a, V.slot_map, passes, V.keys[cur ^ 1], V.vals[cur ^ 1], sort_scratch(V.sort).ghist);
    }
    int res = 0;
    if (int rc = voc_sort(c, na, passes, cur ^ 1, &res)) return rc;
    int32_t err = 0;
    HIPCHK(c, hipMemcpyAsync(&err, V.err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (err) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: radix sort look-back spin expired");
    cur = res, na = next_na;
    segs.swap(next);
  }

  // C1's ids: a node's children at the push, child 0's whole subtree first
  const size_t nn = nodes.size();
  std::vector<int32_t> id(nn, 0), of_id(nn, 0);
  {
    int32_t next_id = 1;
    std::vector<std::pair<uint32_t, uint32_t>> stack;  // (node, the child to go down next)
    auto push = [&](uint32_t u) {
      for (uint32_t j = 0; j < nodes[u].n_child; j++) id[nodes[u].first_child + j] = next_id++;
      stack.emplace_back(u, 0u);
    };
    push(0);
    while (!stack.empty()) {
      auto& top = stack.back();
      if (top.second == nodes[top.first].n_child) {
        stack.pop_back();
        continue;
      }
      const uint32_t ch = nodes[top.first].first_child + top.second++;
      if (nodes[ch].n_child) push(ch);
    }
    for (size_t u = 1; u < nn; u++) of_id[id[u]] = (int32_t)u;
  }
  // C4, C6
  std::vector<int32_t> leaf_ids;
  for (size_t i = 1; i < nn; i++) {
    const VocNode& u = nodes[of_id[i]];
    info->max_children = std::max<int32_t>(info->max_children, (int32_t)u.n_child);
    if (!u.n_child) leaf_ids.push_back((int32_t)i), info->depth = std::max(info->depth, u.depth);
  }
  info->max_children = std::max<int32_t>(info->max_children, (int32_t)nodes[0].n_child);
  const size_t nNodes = nn - 1, nWords = leaf_ids.size();
  std::vector<uint8_t> img(kBowHeaderBytes + nNodes * kBowNodeBytes + nWords * kBowWordBytes, 0);
  voc_put_i32(img, 0, k), voc_put_i32(img, 4, L), voc_put_i32(img, 8, P.scoring), voc_put_i32(img, 12, P.weighting);
  voc_put_i32(img, 16, (int32_t)nNodes), voc_put_i32(img, 20, (int32_t)nWords);
  const double one = 1.0;
  for (size_t i = 1; i < nn; i++) {
    const VocNode& u = nodes[of_id[i]];
    const size_t at = kBowHeaderBytes + (i - 1) * kBowNodeBytes;
    voc_put_i32(img, at, (int32_t)i), voc_put_i32(img, at + 4, id[u.parent]);
    if (!u.n_child) memcpy(img.data() + at + 8, &one, 8);
    memcpy(img.data() + at + 16, u.desc, 32);
  }
  const size_t words_at = kBowHeaderBytes + nNodes * kBowNodeBytes;
  for (size_t w = 0; w < nWords; w++) voc_put_i32(img, words_at + w * 8, leaf_ids[w]), voc_put_i32(img, words_at + w * 8 + 4, (int32_t)w);
  esvio_fe_bow_vocabulary_info vinfo;
  BowLayout lay;
  if (int rc = bow_parse(img.data(), img.size(), &vinfo, &lay)) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: the image fails its own check (%d): %s", rc, vinfo.message);

  if (P.weighting == 0 || P.weighting == 2) {  // TF_IDF, IDF: setNodeWeights, TemplatedVocabulary.h:954-993
    if (int rc = V.tree_desc.grow(c, nn * 2)) return rc;
    if (int rc = V.tree_kids.grow(c, nn)) return rc;
    if (int rc = V.tree_word.grow(c, nn)) return rc;
    if (int rc = V.tree_weight.grow(c, nn)) return rc;
    if (int rc = V.word.grow(c, n)) return rc;
    if (int rc = V.weight.grow(c, n)) return rc;
    if (int rc = V.ni.grow(c, nWords)) return rc;
    if (int rc = V.doc_off.grow(c, (size_t)n_docs + 1)) return rc;
    HIPCHK(c, hipMemcpyAsync(V.tree_desc, lay.desc.data(), nn * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(V.tree_kids, lay.kids.data(), nn * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(V.tree_word, lay.word.data(), nn * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(V.tree_weight, lay.weight.data(), nn * 8, hipMemcpyHostToDevice, s));  // 1.0 at every leaf: no key is stopped
    HIPCHK(c, hipMemcpyAsync(V.doc_off, doc_offsets, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(V.ni, 0, nWords * 4, s));
    const int passes = voc_key_passes(nWords);
    if (int rc = voc_sort_clear(c, n, passes)) return rc;
    {
      ScopedKernel t(c, K_BOW_WALK, (uint64_t)n * (32 + 32 * (uint64_t)vinfo.max_children * (uint64_t)vinfo.depth + 20));
      launch_bow_walk(s, d, n, V.tree_desc, V.tree_kids, V.tree_word, V.tree_weight, (uint32_t)nWords, passes, V.word, V.weight,
                      V.keys[0], V.vals[0], sort_scratch(V.sort).ghist);
    }
    int res = 0;
    if (int rc = voc_sort(c, n, passes, 0, &res)) return rc;
    {
      ScopedKernel t(c, K_VOC_DOC_COUNT, (uint64_t)n * 20);
      launch_voc_doc_count(s, V.keys[res], V.vals[res], n, V.doc_off, (uint32_t)n_docs, (uint32_t)nWords, V.ni);
    }
    std::vector<uint32_t> ni(nWords);
    int32_t err = 0;
    HIPCHK(c, hipMemcpyAsync(ni.data(), V.ni, nWords * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&err, V.err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (err) return fail(c, ESVIO_FE_EINTERNAL, "bow_create_vocabulary: radix sort look-back spin expired");
    for (size_t w = 0; w < nWords; w++) {
      const double wt = ni[w] ? log((double)n_docs / (double)ni[w]) : 0.0;  // :985-991; Node() leaves 0
      memcpy(img.data() + kBowHeaderBytes + (size_t)(leaf_ids[w] - 1) * kBowNodeBytes + 8, &wt, 8);
    }
  }
  info->nodes = (int32_t)nNodes, info->words = (int32_t)nWords, info->bytes = img.size();
  V.image.swap(img);
  return 0;
}
}  // namespace

extern "C" {

int esvio_fe_bow_create_kernel_count(void) { return kVocKernels; }
const char* esvio_fe_bow_create_kernel_name(int which) { return which >= 0 && which < kVocKernels ? kVocKernelNames[which] : ""; }
int esvio_fe_bow_create_kernel_stats(esvio_fe_handle c, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c || which < 0 || which >= kVocKernels) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  const KStat& s = c->stats[K_VOC_FIRST + which];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}

int esvio_fe_bow_create_vocabulary(esvio_fe_handle c, const uint32_t* desc, int64_t n, int space, const int64_t* doc_offsets,
                                   int32_t n_docs, const esvio_fe_bow_create_params* params, esvio_fe_bow_create_info* info) {
  if (!info) return fail(c, ESVIO_FE_EINVAL, "bow_create_vocabulary: info is null");
  memset(info, 0, sizeof *info);
  if (!params) return voc_refuse(c, info, ESVIO_FE_EINVAL, "params is null");
  const esvio_fe_bow_create_params P = *params;
  // C7 (a null handle is refused behind it: the checks need neither a handle nor a device)
  if (!kf_space_ok(space)) return voc_refuse(c, info, ESVIO_FE_EINVAL, "bad memory space %d", space);
  if (n < 1 || n > kVocMaxDesc) return voc_refuse(c, info, ESVIO_FE_EINVAL, "n must be in 1..2^24 (got %lld)", (long long)n);
  if (P.k < 2 || P.k > 32) return voc_refuse(c, info, ESVIO_FE_EINVAL, "k must be in 2..32 (got %d)", P.k);
  if (P.L < 1 || P.L > 10) return voc_refuse(c, info, ESVIO_FE_EINVAL, "L must be in 1..10 (got %d)", P.L);
  if (P.weighting < 0 || P.weighting > 3) return voc_refuse(c, info, ESVIO_FE_EINVAL, "weighting %d is outside 0..3", P.weighting);
  if (P.scoring != 0) return voc_refuse(c, info, ESVIO_FE_ENOTIMPL, "scoring %d: only L1_NORM (0) is built", P.scoring);
  if (P.max_passes < 0) return voc_refuse(c, info, ESVIO_FE_EINVAL, "max_passes must not be negative (got %d)", P.max_passes);
  if (!desc || !doc_offsets) return voc_refuse(c, info, ESVIO_FE_EINVAL, "desc or doc_offsets is null");
  if (n_docs < 1) return voc_refuse(c, info, ESVIO_FE_EINVAL, "n_docs must be at least 1 (got %d)", n_docs);
  if (doc_offsets[0] != 0) return voc_refuse(c, info, ESVIO_FE_EINVAL, "doc_offsets[0] is %lld, not 0", (long long)doc_offsets[0]);
  for (int32_t j = 0; j < n_docs; j++)
    if (doc_offsets[j + 1] < doc_offsets[j])
      return voc_refuse(c, info, ESVIO_FE_EINVAL, "doc_offsets[%d] = %lld lies below doc_offsets[%d] = %lld", j + 1, (long long)doc_offsets[j + 1], j, (long long)doc_offsets[j]);
  if (doc_offsets[n_docs] != n)
    return voc_refuse(c, info, ESVIO_FE_EINVAL, "doc_offsets[n_docs] is %lld, not n = %lld", (long long)doc_offsets[n_docs], (long long)n);
  if (!kf_desc_aligned(desc, space)) return voc_refuse(c, info, ESVIO_FE_EINVAL, "device descriptors must be 16-byte aligned");
  if (!c) return voc_refuse(c, info, ESVIO_FE_EINVAL, "the handle is null");
  KfAllocs allocs(c);
  HIPCHK(c, hipSetDevice(c->dev));
  Voc& V = c->voc;
  hipStream_t s = cur_stream(c);
  const size_t N = (size_t)n;
  const uint32_t* d = desc;
  const uint32_t* h = desc;
  std::vector<uint32_t> host_copy;
  if (space == ESVIO_FE_HOST) {
    if (int rc = V.desc.grow(c, N * 8)) return rc;
    HIPCHK(c, hipMemcpyAsync(V.desc, desc, N * 32, hipMemcpyHostToDevice, s));
    d = V.desc;
  } else {  // (the m <= k nodes' children are features: the host writes them into the image)
    host_copy.resize(N * 8);
    HIPCHK(c, hipMemcpyAsync(host_copy.data(), desc, N * 32, hipMemcpyDeviceToHost, s));
    h = host_copy.data();
  }
  HIPCHK(c, hipStreamSynchronize(s));
  const int rc = voc_create_run(c, d, h, (uint32_t)n, doc_offsets, n_docs, P, info);
  if (rc) {
    (void)hipStreamSynchronize(s);
    esvio_fe_bow_create_info failed = {};
    snprintf(failed.message, sizeof failed.message, "%s", info->message[0] ? info->message : c->err.c_str());
    *info = failed;
    return rc;
  }
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_get_created(esvio_fe_handle c, void* out, size_t cap) {
  if (!c) return ESVIO_FE_EINVAL;
  const std::vector<uint8_t>& img = c->voc.image;
  if (img.empty()) return fail(c, ESVIO_FE_EINVAL, "bow_get_created: no vocabulary has been created (esvio_fe_bow_create_vocabulary)");
  if (!out || cap < img.size()) return fail(c, ESVIO_FE_EINVAL, "bow_get_created: the image takes %zu bytes (info.bytes), out has room for %zu", img.size(), out ? cap : (size_t)0);
  memcpy(out, img.data(), img.size());
  return 0;
}

int esvio_fe_bow_create_pick(esvio_fe_handle c, const uint32_t* min_dist, int64_t n, const uint32_t* seg_off, int32_t n_seg,
                             const double* cut_d, uint32_t* pick) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_create_pick";
  KfAllocs allocs(c);
  if (!min_dist || !seg_off || !cut_d || !pick) return fail(c, ESVIO_FE_EINVAL, "%s: a null array", who);
  if (n < 1 || n > kVocMaxDesc || n_seg < 1 || n_seg > n + 1) return fail(c, ESVIO_FE_EINVAL, "%s: n must be in 1..2^24 and n_seg in 1..n + 1 (got %lld, %d)", who, (long long)n, n_seg);
  for (int32_t j = 0; j <= n_seg; j++)
    if (seg_off[j] > (uint64_t)n || (j && seg_off[j] < seg_off[j - 1]))
      return fail(c, ESVIO_FE_EINVAL, "%s: seg_off[%d] = %u is not ascending inside 0..n", who, j, seg_off[j]);
  HIPCHK(c, hipSetDevice(c->dev));
  Voc& V = c->voc;
  hipStream_t s = cur_stream(c);
  const uint32_t n32 = (uint32_t)n, S = (uint32_t)n_seg;
  if (int rc = V.min_dist.grow(c, n32)) return rc;
  if (int rc = V.run.grow(c, n32)) return rc;
  if (int rc = V.tile_sum.grow(c, voc_tiles(n32))) return rc;
  if (int rc = V.seg_off.grow(c, (size_t)S + 1)) return rc;
  if (int rc = V.cut_d.grow(c, S)) return rc;
  if (int rc = V.pick.grow(c, S)) return rc;
  HIPCHK(c, hipMemcpyAsync(V.min_dist, min_dist, (size_t)n32 * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(V.seg_off, seg_off, ((size_t)S + 1) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(V.cut_d, cut_d, (size_t)S * 8, hipMemcpyHostToDevice, s));
  if (int rc = voc_scan(c, V.min_dist, n32, V.tile_sum, V.run)) return rc;
  {
    ScopedKernel t(c, K_VOC_PICK, (uint64_t)S * (8 + 8 + 4 + 8 * 24));
    launch_voc_pick(s, V.run, V.seg_off, V.seg_off.p + 1, V.cut_d, S, V.pick, VocArgs{}, 0);
  }
  HIPCHK(c, hipMemcpyAsync(pick, V.pick, (size_t)S * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

}  // extern "C"
