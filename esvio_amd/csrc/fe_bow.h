// fe_bow.h — the host side of loop detection (esvio_fe_bow_*): the vocabulary file's check and its layout for the
// device, DBoW2's transform / add / query as launches (PoseGraph::detectLoop, pose_graph/src/pose_graph.cpp:331-406).
// include/esvio_fe.h "loop detection" holds the rules, fe_kernels.h the kernels, esvio_fe_ctx::Bow the state.  Included
// by fe_api.cpp alone, behind fe_kf.h (whose argument helpers it shares).
#pragma once
#include "fe_internal.h"

namespace {
using Bow = esvio_fe_ctx::Bow;
constexpr int kBowMaxDesc = 1 << 20;
constexpr size_t kBowHeaderBytes = 24, kBowNodeBytes = 48, kBowWordBytes = 8;

// the tree as the kernels read it (fe_kernels.h): node 0 the root, every node's children contiguous in child order
struct BowLayout {
  std::vector<uint32_t> desc;  // [nodes + 1][8]
  std::vector<uint32_t> kids;  // [nodes + 1][2]: first child, child count
  std::vector<int32_t> word;   // [nodes + 1]: -1 at inner nodes
  std::vector<double> weight;  // [nodes + 1]
  std::vector<double> word_weight;  // [words]
};

int bow_refuse(esvio_fe_bow_vocabulary_info* info, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(info->message, sizeof info->message, fmt, ap);
  va_end(ap);
  return code;
}
int32_t bow_i32(const uint8_t* p) {
  int32_t v;
  memcpy(&v, p, 4);
  return v;
}

// rule V: every item that would make loadBin (TemplatedVocabulary.h:1509-1561) or a walk read out of bounds is refused by
// name; `out` (optional) receives the layout.  No device, no handle.
int bow_parse(const uint8_t* b, size_t nb, esvio_fe_bow_vocabulary_info* info, BowLayout* out) {
  memset(info, 0, sizeof *info);
  if (nb < kBowHeaderBytes) return bow_refuse(info, ESVIO_FE_EINVAL, "byte count: %zu bytes, the header alone takes %zu", nb, kBowHeaderBytes);
  info->k = bow_i32(b), info->L = bow_i32(b + 4), info->scoring = bow_i32(b + 8), info->weighting = bow_i32(b + 12);
  info->nodes = bow_i32(b + 16), info->words = bow_i32(b + 20);
  const int64_t nNodes = info->nodes, nWords = info->words;
  if (nNodes < 1) return bow_refuse(info, ESVIO_FE_EINVAL, "nNodes is %lld: below 1", (long long)nNodes);
  if (nWords < 0) return bow_refuse(info, ESVIO_FE_EINVAL, "byte count: nWords is %lld, no size follows from it", (long long)nWords);
  const uint64_t want = kBowHeaderBytes + (uint64_t)nNodes * kBowNodeBytes + (uint64_t)nWords * kBowWordBytes;
  if ((uint64_t)nb != want)
    return bow_refuse(info, ESVIO_FE_EINVAL, "byte count: %zu bytes, the header implies %llu (%lld nodes, %lld words)", nb,
                      (unsigned long long)want, (long long)nNodes, (long long)nWords);
  if (info->weighting < 0 || info->weighting > 3) return bow_refuse(info, ESVIO_FE_EINVAL, "weighting %d is outside 0..3", info->weighting);
  if (info->scoring != 0) return bow_refuse(info, ESVIO_FE_ENOTIMPL, "scoring %d: only L1_NORM (0) is built", info->scoring);
  const size_t nn = (size_t)nNodes + 1;
  const uint8_t* nodes = b + kBowHeaderBytes;
  const uint8_t* words = nodes + (size_t)nNodes * kBowNodeBytes;
  std::vector<int32_t> rec_of(nn, -1), parent(nn, 0);
  std::vector<uint32_t> cnt(nn, 0), start(nn + 1, 0);
  for (int64_t r = 0; r < nNodes; r++) {
    const int32_t id = bow_i32(nodes + r * kBowNodeBytes), pid = bow_i32(nodes + r * kBowNodeBytes + 4);
    if (id < 1 || id > nNodes) return bow_refuse(info, ESVIO_FE_EINVAL, "nodeId %d of record %lld is outside 1..%lld", id, (long long)r, (long long)nNodes);
    if (rec_of[id] != -1) return bow_refuse(info, ESVIO_FE_EINVAL, "nodeId %d is duplicated (records %d and %lld)", id, rec_of[id], (long long)r);
    if (pid < 0 || pid > nNodes) return bow_refuse(info, ESVIO_FE_EINVAL, "parentId %d of node %d is outside 0..%lld", pid, id, (long long)nNodes);
    if (pid == id) return bow_refuse(info, ESVIO_FE_EINVAL, "parentId %d equals its own node", pid);
    rec_of[id] = (int32_t)r, parent[id] = pid, cnt[pid]++;
  }
  if (!cnt[0]) return bow_refuse(info, ESVIO_FE_EINVAL, "the root has no children");
  for (size_t i = 0; i < nn; i++) start[i + 1] = start[i] + cnt[i];
  // children.push_back: file order
  std::vector<int32_t> child(nNodes);
  {
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (int64_t r = 0; r < nNodes; r++) {
      const int32_t id = bow_i32(nodes + r * kBowNodeBytes);
      child[fill[parent[id]]++] = id;
    }
  }
  // breadth first from the root: a node's children get consecutive places
  std::vector<int32_t> new_of(nn, -1), old_of, depth(nn, 0);
  old_of.reserve(nn);
  old_of.push_back(0);
  new_of[0] = 0;
  for (size_t head = 0; head < old_of.size(); head++) {
    const int32_t o = old_of[head];
    for (uint32_t j = start[o]; j < start[o + 1]; j++) {
      const int32_t ch = child[j];
      new_of[ch] = (int32_t)old_of.size();
      depth[ch] = depth[o] + 1;
      old_of.push_back(ch);
    }
  }
  if (old_of.size() != nn)
    for (size_t id = 1; id < nn; id++)
      if (new_of[id] < 0) return bow_refuse(info, ESVIO_FE_EINVAL, "node %zu is not reachable from the root", id);
  std::vector<int32_t> word_of(nn, -1), node_of_word((size_t)nWords, -1);
  for (int64_t r = 0; r < nWords; r++) {
    const int32_t nid = bow_i32(words + r * kBowWordBytes), wid = bow_i32(words + r * kBowWordBytes + 4);
    if (wid < 0 || wid >= nWords) return bow_refuse(info, ESVIO_FE_EINVAL, "wordId %d is outside 0..%lld", wid, (long long)nWords - 1);
    if (node_of_word[wid] != -1) return bow_refuse(info, ESVIO_FE_EINVAL, "wordId %d is duplicated", wid);
    if (nid < 1 || nid > nNodes) return bow_refuse(info, ESVIO_FE_EINVAL, "word %d is on nodeId %d, outside 1..%lld", wid, nid, (long long)nNodes);
    if (cnt[nid]) return bow_refuse(info, ESVIO_FE_EINVAL, "word %d is on node %d, which has children", wid, nid);
    node_of_word[wid] = nid, word_of[nid] = wid;
  }
  for (size_t id = 1; id < nn; id++) {
    info->max_children = std::max<int32_t>(info->max_children, (int32_t)cnt[id]);
    if (cnt[id]) continue;
    info->leaves++;
    info->depth = std::max(info->depth, depth[id]);
    if (word_of[id] < 0) return bow_refuse(info, ESVIO_FE_EINVAL, "leaf node %zu has no word", id);
  }
  info->max_children = std::max<int32_t>(info->max_children, (int32_t)cnt[0]);
  if (!out) return 0;
  out->desc.assign(nn * 8, 0), out->kids.assign(nn * 2, 0), out->word.assign(nn, -1), out->weight.assign(nn, 0.0);
  out->word_weight.assign((size_t)nWords, 0.0);
  for (size_t i = 0; i < nn; i++) {
    const int32_t o = old_of[i];
    out->kids[2 * i] = cnt[o] ? (uint32_t)new_of[child[start[o]]] : 0u;
    out->kids[2 * i + 1] = cnt[o];
    if (!o) continue;
    const uint8_t* rec = nodes + (size_t)rec_of[o] * kBowNodeBytes;
    memcpy(&out->weight[i], rec + 8, 8);
    memcpy(&out->desc[i * 8], rec + 16, 32);  // bit i = bit i & 63 of descriptor[i >> 6] = bit i & 31 of word i >> 5
    out->word[i] = word_of[o];
  }
  for (int64_t w = 0; w < nWords; w++) out->word_weight[w] = out->weight[new_of[node_of_word[w]]];
  return 0;
}

int bow_ready(esvio_fe_ctx* c, const char* who) {
  return c->bow.has_voc ? 0 : fail(c, ESVIO_FE_EINVAL, "%s: no vocabulary is set (esvio_fe_bow_set_vocabulary)", who);
}
int bow_desc_check(esvio_fe_ctx* c, const char* who, const uint32_t* desc, int n, int space) {
  if (!kf_space_ok(space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d", who, space);
  if (n < 0 || n > kBowMaxDesc) return fail(c, ESVIO_FE_EINVAL, "%s: n must be in 0..2^20 (got %d)", who, n);
  if (n && !desc) return fail(c, ESVIO_FE_EINVAL, "%s: desc is null with n = %d", who, n);
  if (n && !kf_desc_aligned(desc, space)) return fail(c, ESVIO_FE_EINVAL, "%s: device descriptors must be 16-byte aligned", who);
  return bow_ready(c, who);
}
uint32_t bow_entries(const Bow& B) { return (uint32_t)(B.off.size() - 1); }

// W and T of n descriptors: word / weight per descriptor in B.word / B.weight, the vector in B.q_word / B.q_val, its
// length in B.q_n.  Waits for the vector's length.
int bow_transform_run(esvio_fe_ctx* c, const uint32_t* desc, int n, int space) {
  Bow& B = c->bow;
  B.q_n = 0;
  if (!n) return 0;
  hipStream_t s = cur_stream(c);
  const size_t N = (size_t)n;
  const uint32_t n32 = (uint32_t)n;
  if (space == ESVIO_FE_HOST)
    if (int rc = B.desc.grow(c, N * 8)) return rc;
  if (int rc = B.word.grow(c, N)) return rc;
  if (int rc = B.weight.grow(c, N)) return rc;
  for (int k = 0; k < 2; k++) {
    if (int rc = B.keys[k].grow(c, N)) return rc;
    if (int rc = B.vals[k].grow(c, N)) return rc;
  }
  if (int rc = B.heads.grow(c, N)) return rc;
  if (int rc = B.q_word.grow(c, N)) return rc;
  if (int rc = B.q_val.grow(c, N)) return rc;
  if (int rc = B.sort.grow(c, sort_scratch_words(N))) return rc;
  if (!B.cnt)
    if (int rc = B.cnt.alloc(c, 4)) return rc;
  if (!B.err)
    if (int rc = B.err.alloc(c, 1)) return rc;
  const uint32_t* d = desc;
  if (space == ESVIO_FE_HOST) {
    HIPCHK(c, hipMemcpyAsync(B.desc, desc, N * 32, hipMemcpyHostToDevice, s));
    d = B.desc;
  }
  const SortScratch sc = sort_scratch(B.sort);
  const size_t pass_words = (size_t)radix_blocks(n32) << kRadixMaxBits;
  HIPCHK(c, hipMemsetAsync(B.sort, 0, (kSortHeadWords + (size_t)B.passes * pass_words) * 4, s));  // histograms, tickets, look-back words
  HIPCHK(c, hipMemsetAsync(B.err, 0, 4, s));
  const uint32_t invalid = (uint32_t)B.info.words;  // above every word id, inside the passes' digits
  {
    // the descriptor, at most max_children x depth child descriptors, word, weight and the sort's pair
    ScopedKernel k(c, K_BOW_WALK, (uint64_t)n * (32 + 32 * (uint64_t)B.info.max_children * (uint64_t)B.info.depth + 20));
    launch_bow_walk(s, d, n32, B.node_desc, B.kids, B.node_word, B.node_weight, invalid, B.passes, B.word, B.weight, B.keys[0],
                    B.vals[0], sc.ghist);
  }
  int cur = 0;
  for (int p = 0; p < B.passes; p++) {
    ScopedKernel k(c, K_RADIX_PASS, (uint64_t)n * 16);
    launch_radix_pass(s, B.keys[cur], B.vals[cur], n32, p * kRadixMaxBits, kRadixMaxBits, sc.ghist + ((size_t)p << kRadixMaxBits),
                      sc.lookback + p * pass_words, sc.tickets + p, B.keys[cur ^ 1], B.vals[cur ^ 1], B.err, c->lim.lookback);
    cur ^= 1;
  }
  {
    ScopedKernel k(c, K_BOW_VECTOR, (uint64_t)n * (4 + 4 + 12 + 8));  // keys, heads, the vector written, its values divided
    launch_bow_vector(s, B.keys[cur], n32, invalid, B.word_weight, B.info.weighting <= 1, B.heads, B.q_word, B.q_val, B.cnt);
  }
  uint32_t cnt[2] = {0, 0};
  int32_t err = 0;
  HIPCHK(c, hipMemcpyAsync(cnt, B.cnt, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(&err, B.err, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (err) return fail(c, ESVIO_FE_EINTERNAL, "bow: radix sort look-back spin expired");
  if (cnt[0] > n32) return fail(c, ESVIO_FE_EINTERNAL, "bow: a vector of %u words from %d descriptors", cnt[0], n);
  B.q_n = cnt[0];
  return 0;
}

// room for `need` elements in a pool whose first `used` are kept.  (db_off after a reserve on an empty database is
// allocated and not yet written: its one "used" element is copied as it is, which is harmless — every add writes
// db_off[N] and db_off[N + 1] itself, and nothing reads an offset beyond the entries.)
template <class T>
int bow_pool_grow(esvio_fe_ctx* c, DevBuf<T>& buf, size_t used, size_t need, bool spare) {
  if (need <= buf.cap) return 0;
  DevBuf<T> bigger;
  if (int rc = bigger.alloc(c, spare ? std::max<size_t>(need + need / 4, 1024) : need)) return rc;
  if (used) HIPCHK(c, hipMemcpyAsync(bigger.p, buf.p, used * sizeof(T), hipMemcpyDeviceToDevice, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  buf = std::move(bigger);
  return 0;
}
int bow_room(esvio_fe_ctx* c, size_t entries, size_t words, bool spare) {
  Bow& B = c->bow;
  const size_t N = bow_entries(B);
  if (int rc = bow_pool_grow(c, B.db_word, (size_t)B.off[N], words, spare)) return rc;
  if (int rc = bow_pool_grow(c, B.db_val, (size_t)B.off[N], words, spare)) return rc;
  if (int rc = bow_pool_grow(c, B.db_off, B.db_off ? N + 1 : 0, entries + 1, spare)) return rc;
  if (spare) {
    if (int rc = B.score.grow(c, entries)) return rc;
    return B.present.grow(c, entries);
  }
  if (entries > B.score.cap)
    if (int rc = B.score.alloc(c, entries)) return rc;
  if (entries > B.present.cap)
    if (int rc = B.present.alloc(c, entries)) return rc;
  return 0;
}

// A with the vector bow_transform_run left
int bow_add_run(esvio_fe_ctx* c, int32_t* entry_id) {
  Bow& B = c->bow;
  const size_t N = bow_entries(B), m = B.q_n;
  if (N >= 0x7ffffffeu) return fail(c, ESVIO_FE_EINVAL, "bow_add: the database is full");
  if (int rc = bow_room(c, N + 1, (size_t)B.off[N] + m, true)) return rc;
  hipStream_t s = cur_stream(c);
  if (m) {
    HIPCHK(c, hipMemcpyAsync(B.db_word.p + B.off[N], B.q_word, m * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemcpyAsync(B.db_val.p + B.off[N], B.q_val, m * 8, hipMemcpyDeviceToDevice, s));
  }
  // the entry exists on the host only once the device holds it: a failed copy leaves the database as it was
  const uint64_t ends[2] = {B.off[N], B.off[N] + m};
  HIPCHK(c, hipMemcpyAsync(B.db_off.p + N, ends, 16, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));
  B.off.push_back(ends[1]);
  if (entry_id) *entry_id = (int32_t)N;
  return 0;
}

// Q's sums for the vector bow_transform_run left: B.score / B.present for every entry.  Nothing is waited for.
int bow_score_enqueue(esvio_fe_ctx* c, int max_id) {
  Bow& B = c->bow;
  const uint32_t N = bow_entries(B);
  if (!N) return 0;
  uint64_t words = B.off[N];
  // the entries' pairs, the query's words per workgroup, the results
  ScopedKernel k(c, K_BOW_SCORE, words * 12 + (uint64_t)std::min<uint32_t>((N + 3) / 4, 1024) * B.q_n * 4 + (uint64_t)N * 17);
  launch_bow_score(cur_stream(c), B.q_word, B.q_val, B.q_n, B.db_word, B.db_val, B.db_off, N, max_id, B.score, B.present);
  return 0;
}
// ... and the first max_results of them on the host
int bow_select_run(esvio_fe_ctx* c, int max_results, esvio_fe_bow_result* results, int32_t* n_results) {
  Bow& B = c->bow;
  const uint32_t N = bow_entries(B);
  *n_results = 0;
  if (!N) return 0;
  hipStream_t s = cur_stream(c);
  if (!B.res_id) {
    if (int rc = B.res_id.alloc(c, kBowMaxResults)) return rc;
    if (int rc = B.res_score.alloc(c, kBowMaxResults)) return rc;
    if (int rc = B.res_raw.alloc(c, kBowMaxResults)) return rc;
  }
  {
    ScopedKernel k(c, K_BOW_SELECT, (uint64_t)N * 9);  // (per result taken)
    launch_bow_select(s, B.score, B.present, N, max_results, B.res_id, B.res_score, B.res_raw, B.cnt.p + 2);
  }
  int32_t id[kBowMaxResults];
  double score[kBowMaxResults];
  uint32_t k = 0;
  HIPCHK(c, hipMemcpyAsync(id, B.res_id, (size_t)max_results * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(score, B.res_score, (size_t)max_results * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(&k, B.cnt.p + 2, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (k > (uint32_t)max_results) return fail(c, ESVIO_FE_EINTERNAL, "bow: %u results of %d", k, max_results);
  for (uint32_t i = 0; i < k; i++) results[i].id = id[i], results[i].score = score[i];
  *n_results = (int32_t)k;
  return 0;
}
// the query's scratch for `entries` entries, on first use (the cnt word the selection counts in is bow_transform_run's)
int bow_query_room(esvio_fe_ctx* c) {
  Bow& B = c->bow;
  const size_t N = bow_entries(B);
  if (!B.cnt)
    if (int rc = B.cnt.alloc(c, 4)) return rc;
  if (int rc = B.score.grow(c, N)) return rc;
  return B.present.grow(c, N);
}
}  // namespace

extern "C" {

int esvio_fe_bow_kernel_count(void) { return kBowKernels; }
const char* esvio_fe_bow_kernel_name(int which) { return which >= 0 && which < kBowKernels ? kBowKernelNames[which] : ""; }
int esvio_fe_bow_kernel_stats(esvio_fe_handle c, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c || which < 0 || which >= kBowKernels) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  const KStat& s = c->stats[K_BOW_WALK + which];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}
int esvio_fe_bow_limits(esvio_fe_bow_limits_info* out) {
  if (!out) return ESVIO_FE_EINVAL;
  out->group_lanes = kBowGroup, out->lds_words = kBowLdsWords, out->vector_block = kBowVectorBlock, out->max_results = kBowMaxResults;
  return 0;
}

int esvio_fe_bow_vocabulary_header(const void* bytes, size_t n_bytes, esvio_fe_bow_vocabulary_info* info) {
  if (!info) return ESVIO_FE_EINVAL;
  if (!bytes) {
    memset(info, 0, sizeof *info);
    return bow_refuse(info, ESVIO_FE_EINVAL, "the file image is null");
  }
  return bow_parse((const uint8_t*)bytes, n_bytes, info, nullptr);
}

int esvio_fe_bow_set_vocabulary(esvio_fe_handle c, const void* bytes, size_t n_bytes) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_set_vocabulary";
  KfAllocs allocs(c);
  Bow& B = c->bow;
  if (!bytes) return fail(c, ESVIO_FE_EINVAL, "%s: the file image is null", who);
  if (bow_entries(B)) return fail(c, ESVIO_FE_EINVAL, "%s: the database holds %u entries of the vocabulary in use (esvio_fe_bow_clear)", who, bow_entries(B));
  esvio_fe_bow_vocabulary_info info;
  BowLayout lay;
  if (int rc = bow_parse((const uint8_t*)bytes, n_bytes, &info, &lay)) return fail(c, rc, "%s: %s", who, info.message);
  int passes = 1;  // the keys are 0..words, `words` the stopped descriptors' key
  while (passes < kRadixMaxPasses && ((uint64_t)info.words >> (passes * kRadixMaxBits))) passes++;
  HIPCHK(c, hipSetDevice(c->dev));
  hipStream_t s = cur_stream(c);
  HIPCHK(c, hipStreamSynchronize(s));
  B.has_voc = false;
  const size_t nn = (size_t)info.nodes + 1;
  if (int rc = B.node_desc.alloc(c, nn * 2)) return rc;
  if (int rc = B.kids.alloc(c, nn)) return rc;
  if (int rc = B.node_word.alloc(c, nn)) return rc;
  if (int rc = B.node_weight.alloc(c, nn)) return rc;
  if (int rc = B.word_weight.alloc(c, (size_t)info.words)) return rc;
  HIPCHK(c, hipMemcpyAsync(B.node_desc, lay.desc.data(), nn * 32, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(B.kids, lay.kids.data(), nn * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(B.node_word, lay.word.data(), nn * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(B.node_weight, lay.weight.data(), nn * 8, hipMemcpyHostToDevice, s));
  if (info.words) HIPCHK(c, hipMemcpyAsync(B.word_weight, lay.word_weight.data(), (size_t)info.words * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));
  B.info = info, B.passes = passes, B.q_n = 0, B.has_voc = true;
  return 0;
}

int esvio_fe_bow_transform(esvio_fe_handle c, const uint32_t* desc, int n, int space, int32_t* word, double* weight,
                           uint32_t* bow_word, double* bow_value, int32_t bow_cap, int32_t* n_bow) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_transform";
  KfAllocs allocs(c);
  if (n_bow) *n_bow = 0;
  if (int rc = bow_desc_check(c, who, desc, n, space)) return rc;
  if (bow_cap < 0 || (bow_cap > 0 && (!bow_word || !bow_value || !n_bow)))
    return fail(c, ESVIO_FE_EINVAL, "%s: bow_cap %d without bow_word, bow_value and n_bow", who, bow_cap);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_transform_run(c, desc, n, space)) return rc;
  Bow& B = c->bow;
  hipStream_t s = cur_stream(c);
  const size_t k = std::min<size_t>(B.q_n, (size_t)bow_cap);
  if (n && word) HIPCHK(c, hipMemcpyAsync(word, B.word, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (n && weight) HIPCHK(c, hipMemcpyAsync(weight, B.weight, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  if (k) {
    HIPCHK(c, hipMemcpyAsync(bow_word, B.q_word, k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(bow_value, B.q_val, k * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  if (n_bow) *n_bow = (int32_t)B.q_n;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_add(esvio_fe_handle c, const uint32_t* desc, int n, int space, int32_t* entry_id) {
  if (!c) return ESVIO_FE_EINVAL;
  KfAllocs allocs(c);
  if (int rc = bow_desc_check(c, "bow_add", desc, n, space)) return rc;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_transform_run(c, desc, n, space)) return rc;
  if (int rc = bow_add_run(c, entry_id)) return rc;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_query(esvio_fe_handle c, const uint32_t* desc, int n, int space, int max_results, int max_id,
                       esvio_fe_bow_result* results, int32_t* n_results) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_query";
  KfAllocs allocs(c);
  if (n_results) *n_results = 0;
  if (int rc = bow_desc_check(c, who, desc, n, space)) return rc;
  if (max_results < 1 || max_results > kBowMaxResults)
    return fail(c, ESVIO_FE_EINVAL, "%s: max_results must be in 1..%d (got %d; the \"all results\" form is not built)", who, kBowMaxResults, max_results);
  if (!results || !n_results) return fail(c, ESVIO_FE_EINVAL, "%s: results or n_results is null", who);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_query_room(c)) return rc;
  if (int rc = bow_transform_run(c, desc, n, space)) return rc;
  if (int rc = bow_score_enqueue(c, max_id)) return rc;
  if (int rc = bow_select_run(c, max_results, results, n_results)) return rc;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_scores(esvio_fe_handle c, const uint32_t* desc, int n, int space, int max_id, double* score, uint8_t* present) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_scores";
  KfAllocs allocs(c);
  if (int rc = bow_desc_check(c, who, desc, n, space)) return rc;
  Bow& B = c->bow;
  const uint32_t N = bow_entries(B);
  if (N && (!score || !present)) return fail(c, ESVIO_FE_EINVAL, "%s: score or present is null with %u entries", who, N);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_query_room(c)) return rc;
  if (int rc = bow_transform_run(c, desc, n, space)) return rc;
  if (!N) return 0;
  if (int rc = bow_score_enqueue(c, max_id)) return rc;
  hipStream_t s = cur_stream(c);
  HIPCHK(c, hipMemcpyAsync(score, B.score, (size_t)N * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(present, B.present, (size_t)N, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_detect_loop(esvio_fe_handle c, const uint32_t* desc, int n, int space, int frame_index, int32_t* loop_index,
                             esvio_fe_bow_result* results, int32_t* n_results) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_detect_loop";
  KfAllocs allocs(c);
  if (n_results) *n_results = 0;
  if (loop_index) *loop_index = -1;
  if (int rc = bow_desc_check(c, who, desc, n, space)) return rc;
  if (!loop_index) return fail(c, ESVIO_FE_EINVAL, "%s: loop_index is null", who);
  if (frame_index < 0) return fail(c, ESVIO_FE_EINVAL, "%s: frame_index must not be negative (got %d)", who, frame_index);
  if ((results == nullptr) != (n_results == nullptr)) return fail(c, ESVIO_FE_EINVAL, "%s: results and n_results go together", who);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_query_room(c)) return rc;
  if (int rc = bow_transform_run(c, desc, n, space)) return rc;  // once, for the query and the add
  esvio_fe_bow_result R[ESVIO_FE_BOW_LOOP_RESULTS];
  int32_t nr = 0;
  if (int rc = bow_score_enqueue(c, frame_index - ESVIO_FE_BOW_LOOP_GAP)) return rc;
  if (int rc = bow_select_run(c, ESVIO_FE_BOW_LOOP_RESULTS, R, &nr)) return rc;
  if (int rc = bow_add_run(c, nullptr)) return rc;
  // pose_graph.cpp:377-404
  bool find = false;
  if (nr >= 1 && R[0].score > ESVIO_FE_BOW_LOOP_MIN_FIRST)
    for (int i = 1; i < nr; i++)
      if (R[i].score > ESVIO_FE_BOW_LOOP_MIN_OTHER) find = true;
  int32_t m = -1;
  if (find && frame_index > ESVIO_FE_BOW_LOOP_GAP)
    for (int i = 0; i < nr; i++)
      if (m == -1 || (R[i].id < m && R[i].score > ESVIO_FE_BOW_LOOP_MIN_OTHER)) m = R[i].id;
  *loop_index = m;
  if (results) {
    for (int i = 0; i < nr; i++) results[i] = R[i];
    *n_results = nr;
  }
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_bow_clear(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = bow_ready(c, "bow_clear")) return rc;
  c->bow.off.assign(1, 0);  // (every call has waited for its own work: nothing reads the pools)
  return 0;
}
int esvio_fe_bow_entries(esvio_fe_handle c) { return c ? (int)bow_entries(c->bow) : ESVIO_FE_EINVAL; }
int esvio_fe_bow_reserve(esvio_fe_handle c, int64_t entries, int64_t words) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "bow_reserve";
  KfAllocs allocs(c);
  if (int rc = bow_ready(c, who)) return rc;
  if (entries < 0 || entries > 0x7ffffffe || words < 0 || words > ((int64_t)1 << 40))
    return fail(c, ESVIO_FE_EINVAL, "%s: entries must be in 0..2^31-2 and words in 0..2^40 (got %lld, %lld)", who, (long long)entries, (long long)words);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = bow_room(c, (size_t)entries, (size_t)words, false)) return rc;
  if (!c->bow.res_id) {
    Bow& B = c->bow;
    if (int rc = B.res_id.alloc(c, kBowMaxResults)) return rc;
    if (int rc = B.res_score.alloc(c, kBowMaxResults)) return rc;
    if (int rc = B.res_raw.alloc(c, kBowMaxResults)) return rc;
  }
  return 0;
}

}  // extern "C"
