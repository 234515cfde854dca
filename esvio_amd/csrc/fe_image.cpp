// fe_image.cpp — the image front-end: FeatureTracker::trackImage
// (feature_tracker.cpp:164-338) and cv::goodFeaturesToTrack on the kernels of fe_kernels.hip.
#include "fe_internal.h"

namespace esvio {
namespace fe {

// ================================================================ image front-end
// half-widths of the open Euclidean disc dx*dx + dy*dy < md*md (goodFeaturesToTrack's distance test)
void euclid_halfwidths(double md, int8_t* hw /*[kMaxDiscR+1]*/, int* radius) {
  const double md2 = md * md;
  *radius = 0;
  for (int dy = 0; dy <= kMaxDiscR; dy++) {
    int w = -1;
    for (int dx = 0; dx <= kMaxDiscR; dx++)
      if ((double)dx * dx + (double)dy * dy < md2) w = dx;
    hw[dy] = (int8_t)w;
    if (w >= 0) *radius = dy;
  }
}

// What every FAST pass starts with, on the current stream: the score map of the W x H image at `img` (in fc.m), the
// per-block lists of `cs` — positions in xy, scores in idx — with the counts before them in fc.det, and the lists'
// compaction.  skip_center: FastArgs::skip_center.  n_detected (device, may be null): where the sum of fc.det goes.
static void fast_lists(esvio_fe_ctx* c, const uint8_t* img, int stride, int arc, int barrier, bool nonmax, int skip_center,
                       const esvio_fe_ctx::CandSet& cs, const esvio_fe_ctx::FastCand& fc, uint32_t* n_detected) {
  const size_t P = (size_t)c->W * c->H;
  hipStream_t s = cur_stream(c);
  FastArgs a{};
  a.img = img;
  a.stride = stride;
  a.W = c->W;
  a.H = c->H;
  a.arc = arc;
  a.barrier = barrier;
  a.nonmax = nonmax ? 1 : 0;
  a.m = fc.m;
  a.cand_xy = cs.xy;
  a.cand_score = cs.idx;
  a.cand_cnt = cs.cnt;
  a.det_cnt = fc.det;
  a.n_detected = n_detected;
  a.skip_center = skip_center;
  {
    ScopedKernel k(c, K_FAST_SCORE, 2 * P);  // the image read once, the map written
    launch_fast_score(s, a);
  }
  {
    ScopedKernel k(c, K_FAST_COLLECT, P);
    launch_fast_collect(s, a);
  }
  compact_set(c, cs, (uint32_t)((P + kArcBlock - 1) / kArcBlock), true);
}

// the score map and the per-block counts before non-max: what fast_lists needs of a FastCand
static int fast_map_alloc(esvio_fe_ctx* c, esvio_fe_ctx::FastCand& f) {
  if (f.det) return 0;  // (the last one: "all of them")
  const size_t P = (size_t)c->W * c->H;
  if (int rc = f.m.alloc(c, P)) return rc;
  return f.det.alloc(c, (P + kArcBlock - 1) / kArcBlock);
}

// esvio_fe_fast_corners' candidate set and score map (esvio_fe_ctx::fast_own, fast_own_fc), on the first call
static int fast_own_alloc(esvio_fe_ctx* c) {
  if (c->fast_own.cap) return 0;
  if (int rc = fast_map_alloc(c, c->fast_own_fc)) return rc;
  // total[0]: k_compact's total; total[1]: the count before non-max — side by side, one copy for both
  return cand_set_alloc(c, c->fast_own, ((size_t)c->W * c->H + kArcBlock - 1) / kArcBlock * kArcBlock, 2);
}

// fast::fast_corner_detect_9 / _10 (+ fast_corner_score_10, fast_nonmax_3x3) of the reference's vendored FAST
// (dependences/fast_neon-master/include/fast/fast.h:22-47) on a device image.  A candidate set and a score map of
// its own (fast_own, fast_own_fc), allocated on the first call: nothing the tracker, a prefetched batch or the stage
// tap uses is touched.
int fast_run(esvio_fe_ctx* c, const uint8_t* img, int stride, int arc, int barrier, bool nonmax, int16_t* out_xy,
             int32_t* out_score, int32_t capacity, int32_t* n_out, int32_t* n_detected) {
  esvio_fe_ctx::CandSet& cs = c->fast_own;
  if (int rc = fast_own_alloc(c)) return rc;
  hipStream_t s = cur_stream(c);
  // (without non-max the count before it is the total)
  fast_lists(c, img, stride, arc, barrier, nonmax, -1, cs, c->fast_own_fc, (n_detected && nonmax) ? cs.total + 1 : nullptr);
  uint32_t tot[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(tot, cs.total, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  const size_t k = std::min<size_t>(tot[0], capacity > 0 ? (size_t)capacity : 0);
  if (k && out_xy) HIPCHK(c, hipMemcpyAsync(out_xy, cs.comp_xy, k * 4, hipMemcpyDeviceToHost, s));  // x | y<<16 = int16 x, y
  if (k && out_score) HIPCHK(c, hipMemcpyAsync(out_score, cs.comp_idx, k * 4, hipMemcpyDeviceToHost, s));
  if (k) HIPCHK(c, hipStreamSynchronize(s));
  *n_out = (int32_t)tot[0];
  if (n_detected) *n_detected = (int32_t)(nonmax ? tot[1] : tot[0]);
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// cv::FAST(image, keypoints, threshold, true) as include/esvio_fe.h "keyframes" states it (rule F), for
// esvio_fe_kf_fast / esvio_fe_kf_describe: arc 9, the score, the strict 3x3 non-max, on the kernels and in the scratch
// of fast_run above.  The whole list comes to the host (xy[i] = x | y << 16 in raster order, score[i]): a corner of
// score 0 — possible at threshold 0 only — is not greater than the 0 of a pixel that is no corner and is dropped here,
// which k_fast_collect's map of score + 1 cannot say.  Synchronises the stream.
int fast_keyframe_run(esvio_fe_ctx* c, const uint8_t* img, int stride, int threshold, std::vector<uint32_t>& xy,
                      std::vector<uint32_t>& score, int32_t* n_detected) {
  esvio_fe_ctx::CandSet& cs = c->fast_own;
  if (int rc = fast_own_alloc(c)) return rc;
  hipStream_t s = cur_stream(c);
  fast_lists(c, img, stride, 9, threshold, true, -1, cs, c->fast_own_fc, cs.total + 1);
  uint32_t tot[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(tot, cs.total, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (tot[0] > cs.cap) return fail(c, ESVIO_FE_EINTERNAL, "kf_fast: %u corners in a set of %zu", tot[0], cs.cap);
  xy.resize(tot[0]);
  score.resize(tot[0]);
  if (tot[0]) {
    HIPCHK(c, hipMemcpyAsync(xy.data(), cs.comp_xy, (size_t)tot[0] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(score.data(), cs.comp_idx, (size_t)tot[0] * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  if (threshold == 0) {
    size_t k = 0;
    for (size_t i = 0; i < xy.size(); i++)
      if (score[i]) xy[k] = xy[i], score[k++] = score[i];
    xy.resize(k);
    score.resize(k);
  }
  if (n_detected) *n_detected = (int32_t)tot[1];
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// ---- ESVIO_FE_DETECT_FAST: FAST as trackEvent's detector (include/esvio_fe.h: esvio_fe_set_detector)
// The survivors of a 3x3 non-max with ">=" are never 8-neighbours of each other: one per 2 x 2 pixels at most.
static uint32_t fast_cand_max(const esvio_fe_ctx* c) { return (uint32_t)((c->W + 1) / 2) * (uint32_t)((c->H + 1) / 2); }

static int fast_scratch_alloc(esvio_fe_ctx* c, esvio_fe_ctx::FastCand& f) {
  if (f.hist) return 0;  // (the last one: "all of them")
  const size_t n_max = fast_cand_max(c);
  if (int rc = fast_map_alloc(c, f)) return rc;
  if (int rc = f.tot.alloc(c, 1)) return rc;
  if (int rc = f.keys.alloc(c, n_max)) return rc;
  if (int rc = f.vals.alloc(c, n_max)) return rc;
  return f.hist.alloc(c, sort_scratch_words(n_max));
}

// the stage tap's: its scratch, its candidate set (one entry per pixel), the device copy of a caller's host image
int ensure_fast_tap(esvio_fe_ctx* c) {
  if (c->fast_tap.cap) return 0;
  const size_t P = (size_t)c->W * c->H;
  if (int rc = fast_scratch_alloc(c, c->fastc[kRightSlots])) return rc;
  if (int rc = c->d_fast_tap_img.alloc(c, P)) return rc;
  return cand_set_alloc(c, c->fast_tap, (P + kArcBlock - 1) / kArcBlock * kArcBlock);
}

// ... and the tracker's: the per-block lists of a pass are its candidate set's own (cand[set].xy / idx / cnt), one
// entry per pixel.  (Growing a set frees it: the caller has made sure that nothing is in flight.)
int ensure_fast_detector(esvio_fe_ctx* c) {
  for (int k = 0; k < kRightSlots; k++) {
    if (int rc = ensure_cand_capacity(c, k, (size_t)c->W * c->H)) return rc;
    if (int rc = fast_scratch_alloc(c, c->fastc[k])) return rc;
  }
  return ensure_fast_tap(c);
}

int fast_cand_pass(esvio_fe_ctx* c, const uint8_t* img, int stride, int barrier, const esvio_fe_ctx::CandSet& cs,
                   const esvio_fe_ctx::FastCand& fc, bool want_count) {
  const uint32_t n_max = fast_cand_max(c);
  const double thr = c->cfg.ts_lk_threshold;
  hipStream_t s = cur_stream(c);
  const int skip_center = thr >= 0 && thr < 256 ? (int)(uint8_t)thr : 256;  // (a byte that no pixel has: nobody is left out)
  fast_lists(c, img, stride, 10, barrier, true, skip_center, cs, fc, want_count ? fc.tot.p : nullptr);
  // raster order -> by score, descending: keys + one stable 8-bit pass, booked together as one k_radix_pass entry.
  // The count stays on the device (cs.total): both launches are sized for n_max.  The pass writes the set's own
  // lists: comp_xy = the positions, comp_idx = the keys (score in bits 8..15), which the selection hands through.
  const SortScratch sc = sort_scratch(fc.hist);
  ScopedKernel k(c, K_RADIX_PASS, 0);
  HIPCHK(c, hipMemsetAsync(fc.hist, 0, (size_t)sc.head_words * 4, s));
  launch_fast_keys(s, cs.comp_xy, cs.comp_idx, cs.total, n_max, fc.keys, fc.vals, sc.ghist, sc.lookback);
  radix_sort_pairs(c, SortBufs{{fc.keys, cs.comp_idx}, {fc.vals, cs.comp_xy}, fc.hist, cs.total}, n_max, 1, 8, false);
  return 0;
}

int run_fast_cand(esvio_fe_ctx* c, const PyrDesc& ts, int set) {
  return fast_cand_pass(c, px00(ts), ts.stride[0], c->fast_barrier, c->cand[set], c->fastc[set], false);
}

// cv::goodFeaturesToTrack on the level-0 image of pyramid `d` (padded, so no border arithmetic);
// up to max_corners corners are written at out_pts[out_base ..], counts mirrored to host_counts.
// `use_mask`: d_mask_bits holds the blocked pixels.  Synchronises the stream once (the number of
// local maxima sizes the sort).
int gftt_run(esvio_fe_ctx* c, const PyrDesc& d, int max_corners, double quality, double min_distance,
             bool use_mask, float2* out_pts, int out_base, int* host_counts) {
  const size_t P = (size_t)c->W * c->H;
  if (!c->d_gftt_max) {  // (the last one: "all of them")
    if (int rc = c->d_gftt_cov.alloc(c, P)) return rc;
    if (int rc = c->d_gftt_rowsum.alloc(c, P)) return rc;
    if (int rc = c->d_gftt_eig.alloc(c, P)) return rc;
    if (int rc = c->d_gftt_max.alloc(c, 1)) return rc;
  }
  const int set = c->cand_cur;
  if (int rc = ensure_cand_capacity(c, set, P)) return rc;
  const esvio_fe_ctx::CandSet& cs = c->cand[set];
  GfttArgs g{};
  g.img = px00(d);
  g.stride = d.stride[0];
  g.W = c->W;
  g.H = c->H;
  g.cov = c->d_gftt_cov;
  g.rowsum = c->d_gftt_rowsum;
  g.eig = c->d_gftt_eig;
  g.mask_bits = use_mask ? c->d_mask_bits.p : nullptr;
  g.wpr = (c->W + 31) / 32;
  g.max_key = c->d_gftt_max;
  g.quality = quality;
  g.cand_xy = cs.xy;
  g.cand_val = cs.idx;
  g.cand_cnt = cs.cnt;
  launch_gftt_response(cur_stream(c), g);
  launch_gftt_collect(cur_stream(c), g);
  compact_set(c, cs, (uint32_t)((P + kArcBlock - 1) / kArcBlock), false);
  uint32_t n = 0;
  HIPCHK(c, hipMemcpyAsync(&n, cs.total, 4, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  const uint32_t* sorted_xy = cs.comp_xy;
  if (n > 1) {  // by response, then address, both descending: 4 x 8-bit stable radix passes
    if (int rc = ensure_sort_capacity(c, n)) return rc;
    const SortScratch sc = sort_scratch(c->hist);
    HIPCHK(c, hipMemsetAsync(c->hist, 0, (size_t)sc.head_words * 4, cur_stream(c)));
    launch_gftt_sortprep(cur_stream(c), cs.comp_xy, cs.comp_idx, n, c->keys[0], c->vals[0], sc.ghist, sc.lookback,
                         4u * (radix_blocks(n) << 8));
    const int cur = radix_sort_pairs(c, n, 4, 8, false);
    HIPCHK(c, hipMemsetAsync(c->hist, 0, (size_t)sc.head_words * 4, cur_stream(c)));  // as k_sae_apply leaves it
    sorted_xy = c->vals[cur];
  }
  // the sorted list (positions only), the open Euclidean disc of min_distance, the counts mirrored to the host
  SelectArgs sa = make_select_args(c, set, max_corners, out_pts, out_base, nullptr);
  sa.comp_xy = sa.comp_idx = sorted_xy;
  euclid_halfwidths(min_distance, sa.hw, &sa.radius);
  sa.disc_c = disc_threshold(sa.hw, sa.radius);
  sa.host_counts = host_counts;
  launch_select_args(c, sa);
  return 0;
}

// Image_setMask (feature_tracker.cpp:90-119, FISHEYE 0): like Event_setMask on a CV_8UC1 mask;
// c->mask_event then holds the BLOCKED pixels (the reference's mask_image == 0)
void image_set_mask(esvio_fe_ctx* c) {
  c->mask_event.reset(c->W, c->H);
  std::vector<std::pair<int, std::pair<P2f, int>>> cnt_pts_id;
  cnt_pts_id.reserve(c->cur_pts.size());
  for (unsigned int i = 0; i < c->cur_pts.size(); i++)
    cnt_pts_id.push_back(std::make_pair(c->track_cnt[i], std::make_pair(c->cur_pts[i], c->ids[i])));
  std::sort(cnt_pts_id.begin(), cnt_pts_id.end(),
            [](const std::pair<int, std::pair<P2f, int>>& a,
               const std::pair<int, std::pair<P2f, int>>& b) { return a.first > b.first; });
  c->cur_pts.clear();
  c->ids.clear();
  c->track_cnt.clear();
  for (auto& it : cnt_pts_id) {
    const int px = host::cv_round(it.second.first.x), py = host::cv_round(it.second.first.y);
    if (px < 0 || px >= c->W || py < 0 || py >= c->H) continue;  // cannot happen after inBorder
    if (!c->mask_event.test(px, py)) {
      c->cur_pts.push_back(it.second.first);
      c->ids.push_back(it.second.second);
      c->track_cnt.push_back(it.first);
      c->mask_event.stamp_disc(px, py, c->cfg.min_dist, c->hw);
    }
  }
}

// FeatureTracker::trackImage (feature_tracker.cpp:164-338) for a handle whose width/height/max_cnt/
// min_dist are the image camera's COL/ROW/MAX_CNT_IMG/MIN_DIST_IMG.  cfg.equalize applies the
// node's CLAHE (stereo_image_tracker_node.cpp:92-96, no normalisation) to both images first.
// No pipelining here: one frame at a time on the main stream.
int track_image_impl(esvio_fe_ctx* c, double _cur_time, const uint8_t* img_left,
                     const uint8_t* img_right, bool PUB_THIS_FRAME, int space) {
  const esvio_fe_config& cfg = c->cfg;
  const int M = cfg.max_cnt;
  if (int rc = finalize_lazy(c)) return rc;  // (a lazy trackEvent call came before)
  if (int rc = cancel_chain(c)) return rc;
  const ResView &pin = c->pin[0], &zpin = c->zpin[0];
  c->cur_time = _cur_time;
  const bool first = !c->have_img;
  const bool have_right = img_right != nullptr;
  rotate_slots(c, false);  // as in trackEvent's plain path
  const PyrDesc& L = c->pyr[c->slot_curL].d;
  const PyrDesc& R = c->pyr[c->slot_curR].d;
  if (cfg.equalize) {
    const PyrDesc& rl = c->raw[c->raw_cur][0].d;
    const PyrDesc& rr = c->raw[c->raw_cur][1].d;
    if (int rc = copy_level0_in(c, rl, img_left, space)) return rc;
    if (have_right)
      if (int rc = copy_level0_in(c, rr, img_right, space)) return rc;
    run_clahe(c, px00(rl), have_right ? px00(rr) : px00(rl), rl.stride[0], px00(L), have_right ? px00(R) : px00(L),
              L.stride[0], have_right ? 2 : 1, 2, 0);
  } else {
    if (int rc = copy_level0_in(c, L, img_left, space)) return rc;
    if (have_right)
      if (int rc = copy_level0_in(c, R, img_right, space)) return rc;
  }
  {
    PyrDesc two[2] = {L, R};
    pyr_build(c, two, have_right ? 2 : 1);
  }
  if (first) c->slot_prevL = c->slot_curL;
  c->have_img = true;
  const PyrDesc& prevL = c->pyr[c->slot_prevL].d;
  c->cur_pts.clear();

  if (c->prev_pts.size() > 0) {  // :180-209: forward, and backward with maxLevel 3 / no initial flow
    const int n = (int)c->prev_pts.size();
    std::memcpy(pin.A, c->prev_pts.data(), (size_t)n * 8);
    run_lk_pair(c, lk_pair(prevL, L, zpin.A, nullptr, n, kLkStereo, zpin.s1));
    HIPCHK(c, sync_main(c));
    const LkOut& r = pin.s1;
    std::vector<uint8_t> status(r.st_fwd, r.st_fwd + n);
    c->cur_pts.assign(r.fwd, r.fwd + n);
    if (cfg.flow_back)
      for (int i = 0; i < n; i++)
        status[i] = status[i] && r.st_back[i] && pt_distance(c->prev_pts[i], r.back[i]) <= 0.5;
    for (int i = 0; i < n; i++)
      if (status[i] && !in_border_event(c, c->cur_pts[i])) status[i] = 0;
    reduce_vector(c->prev_pts, status);
    reduce_vector(c->cur_pts, status);
    reduce_vector(c->ids, status);
    reduce_vector(c->track_cnt, status);
  }
  for (auto& n : c->track_cnt) n++;

  if (PUB_THIS_FRAME) {  // :214-241
    image_set_mask(c);
    const int n_max_cnt = M - (int)c->cur_pts.size();
    c->n_pts.clear();
    if (n_max_cnt > 0) {
      std::memcpy(pin.mask, c->mask_event.bits.data(), c->mask_event.bits.size() * 4);
      HIPCHK(c, hipMemcpyAsync(c->d_mask_bits, pin.mask, c->mask_event.bits.size() * 4,
                               hipMemcpyHostToDevice, cur_stream(c)));
      if (int rc = gftt_run(c, L, n_max_cnt, 0.01, (double)cfg.min_dist, true, (float2*)zpin.news, 0, zpin.counts))
        return rc;
      HIPCHK(c, sync_main(c));
      if (int rc = lookback_expired(c)) return rc;
      c->n_pts.assign(pin.news, pin.news + pin.counts[0]);
    }
    for (auto& p : c->n_pts) {
      c->cur_pts.push_back(p);
      c->ids.push_back(c->n_id++);
      c->track_cnt.push_back(1);
    }
  }
  c->cur_un_pts = undistorted_pts(c->cur_pts, cfg.cam[0]);
  c->pts_velocity = pts_velocity_fn(c->ids, c->cur_un_pts, c->cur_un_pts_map, c->prev_un_pts_map,
                                    c->cur_time - c->prev_time, c->cur_pts.size());

  if (have_right) {  // :249-318
    c->ids_right.clear();
    c->cur_right_pts.clear();
    c->cur_un_right_pts.clear();
    c->right_pts_velocity.clear();
    c->cur_un_right_pts_map.clear();
    c->track_cnt_right.clear();
    if (!c->cur_pts.empty()) {
      const int n = (int)c->cur_pts.size();
      std::memcpy(pin.A, c->cur_pts.data(), (size_t)n * 8);
      run_lk_pair(c, lk_pair(L, R, zpin.A, nullptr, n, kLkStereo, zpin.s1));
      HIPCHK(c, sync_main(c));
      const LkOut& r = pin.s1;
      std::vector<uint8_t> status(r.st_fwd, r.st_fwd + n);
      c->cur_right_pts.assign(r.fwd, r.fwd + n);
      if (cfg.flow_back)
        for (int i = 0; i < n; i++)
          status[i] = status[i] && r.st_back[i] && in_border_event(c, c->cur_right_pts[i]) &&
                      pt_distance(c->cur_pts[i], r.back[i]) <= 0.5;
      c->ids_right = c->ids;
      reduce_vector(c->cur_right_pts, status);
      reduce_vector(c->ids_right, status);
      c->cur_un_right_pts = undistorted_pts(c->cur_right_pts, cfg.cam[1]);
      c->right_pts_velocity =
          pts_velocity_fn(c->ids_right, c->cur_un_right_pts, c->cur_un_right_pts_map,
                          c->prev_un_right_pts_map, c->cur_time - c->prev_time, c->cur_pts.size());
    }
    c->prev_un_right_pts_map.swap(c->cur_un_right_pts_map);
  }
  c->slot_prevL = c->slot_curL;
  c->prev_pts = c->cur_pts;
  c->prev_un_pts_map.swap(c->cur_un_pts_map);
  c->prev_time = c->cur_time;
  if (c->prof_on) resolve_profile(c);
  return 0;
}


}  // namespace fe
}  // namespace esvio
