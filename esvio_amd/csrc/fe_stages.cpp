// fe_stages.cpp — device memory and the per-stage launches of the event front-end, plus the host
// bookkeeping helpers the reference keeps on the CPU (feature_tracker.cpp:48-151,910-1045).
// Every data-parallel stage is a HIP kernel from fe_kernels.hip; there is no CPU fallback.
#include "fe_internal.h"

#include <optional>

namespace esvio {
namespace fe {

// ---------------------------------------------------------------- memory

int ensure_event_capacity(esvio_fe_ctx* c, size_t n) { return c->d_ev.grow(c, n); }

// keys, vals and sae_marks share one capacity (sort_cap: set once all five are there)
static int grow_sort_buffers(esvio_fe_ctx* c, size_t cap) {
  c->sort_cap = 0;
  for (int i = 0; i < 2; i++) {
    c->keys[i].release();
    c->vals[i].release();
  }
  for (int i = 0; i < 2; i++) {
    if (int rc = c->keys[i].alloc(c, cap)) return rc;
    if (int rc = c->vals[i].alloc(c, cap)) return rc;
  }
  if (int rc = c->sae_marks.alloc(c, cap)) return rc;
  c->sort_cap = cap;
  return 0;
}

int ensure_sort_capacity(esvio_fe_ctx* c, size_t n) {
  if (n > c->sort_cap)
    if (int rc = grow_sort_buffers(c, std::max<size_t>(n + n / 4, 1 << 16))) return rc;
  const size_t hneed = sort_scratch_words(c->sort_cap);
  if (hneed > c->hist.cap) {
    if (int rc = c->hist.alloc(c, hneed)) return rc;
    const hipError_t zeroed = hipMemsetAsync(c->hist, 0, hneed * 4, cur_stream(c));
    if (zeroed != hipSuccess) c->hist.release();  // (not zeroed is not there)
    HIPCHK(c, zeroed);
  }
  return 0;
}

// the seven arrays of a candidate set share one capacity (cap: set once all of them are there)
int cand_set_alloc(esvio_fe_ctx* c, esvio_fe_ctx::CandSet& s, size_t cap, size_t total_words) {
  s = esvio_fe_ctx::CandSet();
  if (int rc = s.xy.alloc(c, cap)) return rc;
  if (int rc = s.idx.alloc(c, cap)) return rc;
  if (int rc = s.cnt.alloc(c, cap / kArcBlock)) return rc;
  if (int rc = s.grp.alloc(c, cap / kArcBlock / 64 + 2)) return rc;
  if (int rc = s.comp_xy.alloc(c, cap)) return rc;
  if (int rc = s.comp_idx.alloc(c, cap)) return rc;
  if (int rc = s.total.alloc(c, total_words)) return rc;
  s.cap = cap;
  return 0;
}
static int grow_cand_set(esvio_fe_ctx* c, int set, size_t cap) { return cand_set_alloc(c, c->cand[set], cap); }

int ensure_cand_capacity(esvio_fe_ctx* c, int set, size_t n) {
  if (n <= c->cand[set].cap) return 0;
  size_t cap = std::max<size_t>(n + n / 4, 1 << 16);
  cap = (cap + kArcBlock - 1) / kArcBlock * kArcBlock;
  if (int rc = grow_cand_set(c, set, cap)) return rc;
  // the sets that have never been used get the same size now: in replay mode the Arc* passes rotate
  // through them, and each one's first use would otherwise put seven hipMallocs into some later call
  // (a set that holds candidates is left alone: only its own Arc* pass may replace it)
  for (int k = 0; k < kRightSlots; k++)
    if (k != set && c->cand[k].cap == 0)
      if (int rc = grow_cand_set(c, k, cap)) return rc;
  return 0;
}

// per-event flags (standalone isCorner) and candidate set `set`
int ensure_arc_capacity(esvio_fe_ctx* c, size_t n, int set) {
  if (int rc = ensure_cand_capacity(c, set, n)) return rc;
  if (n <= c->d_flags.cap) return 0;
  const size_t cap = std::max<size_t>(n + n / 4, 1 << 16);
  return c->d_flags.alloc(c, (cap + kArcBlock - 1) / kArcBlock * kArcBlock);
}

int pyr_alloc(esvio_fe_ctx* c, PyrStore& ps, int w, int h, int max_level) {
  if (ps.mem && ps.w == w && ps.h == h && ps.max_level == max_level) return 0;
  ps = PyrStore();
  const int levels = pyr_levels(w, h, kLkWin, max_level);
  size_t off = 0, img_off[kMaxLevels], der_off[kMaxLevels];
  int lw = w, lh = h;
  for (int l = 0; l <= levels; l++) {
    ps.d.stride[l] = pyr_stride(lw);
    const size_t area = (size_t)ps.d.stride[l] * (lh + 2 * kPad);
    img_off[l] = off;
    off += (area + 255) / 256 * 256;
    der_off[l] = off;
    off += (area * 4 + 255) / 256 * 256;
    ps.d.w[l] = lw;
    ps.d.h[l] = lh;
    lw = (lw + 1) / 2;
    lh = (lh + 1) / 2;
  }
  if (int rc = ps.mem.alloc(c, off)) return rc;
  HIPCHK(c, hipMemsetAsync(ps.mem, 0, off, cur_stream(c)));  // derivative borders stay 0 forever
  for (int l = 0; l <= levels; l++) {
    ps.d.img[l] = ps.mem + img_off[l];
    ps.d.deriv[l] = (int16_t*)(ps.mem + der_off[l]);
  }
  for (int l = levels + 1; l < kMaxLevels; l++) {
    ps.d.img[l] = ps.d.img[levels];
    ps.d.deriv[l] = ps.d.deriv[levels];
    ps.d.w[l] = ps.d.w[levels];
    ps.d.h[l] = ps.d.h[levels];
    ps.d.stride[l] = ps.d.stride[levels];
  }
  ps.d.levels = levels;
  ps.w = w;
  ps.h = h;
  ps.max_level = max_level;
  return 0;
}

uint64_t pyr_pixels(const PyrDesc& d) {
  uint64_t px = 0;
  for (int l = 0; l <= d.levels; l++) px += (uint64_t)d.w[l] * d.h[l];
  return px;
}

// level 0 interior already written -> pyrDown chain, border fill, Scharr
void pyr_build(esvio_fe_ctx* c, const PyrDesc* p, int nimg) {
  for (int l = 0; l < p[0].levels; l++) {
    uint64_t src = (uint64_t)p[0].w[l] * p[0].h[l], dst = (uint64_t)p[0].w[l + 1] * p[0].h[l + 1];
    ScopedKernel k(c, K_PYR_DOWN, (src + dst) * nimg);
    launch_pyr_down(cur_stream(c), p, nimg, l);
  }
  {
    ScopedKernel k(c, K_PYR_PAD, 0);
    launch_pyr_pad(cur_stream(c), p, nimg);
  }
  {
    ScopedKernel k(c, K_SCHARR, pyr_pixels(p[0]) * 5 * nimg);  // 1 B read + 4 B written per pixel
    launch_scharr(cur_stream(c), p, nimg);
  }
}

// ---------------------------------------------------------------- SAE update (both cameras)
// Motion_correction_value -> kernel parameters (the kernels take t_0, the first left event's time,
// feature_tracker.cpp:621, from the batch itself: no host copy of an event for a device batch)
McParams make_mc_params(const esvio_fe_motion* m) {
  McParams p;
  std::memset(&p, 0, sizeof(p));
  p.enabled = 1;
  p.t1 = m->t1;
  const double an = std::sqrt(std::pow((double)m->accel[0], 2) + std::pow((double)m->accel[1], 2) +
                              std::pow((double)m->accel[2], 2));
  p.active = an > 5;  // a_motion_compensation_threshold (event_detector.h:51)
  for (int i = 0; i < 3; i++) {
    p.vsum[i] = (float)m->v[i] + m->v_pre[i];
    p.omega[i] = m->omega[i];
  }
  M3f K;
  std::memset(&K, 0, sizeof(K));
  K.m[0][0] = (float)m->fx;
  K.m[0][2] = (float)m->cx;
  K.m[1][1] = (float)m->fy;
  K.m[1][2] = (float)m->cy;
  K.m[2][2] = 1.f;
  p.K = K;
  p.Kinv = mc_inverse(K);
  return p;
}

// the partition's buffers for batches of up to n events (d_warp only once a motion-compensated batch comes)
int ensure_part_capacity(esvio_fe_ctx* c, size_t n, bool mc) {
  if (n > c->d_part.cap) {
    c->d_warp.release();  // (sized like d_part)
    if (int rc = c->d_part.grow(c, n)) return rc;
  }
  if (mc && !c->d_warp)  // the motion-compensated overload: 4 B per event for the warped pixels
    if (int rc = c->d_warp.alloc(c, c->d_part.cap)) return rc;
  const size_t need = tile_scratch_words(c->d_part.cap);
  if (need > c->d_tile.cap)
    if (int rc = c->d_tile.alloc(c, need)) return rc;
  return 0;
}

int sae_update_tiled(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
                     double2* L2, double2* S2, uint8_t* arc_touched, const McParams* mc) {
  const uint32_t n = nL + nR;
  if (int rc = ensure_part_capacity(c, n, mc != nullptr)) return rc;
  const TileScratch sc = tile_scratch(c->d_tile, c->d_part.cap);
  {
    ScopedKernel k(c, K_TILE_HIST, (uint64_t)n * 16);  // ingest: the raw records, read once
    launch_tile_hist(cur_stream(c), evL, nL, evR, nR, c->tgeom, sc, c->d_rejected, mc, mc ? c->d_warp.p : nullptr);
  }
  {
    ScopedKernel k(c, K_TILE_SCAN, 0);  // (the count matrices: not in SURVEY's accounting)
    launch_tile_scan(cur_stream(c), nL, nR, c->tgeom, sc, c->d_rejected);
  }
  {
    ScopedKernel k(c, K_TILE_SCATTER, (uint64_t)n * 24);  // the partition's own traffic: 16 B in, 8 B out (16 for wide records)
    launch_tile_scatter(cur_stream(c), evL, nL, evR, nR, c->tgeom, sc, c->d_part, mc ? c->d_warp.p : nullptr);
  }
  {
    ScopedKernel k(c, K_TILE_APPLY, (uint64_t)n * 32);
    launch_tile_apply(cur_stream(c), c->d_part, n, c->tgeom, sc, L2, S2, c->cfg.feature_filter_threshold,
                      arc_touched, c->zpin[0].counts + 3, c->lim.ticket);
  }
  return 0;
}

// keys[0] / vals[0] (n pairs, their digit histograms in the sort scratch, look-back words cleared) -> sorted by
// `passes` stable passes of `bits` bits each; returns which of keys[] / vals[] holds the result.  `booked`: the passes
// are booked as K_RADIX_PASS (goodFeaturesToTrack's stages are not in the kernel statistics).
int radix_sort_pairs(esvio_fe_ctx* c, uint32_t n, int passes, int bits, bool booked) {
  return radix_sort_pairs(c, SortBufs{{c->keys[0], c->keys[1]}, {c->vals[0], c->vals[1]}, c->hist, nullptr}, n, passes,
                          bits, booked);
}

int radix_sort_pairs(esvio_fe_ctx* c, const SortBufs& b, uint32_t n, int passes, int bits, bool booked) {
  const SortScratch sc = sort_scratch(b.scratch);
  const size_t pass_words = (size_t)radix_blocks(n) << bits;
  int cur = 0;
  for (int p = 0; p < passes; p++) {
    std::optional<ScopedKernel> k;
    if (booked) k.emplace(c, K_RADIX_PASS, (uint64_t)n * 16);
    launch_radix_pass(cur_stream(c), b.keys[cur], b.vals[cur], n, p * bits, bits, sc.ghist + ((size_t)p << bits),
                      sc.lookback + p * pass_words, sc.tickets + p, b.keys[cur ^ 1], b.vals[cur ^ 1],
                      c->zpin[0].counts + 3, c->lim.lookback, b.n_dev);
    cur ^= 1;
  }
  return cur;
}

// ---------------------------------------------------------------- event images (esvio_fe_set_event_images)
using EvimgSet = esvio_fe_ctx::Evimg::Set;
// a camera's image (and its mark plane) of set S is about to be written on stream s: behind its last writer, if that
// was another stream (a plain call's right camera runs on the stereo stream, an announced batch's on the prefetch stream)
static int evimg_order(esvio_fe_ctx* c, EvimgSet& S, int cams, hipStream_t s) {
  for (int cam = 0; cam < 2; cam++)
    if ((cams >> cam & 1) && S.wstream[cam] && S.wstream[cam] != s) HIPCHK(c, hipStreamWaitEvent(s, S.written[cam], 0));
  return 0;
}
static int evimg_written(esvio_fe_ctx* c, EvimgSet& S, int cams, hipStream_t s) {
  for (int cam = 0; cam < 2; cam++)
    if (cams >> cam & 1) {
      HIPCHK(c, hipEventRecord(S.written[cam], s));
      S.wstream[cam] = s;
    }
  return 0;
}

// the current set's images zero; every_set (esvio_fe_reset, no batch announced any more): every set's, their mark
// planes too, and set 0 is the current one again
int evimg_zero(esvio_fe_ctx* c, bool every_set) {
  esvio_fe_ctx::Evimg& E = c->evimg;
  hipStream_t s = cur_stream(c);
  if (every_set) E.cur = 0;
  for (int k = every_set ? 0 : E.cur; k < (every_set ? E.nsets : E.cur + 1); k++) {
    EvimgSet& S = E.set[k];
    if (int rc = evimg_order(c, S, 3, s)) return rc;
    for (int cam = 0; cam < 2; cam++) {
      HIPCHK(c, hipMemsetAsync(S.img[cam], 0, (size_t)E.groups * 12, s));
      // (the emit leaves the mark planes zero; a call that failed between its mark and its emit may not have)
      if (every_set) HIPCHK(c, hipMemsetAsync(S.marks[cam], 0, (size_t)E.groups * 16, s));
    }
    if (int rc = evimg_written(c, S, 3, s)) return rc;
  }
  E.fresh_cams = 0;
  return 0;
}

// The batch a call's SAE update consumes -> the event images, on the update's stream, behind it (the tiled update has
// filled d_warp by then).  The cameras of E.fresh_cams are rewritten (a track call's: zero, then the rule), the others
// that have events accumulate (a stage call's).  Reads the event arrays on the stream the update reads them on, so
// whatever keeps them alive for the update keeps them alive for this.
// Inside an announced batch's prefetch sequence (t_prefetch_batch; possibly on the launch thread): both cameras of the
// BATCH's set are rewritten, what to wait for comes with the batch, and no word of the handle's own state is touched.
int evimg_update(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR, const McParams* mc) {
  esvio_fe_ctx::Evimg& E = c->evimg;
  const Inflight* job = t_prefetch_batch;
  if (job && job->evset < 0) return 0;
  const uint32_t n = nL + nR;
  EvimgSet& S = E.set[job ? job->evset : E.cur];
  const int fresh = job ? 3 : E.fresh_cams, acc = ((nL ? 1 : 0) | (nR ? 2 : 0)) & ~fresh;
  if (!job) E.fresh_cams = 0;
  if (!(fresh | acc)) return 0;
  hipStream_t s = cur_stream(c);
  if (job) {
    for (int cam = 0; cam < 2; cam++)
      if (job->ev_wait >> cam & 1) HIPCHK(c, hipStreamWaitEvent(s, S.written[cam], 0));
  } else if (int rc = evimg_order(c, S, fresh | acc, s)) {
    return rc;
  }
  if (n) {
    const bool warped = mc && mc->enabled;
    ScopedKernel k(c, K_EVIMG_MARK, (uint64_t)n * (warped && c->tiled ? 24 : 20));  // the record (+ its warped pixel) in, one atomic word out
    launch_evimg_mark(s, evL, nL, evR, nR, c->W, c->H, S.marks[0], S.marks[1],
                      !warped ? kEvimgPixOwn : c->tiled ? kEvimgPixWarp : kEvimgPixMc, c->d_warp, mc);
  }
  for (int form = 0; form < 2; form++) {
    const int cams = form ? acc : fresh;
    if (!cams) continue;
    const int c0 = cams & 1 ? 0 : 1, ncam = cams == 3 ? 2 : 1;
    ScopedKernel k(c, K_EVIMG_EMIT, (uint64_t)E.groups * 4 * (4 + 3) * ncam);  // the marks in, the bytes out (marks set: + 4 B back)
    launch_evimg_emit(s, S.marks[c0], S.img[c0], ncam == 2 ? S.marks[1].p : nullptr, ncam == 2 ? S.img[1].p : nullptr,
                      E.groups, form == 0);
  }
  if (job) {  // (wstream[] was set with the batch's bookkeeping, prefetch_next)
    for (int cam = 0; cam < 2; cam++) HIPCHK(c, hipEventRecord(S.written[cam], s));
    return 0;
  }
  return evimg_written(c, S, fresh | acc, s);
}

// arc_set >= 0: this batch's Arc* pass will run into candidate set arc_set; *arc_marked tells
// whether the update has set that set's touched flags on its way (else run_arc does it)
static int sae_update_planes(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
                             const McParams* mc, double2* L2, double2* S2, int arc_set, bool* arc_marked);
int sae_update(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR,
               uint32_t nR, const McParams* mc, double2* L2, double2* S2, int arc_set, bool* arc_marked) {
  if (int rc = sae_update_planes(c, evL, nL, evR, nR, mc, L2, S2, arc_set, arc_marked)) return rc;
  // the handle's own planes: the event images follow (the time-slice entry points' scratch pair writes none)
  return c->evimg.on && !L2 && !S2 ? evimg_update(c, evL, nL, evR, nR, mc) : 0;
}

static int sae_update_planes(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
                             const McParams* mc, double2* L2, double2* S2, int arc_set, bool* arc_marked) {
  const uint32_t n = nL + nR;
  if (!n) return 0;
  if (!L2) L2 = c->L2;  // (other planes: the scratch pair of the time-slice entry points)
  if (!S2) S2 = c->S2;
  if (arc_marked) *arc_marked = false;
  if (c->tiled) {
    // (motion compensation: the update happens at the warped pixels, Arc* is asked about the events'
    // own pixels (feature_tracker.cpp:698 -> :13-38), so the tiles' touched flags are not Arc*'s)
    uint8_t* mark = arc_set >= 0 && nL && !mc ? c->d_touched[arc_set].p : nullptr;
    if (arc_marked) *arc_marked = mark != nullptr;
    return sae_update_tiled(c, evL, nL, evR, nR, L2, S2, mark, mc);
  }
  if (int rc = ensure_sort_capacity(c, n)) return rc;
  const int passes = (c->key_bits + 6) / 7;
  const int bits = (c->key_bits + passes - 1) / passes;
  const SortScratch sc = sort_scratch(c->hist);
  {
    ScopedKernel k(c, K_SAE_KEYS, (uint64_t)n * 16);
    launch_sae_keys(cur_stream(c), evL, nL, evR, nR, c->W, c->H, c->keys[0], c->vals[0], c->invalid_key,
                    c->d_rejected, passes, bits, sc.ghist, sc.lookback, (uint32_t)passes * (radix_blocks(n) << bits), mc);
  }
  const int cur = radix_sort_pairs(c, n, passes, bits);
  {
    ScopedKernel k(c, K_SAE_APPLY, (uint64_t)n * 32);
    if (n >= c->sae_ev_min)  // many events per pixel: one lane per event
      launch_sae_apply_ev(cur_stream(c), c->keys[cur], c->vals[cur], n, evL, nL, evR, L2, S2,
                          c->cfg.feature_filter_threshold, c->invalid_key, c->hist, sc.head_words, c->sae_marks);
    else
      launch_sae_apply(cur_stream(c), c->keys[cur], c->vals[cur], n, evL, nL, evR, L2, S2,
                       c->cfg.feature_filter_threshold, c->invalid_key, c->hist, sc.head_words);
  }
  return 0;
}

// stage host events into the handle's device buffer; returns device pointers
int stage_events(esvio_fe_ctx* c, const esvio_fe_event* left, size_t nL,
                 const esvio_fe_event* right, size_t nR, int space, const EventRec** dL,
                 const EventRec** dR, int lane) {
  if (space == ESVIO_FE_DEVICE) {
    *dL = (const EventRec*)left;
    *dR = (const EventRec*)right;
    return 0;
  }
  if (space != ESVIO_FE_HOST) return fail(c, ESVIO_FE_EINVAL, "bad memory space %d", space);
  DevBuf<EventRec>& buf = lane >= 0 ? c->d_evp[lane] : c->d_ev;
  if (int rc = buf.grow(c, nL + nR)) return rc;
  if (nL) HIPCHK(c, hipMemcpyAsync(buf, left, nL * 16, hipMemcpyHostToDevice, cur_stream(c)));
  if (nR) HIPCHK(c, hipMemcpyAsync(buf + nL, right, nR * 16, hipMemcpyHostToDevice, cur_stream(c)));
  *dL = buf;
  *dR = buf + nL;
  return 0;
}

void render_ts(esvio_fe_ctx* c, double t_sync, uint8_t* dst0, uint8_t* dst1, int ncam,
               const double2* S2) {
  const int stride = c->pyr[0].d.stride[0];
  const int mk = c->cfg.median_blur_kernel_size;
  uint8_t* r0 = mk > 0 ? c->med_tmp[0].d.img[0] : dst0;
  uint8_t* r1 = mk > 0 ? c->med_tmp[ncam == 2 ? 1 : 0].d.img[0] : dst1;
  {
    ScopedKernel k(c, K_TIME_SURFACE4, (uint64_t)c->P * 17 * ncam);
    k.id = launch_time_surface(cur_stream(c), S2, c->W, c->H, t_sync, c->cfg.decay_ms / 1000.0,
                               c->cfg.ignore_polarity, r0, r1, stride, ncam);
  }
  if (mk > 0) {  // cv::medianBlur(2k+1) of the rendered surface (event_detector.cc:262-264)
    const size_t o = (size_t)kPad * stride + kPad;
    ScopedKernel k(c, K_MEDIAN, 0);
    launch_median(cur_stream(c), r0 + o, r1 + o, stride, dst0 + o, dst1 + o, stride, c->W, c->H, mk, ncam);
  }
}


// CLAHE of nimg images, stages 0 .. stages-1: per-tile LUTs, LUT blending + min/max, MINMAX normalisation in place.
// booked_px: the pixels per image the stages are booked with (0: the image front-end's, which are not)
void run_clahe(esvio_fe_ctx* c, const uint8_t* src0, const uint8_t* src1, int src_stride, uint8_t* dst0, uint8_t* dst1,
               int dst_stride, int nimg, int stages, uint64_t booked_px) {
  for (int stage = 0; stage < stages; stage++) {
    ScopedKernel k(c, K_CLAHE, booked_px * (stage == 0 ? 1 : 2) * nimg);
    launch_clahe(cur_stream(c), src0, src1, src_stride, dst0, dst1, dst_stride, c->W, c->H, c->d_lut, c->d_minmax, nimg,
                 stage);
  }
}

// the image trackEvent feeds to LK: the raw time surface, or CLAHE + normalize of it when
// `equalize` (feature_tracker.cpp:375-387).  cams: bit 0 left, bit 1 right.  Raw surfaces stay
// available for the TS_LK_THRESHOLD test and gettimesurface().
void render_lk_images(esvio_fe_ctx* c, double t_sync, int cams, int slotL, int slotR, int rawbuf) {
  const bool eq = c->cfg.equalize;
  // the cameras rendered: cam0, and with both cam1 = the right one (one camera: both name it)
  const int cam0 = cams == 2 ? 1 : 0, cam1 = cams == 1 ? 0 : 1, nimg = cams == 3 ? 2 : 1;
  const PyrDesc* lk[2] = {&c->pyr[slotL].d, &c->pyr[slotR].d};
  const PyrDesc &l0 = *lk[cam0], &l1 = *lk[cam1];
  const PyrDesc &r0 = eq ? c->raw[rawbuf][cam0].d : l0, &r1 = eq ? c->raw[rawbuf][cam1].d : l1;  // the raw surfaces
  render_ts(c, t_sync, r0.img[0], r1.img[0], nimg, c->S2 + (size_t)cam0 * c->P);
  if (eq) run_clahe(c, px00(r0), px00(r1), r0.stride[0], px00(l0), px00(l1), l0.stride[0], nimg, 3, c->P);
}

// The fused kernels apply — the time surface rendered into level 0 in place, levels 1..3 in one launch, borders and
// Scharr in one — when nothing sits between the surface and the pyramid (no median) and the pyramid has the three
// levels they build.  With `equalize` the middle launch is k_norm_pyr (both cameras only) instead of k_pyr3.
static bool fused_build_ok(const esvio_fe_ctx* c, const PyrDesc& d) {
  return c->fuse_ts_pyr && c->cfg.median_blur_kernel_size <= 0 && d.levels == 3;
}
// ... for one camera alone (a plain call split by camera, fe_track.cpp)
bool render_cam_ok(const esvio_fe_ctx* c) { return !c->cfg.equalize && fused_build_ok(c, c->pyr[0].d); }

// The LK images of the cameras in `cams` (1 left, 2 right, 3 both) at t_sync and their pyramids.  right_imported
// (cams == 1): the right image is in slotR already (esvio_fe_import_image) and gets its pyramid here too.
void build_lk_images(esvio_fe_ctx* c, double t_sync, int cams, int slotL, int slotR, int rawbuf, bool right_imported) {
  const int cam0 = cams == 2 ? 1 : 0, nimg = cams == 3 ? 2 : 1;
  const PyrDesc two[2] = {c->pyr[slotL].d, c->pyr[slotR].d};
  const PyrDesc* p = two + cam0;
  if (right_imported || !fused_build_ok(c, p[0]) || (c->cfg.equalize && cams != 3)) {
    render_lk_images(c, t_sync, cams, slotL, slotR, rawbuf);
    pyr_build(c, p, right_imported ? 2 : nimg);
    return;
  }
  const uint64_t px = pyr_pixels(p[0]);
  if (c->cfg.equalize) {
    // time surfaces -> raw; CLAHE LUTs; CLAHE output -> a linear scratch pair (no in-place normalise:
    // the fused kernel's blocks read their neighbours' pixels); normalise + pyramid levels
    const PyrDesc& rl = c->raw[rawbuf][0].d;
    const PyrDesc& rr = c->raw[rawbuf][1].d;
    render_ts(c, t_sync, rl.img[0], rr.img[0], 2, c->S2);
    run_clahe(c, px00(rl), px00(rr), rl.stride[0], c->d_eq_tmp, c->d_eq_tmp + c->P, c->W, 2, 2, c->P);
    ScopedKernel k(c, K_NORM_PYR, ((uint64_t)c->P + px) * 2);
    launch_norm_pyr(cur_stream(c), c->d_eq_tmp, c->d_eq_tmp + c->P, c->W, c->d_minmax, two);
  } else {
    render_ts(c, t_sync, p[0].img[0], p[nimg - 1].img[0], nimg, c->S2 + (size_t)cam0 * c->P);
    ScopedKernel k(c, K_PYR3, px * nimg);
    launch_pyr3(cur_stream(c), p, nimg);
  }
  ScopedKernel k(c, K_PAD_SCHARR, px * 5 * nimg);
  launch_pad_scharr(cur_stream(c), p, nimg);
}

// the next frame's slots: a left slot that is neither prev nor cur (the first frame: slot 0), the other right slot —
// unless esvio_fe_import_image has advanced it with the image it brought (right_advanced) — and the next raw pair
void rotate_slots(esvio_fe_ctx* c, bool right_advanced) {
  int sl = 0;
  while (c->have_img && (sl == c->slot_prevL || sl == c->slot_curL)) sl++;
  c->slot_curL = sl;
  if (!right_advanced) c->slot_curR = other_right_slot(c);
  c->raw_cur = (c->raw_cur + 1) % kRightSlots;
}

const PyrDesc& raw_ts_desc(const esvio_fe_ctx* c, int cam) {
  if (c->cfg.equalize) return c->raw[c->raw_cur][cam].d;
  return cam ? c->pyr[c->slot_curR].d : c->pyr[c->slot_curL].d;
}

LkArgs make_lk(const PyrDesc& P, const PyrDesc& N, const float2* prev, const float2* init,
               float2* next, uint8_t* status, const int* n_ptr, int n_max, int max_level,
               int max_count, double eps, int flags) {
  LkArgs a;
  a.P = P;
  a.N = N;
  a.prev_pts = prev;
  a.init_pts = init ? init : next;
  a.next_pts = next;
  a.status = status;
  a.n_ptr = n_ptr;
  a.n_max = n_max;
  a.max_level = std::min(max_level, P.levels);
  // TermCriteria normalisation of calcOpticalFlowPyrLK [OpenCV]
  a.max_count = std::min(std::max(max_count, 0), 100);
  double e = std::min(std::max(eps, 0.), 10.);
  a.eps2 = e * e;
  a.flags = flags;
  return a;
}

// forward call (+ optional backward call fused into the same launch)
void run_lk(esvio_fe_ctx* c, const LkArgs& f, const LkArgs* b, float2* back_pts,
            uint8_t* back_status) {
  uint64_t bytes = (uint64_t)f.n_max * (f.max_level + 1) * kLkWin * kLkWin * 5;
  if (b) bytes += (uint64_t)f.n_max * (b->max_level + 1) * kLkWin * kLkWin * 5;
  ScopedKernel k(c, c->cfg.lk_accum == 2 ? K_LK_F32 : K_LK, bytes);
  LkArgs fa = f;
  fa.accum = c->cfg.lk_accum;
  launch_lk(cur_stream(c), fa, b, back_pts, back_status);
}

LkPair lk_pair(const PyrDesc& P, const PyrDesc& N, const P2f* src, const int* n_ptr, int n_max, LkPairKind kind,
               const LkOut& out) {
  const bool t = kind == kLkTemporal;
  return LkPair{make_lk(P, N, (const float2*)src, nullptr, (float2*)out.fwd, out.st_fwd, n_ptr, n_max, 3, 30, 0.01, 0),
                make_lk(N, P, nullptr, nullptr, nullptr, nullptr, n_ptr, n_max, t ? 1 : 3, 30, 0.01,
                        t ? ESVIO_FE_LK_USE_INITIAL_FLOW : 0),
                out};
}

void run_lk_pair(esvio_fe_ctx* c, const LkPair& p) {
  run_lk(c, p.f, c->cfg.flow_back ? &p.b : nullptr, (float2*)p.out.back, p.out.st_back);
}

// A caller's W x H image <-> level 0 of a padded pyramid.  Not as one 2-D copy between the caller's
// pageable memory and the pitched device image: the runtime does that row by row (4.5 ms for a
// stereo pair of 346 x 260 images, more than the rest of trackImage together).  The rows go through
// a pinned staging ring as one block, one linear copy crosses PCIe, and the re-pitching is a
// device-to-device copy.
static int image_stage_slot(esvio_fe_ctx* c, size_t bytes, size_t* off) {
  constexpr int kSlots = 4;  // (a frame stages at most two images; a slot is reused two frames later,
                             // and every call that stages an image waits for its stream before it returns
                             // or, on the way in, before the next trackImage call can come)
  if (!c->d_img || c->d_img.cap < kSlots * bytes) {  // (the pair's second: both are there)
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
    c->d_img.release();
    if (int rc = c->h_img.alloc(c, kSlots * bytes)) return rc;
    if (int rc = c->d_img.alloc(c, kSlots * bytes)) return rc;
  }
  *off = (size_t)(c->img_stage_next++ % kSlots) * (c->d_img.cap / kSlots);
  return 0;
}

int copy_level0_in(esvio_fe_ctx* c, const PyrDesc& d, const uint8_t* in, int space) {
  const int stride = d.stride[0];
  const size_t bytes = (size_t)d.w[0] * d.h[0];
  if (space == ESVIO_FE_DEVICE) {  // a dense image that lies on the device already: the re-pitching alone
    HIPCHK(c, hipMemcpy2DAsync(d.img[0] + (size_t)kPad * stride + kPad, stride, in, d.w[0], d.w[0], d.h[0], hipMemcpyDeviceToDevice,
                               cur_stream(c)));
    return 0;
  }
  size_t off = 0;
  if (int rc = image_stage_slot(c, bytes, &off)) return rc;
  std::memcpy(c->h_img + off, in, bytes);
  HIPCHK(c, hipMemcpyAsync(c->d_img + off, c->h_img + off, bytes, hipMemcpyHostToDevice, cur_stream(c)));
  HIPCHK(c, hipMemcpy2DAsync(d.img[0] + (size_t)kPad * stride + kPad, stride, c->d_img + off, d.w[0], d.w[0],
                             d.h[0], hipMemcpyDeviceToDevice, cur_stream(c)));
  return 0;
}

int copy_level0_out(esvio_fe_ctx* c, const PyrDesc& d, uint8_t* out) {
  const int stride = d.stride[0];
  const size_t bytes = (size_t)d.w[0] * d.h[0];
  size_t off = 0;
  if (int rc = image_stage_slot(c, bytes, &off)) return rc;
  HIPCHK(c, hipMemcpy2DAsync(c->d_img + off, d.w[0], d.img[0] + (size_t)kPad * stride + kPad, stride, d.w[0],
                             d.h[0], hipMemcpyDeviceToDevice, cur_stream(c)));
  HIPCHK(c, hipMemcpyAsync(c->h_img + off, c->d_img + off, bytes, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  std::memcpy(out, c->h_img + off, bytes);
  return 0;
}

// ---------------------------------------------------------------- host bookkeeping (reference
// helpers in feature_tracker.cpp)

bool in_border_event(const esvio_fe_ctx* c, const P2f& pt) {  // :48-54
  const int BORDER_SIZE = 1;
  const int img_x = host::cv_round(pt.x), img_y = host::cv_round(pt.y);
  return BORDER_SIZE <= img_x && img_x < c->W - BORDER_SIZE && BORDER_SIZE <= img_y &&
         img_y < c->H - BORDER_SIZE;
}

double pt_distance(const P2f& a, const P2f& b) {  // :1314-1319
  const double dx = a.x - b.x, dy = a.y - b.y;
  return std::sqrt(dx * dx + dy * dy);
}

// Event_setMask (:123-151): std::sort on the same element type/comparator as the reference so
// the (unstable) permutation of equal track counts is inherited from libstdc++.
void event_set_mask(esvio_fe_ctx* c) {
  c->mask_event.reset(c->W, c->H);
  // (the sort only ever compares .first, so carrying src_idx along as payload leaves the
  // permutation — std::sort is not stable — exactly what it is for the reference's pair type)
  struct Item {
    int first;
    std::pair<P2f, int> second;
    int src;
  };
  std::vector<Item> cnt_pts_id;
  cnt_pts_id.reserve(c->cur_pts.size());
  for (unsigned int i = 0; i < c->cur_pts.size(); i++)
    cnt_pts_id.push_back(Item{c->track_cnt[i], std::make_pair(c->cur_pts[i], c->ids[i]), c->src_idx[i]});
  std::sort(cnt_pts_id.begin(), cnt_pts_id.end(),
            [](const Item& a, const Item& b) { return a.first > b.first; });
  c->cur_pts.clear();
  c->ids.clear();
  c->track_cnt.clear();
  c->src_idx.clear();
  for (auto& it : cnt_pts_id) {
    const int px = host::cv_round(it.second.first.x), py = host::cv_round(it.second.first.y);
    if (px < 0 || px >= c->W || py < 0 || py >= c->H) continue;  // cannot happen after inBorder
    if (!c->mask_event.test(px, py)) {
      c->cur_pts.push_back(it.second.first);
      c->ids.push_back(it.second.second);
      c->track_cnt.push_back(it.first);
      c->src_idx.push_back(it.src);
      c->mask_event.stamp_disc(px, py, c->cfg.min_dist, c->hw);
    }
  }
}

std::vector<P2f> undistorted_pts(const std::vector<P2f>& pts, const esvio_fe_camera& cam) {  // :991
  const size_t n = pts.size();
  std::vector<P2f> un(n);
  if (!n) return un;
  std::vector<double> lx(n), ly(n);
  host::lift_projective_batch(cam, &pts[0].x, (int)n, lx.data(), ly.data());
  for (size_t i = 0; i < n; i++) un[i] = P2f{(float)lx[i], (float)ly[i]};  // b[2] == 1.0
  return un;
}

// ptsVelocity (:1004-1045) incl. its quirk: with no previous map the result is sized by the LEFT
// cur_pts whichever camera it is called for.
// (dt = cur_time - prev_time and the left point count of the frame the call belongs to are passed
// in: the right-camera tail of a frame may run during the next call, see finalize_right.)
std::vector<P2f> pts_velocity_fn(std::vector<int>& ids, std::vector<P2f>& pts, IdMap& cur_id_pts,
                                 IdMap& prev_id_pts, double dt, size_t n_left) {
  std::vector<P2f> vel;
  cur_id_pts.build(ids, pts);
  if (!prev_id_pts.empty()) {
    vel.reserve(pts.size());
    for (unsigned int i = 0; i < pts.size(); i++) {
      const P2f* prev = ids[i] != -1 ? prev_id_pts.find(ids[i]) : nullptr;
      if (prev) {
        const double v_x = (pts[i].x - prev->x) / dt;
        const double v_y = (pts[i].y - prev->y) / dt;
        vel.push_back(P2f{(float)v_x, (float)v_y});
      } else {
        vel.push_back(P2f{0, 0});
      }
    }
  } else {
    vel.assign(n_left, P2f{0, 0});
  }
  return vel;
}

void reject_with_f_event(esvio_fe_ctx* c) {  // :910-947
  if (c->trace) c->tr_fm_class[c->cur_pts.size() < 8 ? 0 : c->cur_pts.size() < 15 ? 1 : 2]++;
  if (c->cur_pts.size() >= 8) {
    const esvio_fe_camera& cam = c->cfg.cam[0];
    const double FOCAL = c->cfg.focal_length;
    const size_t n = c->prev_pts.size();
    std::vector<float> un_cur(n * 2), un_prev(n * 2);
    std::vector<double> lx(n), ly(n);
    const double cx = c->W / 2.0, cy = c->H / 2.0;
    const auto tl = std::chrono::steady_clock::now();
    // (prev_pts' lifts: done under the temporal LK's wait when the frame publishes, TrackCall::temporal)
    const bool pre = c->pre_lift_valid && c->pre_lx.size() == n;
    if (!pre) host::lift_projective_batch(cam, &c->prev_pts[0].x, (int)n, lx.data(), ly.data());
    const double* plx = pre ? c->pre_lx.data() : lx.data();
    const double* ply = pre ? c->pre_ly.data() : ly.data();
    c->pre_lift_valid = false;  // (one use: the vectors belong to the call that made them)
    for (size_t i = 0; i < n; i++) {  // p[2] == 1.0: x / 1.0 is exact
      un_prev[2 * i] = (float)(FOCAL * plx[i] / 1.0 + cx);
      un_prev[2 * i + 1] = (float)(FOCAL * ply[i] / 1.0 + cy);
    }
    host::lift_projective_batch(cam, &c->cur_pts[0].x, (int)n, lx.data(), ly.data());
    for (size_t i = 0; i < n; i++) {
      un_cur[2 * i] = (float)(FOCAL * lx[i] / 1.0 + cx);
      un_cur[2 * i + 1] = (float)(FOCAL * ly[i] / 1.0 + cy);
    }
    std::vector<uint8_t> status(c->cur_pts.size());
    const auto t0 = std::chrono::steady_clock::now();
    host::find_fundamental_mat(un_prev.data(), un_cur.data(), (int)c->cur_pts.size(),
                               c->cfg.f_threshold, 0.99, status.data(), c->pool);
    if (c->trace) {
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      c->tr_fm_ms += ms;
      c->tr_fm_max_ms = std::max(c->tr_fm_max_ms, ms);
      c->tr_lift_ms += std::chrono::duration<double, std::milli>(t0 - tl).count();
    }
    reduce_vector(c->prev_pts, status);
    reduce_vector(c->cur_pts, status);
    reduce_vector(c->ids, status);
    reduce_vector(c->track_cnt, status);
    reduce_vector(c->src_idx, status);
  }
}

void clear_tracker_state(esvio_fe_ctx* c) {
  c->prev_pts.clear();
  c->cur_pts.clear();
  c->cur_right_pts.clear();
  c->n_pts.clear();
  c->cur_un_pts.clear();
  c->cur_un_right_pts.clear();
  c->pts_velocity.clear();
  c->right_pts_velocity.clear();
  c->ids.clear();
  c->ids_right.clear();
  c->track_cnt.clear();
  c->track_cnt_right.clear();
  c->cur_un_pts_map.clear();
  c->prev_un_pts_map.clear();
  c->cur_un_right_pts_map.clear();
  c->prev_un_right_pts_map.clear();
  c->have_img = false;
  c->slot_prevL = c->slot_curL = 0;
  c->slot_curR = kLeftSlots;
  c->ext_right_pending = false;
  c->ext_sae_pending = false;
  c->cur_time = c->prev_time = 0;
}

// the selection over candidate set `set` with the handle's disc (cv::circle of min_dist); what a caller's selection
// differs in — another list, another disc, host_counts, a mask, publication — it sets itself
SelectArgs make_select_args(esvio_fe_ctx* c, int set, int max_corners, float2* out_pts, int out_base,
                            int32_t* out_idx) {
  SelectArgs s{};
  s.comp_xy = c->cand[set].comp_xy;
  s.comp_idx = c->cand[set].comp_idx;
  s.total = c->cand[set].total;
  s.W = c->W;
  s.H = c->H;
  s.wpr = (c->W + 31) / 32;
  s.max_corners = max_corners;
  s.radius = c->cfg.min_dist;
  for (int i = 0; i <= kMaxDiscR; i++) s.hw[i] = i < (int)c->hw.size() ? (int8_t)c->hw[i] : -1;
  s.disc_c = disc_threshold(s.hw, s.radius);
  s.out_pts = out_pts;
  s.out_idx = out_idx;
  s.out_base = out_base;
  s.n_out = c->dres.counts;
  s.n_total = c->dres.counts + 1;
  s.host_counts = nullptr;
  s.init_bits = nullptr;
  s.gbitmap = nullptr;
  s.pub_slots = nullptr;
  s.pub_done = nullptr;
  s.pub_seq = 0;
  s.one_wave = c->select_one_wave ? 1 : 0;
  return s;
}

size_t select_lds_bytes(const esvio_fe_ctx* c) {
  // bitmap + half-width table + the kept points whose discs seed the bitmap
  return ((size_t)c->H * ((c->W + 31) / 32) + 4 + 64 + (size_t)std::max(c->cfg.max_cnt, 1)) * 4;
}
static size_t select_tables_lds_bytes(const esvio_fe_ctx* c) {  // with the bitmap in global memory
  return (4 + 64 + (size_t)std::max(c->cfg.max_cnt, 1)) * 4;
}

// the greedy selection `s` describes, its bitmap in LDS or — where that does not fit (select_ok, esvio_fe_create:
// d_sel_bitmap is there then) — in device memory: slower, same result.  (A caller that has set s.gbitmap itself gets the
// device-memory form on any handle: esvio_fe_select_candidates, test tap)
KernelId launch_select_args(esvio_fe_ctx* c, SelectArgs s) {
  if (!c->select_ok) s.gbitmap = c->d_sel_bitmap;
  ScopedKernel k(c, K_SELECT_MW, 0);
  const KernelId id = launch_select(cur_stream(c), s, s.gbitmap ? select_tables_lds_bytes(c) : select_lds_bytes(c));
  k.id = id;
  return id;
}

// ordered compaction of the first nblk per-block lists of `cs` (right behind the kernel that filled them).  booked: as
// K_COMPACT in the kernel statistics, and with the set's group sums (goodFeaturesToTrack's stages are neither)
void compact_set(esvio_fe_ctx* c, const esvio_fe_ctx::CandSet& cs, uint32_t nblk, bool booked) {
  std::optional<ScopedKernel> k;
  if (booked) k.emplace(c, K_COMPACT, 0);
  launch_compact(cur_stream(c), cs.xy, cs.idx, cs.cnt, nblk, cs.comp_xy, cs.comp_idx, cs.total, booked ? cs.grp.p : nullptr);
}

// the sequential greedy (Event_FeaturesToTrack) over the compacted candidates of set `set`;
// `mask_bits`: blocked pixels the disc bitmap starts from (null: none, or already applied by k_arc)
void run_select(esvio_fe_ctx* c, int set, int max_corners, float2* out_pts, int out_base,
                int32_t* out_idx, const uint32_t* mask_bits, int* host_counts, bool publish,
                const float2* stamp_pts, int n_stamp) {
  SelectArgs s = make_select_args(c, set, max_corners, out_pts, out_base, out_idx);
  s.host_counts = host_counts;
  s.init_bits = mask_bits;
  s.stamp_pts = stamp_pts;
  s.n_stamp = n_stamp;
  if (publish) {
    s.pub_slots = c->d_pub_slots;
    s.pub_done = c->d_pub_done;
    s.pub_seq = c->pub_seq;
  }
  launch_select_args(c, s);
}

// Arc* flags (+ ordered per-block candidate lists into set `set`) for the left events; `ts` is the
// RAW left time surface the TS_LK_THRESHOLD test reads (null: no test)
void run_arc(esvio_fe_ctx* c, const EventRec* ev, uint32_t n, const PyrDesc* ts, bool use_mask,
             bool want_flags, bool want_cand, int set, bool marked) {
  ArcArgs a{};
  a.ev = ev;
  a.n = n;
  a.L2 = c->L2;
  a.S2 = c->S2;
  a.W = c->W;
  a.H = c->H;
  a.filter_threshold = c->cfg.feature_filter_threshold;
  a.border = c->cfg.min_dist + 1;
  a.ts = ts ? ts->img[0] : nullptr;  // RAW left time surface (:26)
  a.ts_stride = ts ? ts->stride[0] : 0;
  a.ts_lk_threshold = c->cfg.ts_lk_threshold;
  a.mask_bits = use_mask ? c->d_mask_bits.p : nullptr;
  a.wpr = (c->W + 31) / 32;
  a.flags = want_flags ? c->d_flags.p : nullptr;
  a.cand_xy = want_cand ? c->cand[set].xy.p : nullptr;
  a.cand_idx = want_cand ? c->cand[set].idx.p : nullptr;
  a.cand_cnt = want_cand ? c->cand[set].cnt.p : nullptr;
  // Only a pixel's earliest candidate can be accepted (a later one finds the pixel blocked whatever happened to the
  // first): an atomicMin per candidate here + k_dedup halve the list k_select walks.  That paid with the one-wave
  // k_select (54 against 57 us at 0.17 M left events); k_select_mw does not care until it has to dig through the
  // whole list — max_cnt 1000: 63 us with, 98 without — while the atomics cost k_arc_ev 2.4 us at C3, 9 at 20 Mev/s
  // (0.131 -> 0.1225 ms per replay step without them), 43 at 3.3 M left events, and most of its HBM writes.  So:
  // handles with max_cnt > 500 only (esvio_fe_create; ESVIO_FE_DEDUP=1 / ESVIO_FE_NO_DEDUP=1 force it), batches < 2^20.
  const bool dedup = want_cand && c->dedup_enabled && c->d_first[set] && n < (1u << 20);
  if (dedup) {
    // keys count down from launch to launch: 0xfe.. for the first, 0x01.. for the 254th, then the
    // map is cleared (to all ones) and the count starts again
    const uint32_t e = c->first_epoch[set]++ % 254u;
    if (e == 0)
      (void)hipMemsetAsync(c->d_first[set], 0xff, (size_t)c->P * 4, cur_stream(c));
    a.first_map = c->d_first[set];
    a.first_key = (254u - e) << 24;
  }
  a.cmap = c->d_cmap[set];
  a.touched = c->d_touched[set];
  {
    // the events' x,y,p once more (16 B records) -> touched bits; then per touched pair its 16/20
    // ring values (counted once per pixel: 16 B) + {L0,L1}
    ScopedKernel k(c, K_ARC_MAP, (uint64_t)n * 16 + (uint64_t)c->P * 32);
    if (!marked) launch_arc_mark(cur_stream(c), a);  // (else: done by the SAE update's first pass)
    launch_arc_map(cur_stream(c), a);
  }
  {
    ScopedKernel k(c, K_ARC_EV, (uint64_t)n * 16);
    launch_arc(cur_stream(c), a);
  }
  if (dedup) {
    ScopedKernel k(c, K_DEDUP, 0);
    launch_dedup(cur_stream(c), a.cand_xy, a.cand_idx, a.cand_cnt, (n + kArcBlock - 1) / kArcBlock,
                 a.first_map, a.first_key, c->W);
  }
}

int run_detect(esvio_fe_ctx* c, const EventRec* ev, uint32_t n, const PyrDesc& ts, int set, bool marked) {
  if (c->detector == ESVIO_FE_DETECT_FAST) return run_fast_cand(c, ts, set);
  run_arc(c, ev, n, &ts, false, false, true, set, marked);
  compact_set(c, c->cand[set], (n + kArcBlock - 1) / kArcBlock, true);
  return 0;
}

// wait for the main stream with a short busy poll first: the two per-frame host syncs are on the
// critical path and an interrupt-driven hipStreamSynchronize wakes up tens of microseconds late
hipError_t sync_main(esvio_fe_ctx* c) {
  for (int i = 0; i < 20000; i++) {
    const hipError_t e = hipStreamQuery(c->stream);
    if (e == hipSuccess) return hipSuccess;
    if (e != hipErrorNotReady) return e;
  }
  return hipStreamSynchronize(c->stream);
}

hipError_t sync_event(hipEvent_t ev) {
  for (int i = 0; i < 20000; i++) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return hipSuccess;
    if (e != hipErrorNotReady) return e;
  }
  return hipEventSynchronize(ev);
}

}  // namespace fe
}  // namespace esvio
