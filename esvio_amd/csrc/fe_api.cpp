// fe_api.cpp — the C ABI (include/esvio_fe.h): handle lifetime and the entry points, each a thin
// layer over fe_stages.cpp / fe_track.cpp / fe_image.cpp.
#include "fe_internal.h"

// RCCL is looked up at run time (dlopen librccl.so), so the library does not depend on it unless the
// exchange entry points are used.
namespace {
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int /*ncclDataType_t*/, void* /*ncclComm_t*/,
                                 hipStream_t);
struct NcclId {
  char internal[128];  // ncclUniqueId
};
typedef int (*nccl_get_id_fn)(NcclId*);
typedef int (*nccl_init_rank_fn)(void** /*ncclComm_t* */, int, NcclId, int);
typedef int (*nccl_destroy_fn)(void*);
// an RCCL that is already in the process (e.g. the one a PyTorch process group uses) is preferred
// to loading a second one
void* rccl_lib() {
  static void* lib = []() -> void* {
    const char* names[] = {"librccl.so.1", "librccl.so"};
    for (const char* n : names)
      if (void* l = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL)) return l;
    for (const char* n : names)
      if (void* l = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) return l;
    return dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  }();
  return lib;
}
template <class F>
F rccl_sym(const char* name) {
  void* l = rccl_lib();
  return l ? (F)dlsym(l, name) : nullptr;
}
nccl_allgather_fn rccl_all_gather() {
  static nccl_allgather_fn fn = rccl_sym<nccl_allgather_fn>("ncclAllGather");
  return fn;
}
int exchange_buffers(esvio_fe_ctx* c, int world) {
  const size_t cnt = (size_t)2 * std::max(c->cfg.max_cnt, 1) * 8;
  if (!c->x_pin) {
    if (int rc = c->x_send.alloc(c, cnt)) return rc;
    if (int rc = c->x_pin.alloc(c, cnt)) return rc;
  }
  if ((size_t)world * cnt > c->x_pin_recv.cap) {  // (the pair's second: both are there)
    c->x_pin_recv.release();
    if (int rc = c->x_recv.alloc(c, (size_t)world * cnt)) return rc;
    if (int rc = c->x_pin_recv.alloc(c, (size_t)world * cnt)) return rc;
  }
  return 0;
}
}  // namespace


// ==================================================================================== C ABI
// the ESVIO_FE_TRACE summary of a handle's life
static void print_trace_summary(const esvio_fe_ctx* c) {
  if (!c->trace || !c->phase_frames) return;
  for (int pub = 0; pub < 2; pub++) {
    if (!c->phase_count[pub]) continue;
    double tot = 0;
    fprintf(stderr, "[esvio_fe trace] %llu %s frames, ms/frame:", (unsigned long long)c->phase_count[pub],
            pub ? "published" : "unpublished");
    for (int i = PH_ENQ_BATCH; i <= PH_TAIL; i++) {
      fprintf(stderr, " %s=%.3f", kPhaseNames[i], c->trace_phase_ms[pub][i] / c->phase_count[pub]);
      tot += c->trace_phase_ms[pub][i] / c->phase_count[pub];
    }
    fprintf(stderr, " | total=%.3f\n", tot);
  }
  if (c->phase_count[1]) {
    fprintf(stderr, "[esvio_fe trace] published frames, parts of 'host mask + enqueue', ms/frame:");
    for (int i = PH_PUB_SETMASK; i <= PH_PUB_PREFETCH; i++)
      fprintf(stderr, " %s=%.3f", kPhaseNames[i] + strlen("pub: "), c->trace_phase_ms[1][i] / c->phase_count[1]);
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "[esvio_fe trace]");
  fprintf(stderr, "\n[esvio_fe trace] findFundamentalMat alone: %.3f ms per published frame (slowest call %.3f ms, "
          "%.3f without it); the two liftProjective batches before it: %.3f ms",
          c->phase_count[1] ? c->tr_fm_ms / c->phase_count[1] : 0.0, c->tr_fm_max_ms,
          c->phase_count[1] > 1 ? (c->tr_fm_ms - c->tr_fm_max_ms) / (c->phase_count[1] - 1) : 0.0,
          c->phase_count[1] ? c->tr_lift_ms / c->phase_count[1] : 0.0);
  for (int pub = 0; pub < 2; pub++)
    if (c->phase_count[pub])
      fprintf(stderr, "\n[esvio_fe trace] %s frames, host bookkeeping, ms/frame: left undistort + velocity=%.4f previous "
              "frames' right tails=%.4f this frame's right tail=%.4f copies + profile + exchange=%.4f",
              pub ? "published" : "unpublished", c->tail_ms[pub][0] / c->phase_count[pub],
              c->tail_ms[pub][1] / c->phase_count[pub], c->tail_ms[pub][2] / c->phase_count[pub],
              c->tail_ms[pub][3] / c->phase_count[pub]);
  fprintf(stderr, "\n[esvio_fe trace] rejectWithF_event calls by point count: %llu with < 8 (skipped), %llu with "
          "8..14 (LMedS, 300 hypotheses), %llu with >= 15 (RANSAC)", (unsigned long long)c->tr_fm_class[0],
          (unsigned long long)c->tr_fm_class[1], (unsigned long long)c->tr_fm_class[2]);
  if (c->tr_gpu_n)
    fprintf(stderr, "\n[esvio_fe trace] device: k_select %.1f us; select end -> next frame's temporal LK done "
            "%.1f us, -> chained one done %.1f us (its frame's pyramids: %.1f us); host: select launch -> "
            "chained results read %.1f us",
            1e3 * c->tr_gpu_sel / c->tr_gpu_n, 1e3 * c->tr_gpu_spec / c->tr_gpu_n,
            1e3 * c->tr_gpu_chain / c->tr_gpu_n, 1e3 * c->tr_gpu_pyr / c->tr_gpu_n,
            1e3 * c->tr_host_chain / c->tr_gpu_n);
  fprintf(stderr, "\n[esvio_fe trace] chained temporal LK: %llu launched, %llu used, %llu cancelled",
          (unsigned long long)c->tr_chain_launch, (unsigned long long)c->tr_chain_used,
          (unsigned long long)c->tr_chain_cancel);
  fprintf(stderr, "\n[esvio_fe trace] survivors/frame=%.1f; detect frames=%llu: candidates/frame=%.0f new/frame=%.1f\n",
          (double)c->tr_surv / c->phase_frames, (unsigned long long)c->tr_detect,
          c->tr_detect ? (double)c->tr_cand / c->tr_detect : 0.0,
          c->tr_detect ? (double)c->tr_new / c->tr_detect : 0.0);
}

extern "C" {

const char* esvio_fe_version(void) { return "esvio_fe 0.1 (gfx950)"; }

const char* esvio_fe_last_error(esvio_fe_handle h) { return h ? h->err.c_str() : "null handle"; }

int esvio_fe_destroy(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  (void)hipSetDevice(c->dev);
  (void)launcher_set(c, false);
  for (hipStream_t st : {(hipStream_t)c->stream3, (hipStream_t)c->stream4, (hipStream_t)c->stream6,
                         (hipStream_t)c->stream2, (hipStream_t)c->stream})
    if (st) (void)hipStreamSynchronize(st);
  host::ransac_pool_destroy(c->pool);
  c->pool = nullptr;
  stager_destroy(c);
  print_trace_summary(c);
  if (c->x_pending) (void)hipEventSynchronize(c->x_done);
  if (c->x_comm)  // (before the stream it runs on)
    if (nccl_destroy_fn destroy = rccl_sym<nccl_destroy_fn>("ncclCommDestroy")) (void)destroy(c->x_comm);
  delete c;  // (every buffer, event and stream: fe_res.h)
  return 0;
}

int esvio_fe_create(const esvio_fe_config* cfg, esvio_fe_handle* out) {
  if (!cfg || !out) return ESVIO_FE_EINVAL;
  *out = nullptr;
  if (cfg->width < 2 * kLkWin || cfg->height < 2 * kLkWin || cfg->width > 8192 || cfg->height > 8192)
    return ESVIO_FE_EINVAL;
  if (cfg->max_cnt < 1 || cfg->max_cnt > 65536) return ESVIO_FE_EINVAL;
  if (cfg->min_dist < 3 || cfg->min_dist > kMaxDiscR) return ESVIO_FE_EINVAL;  // Arc* ring r=4
  if (cfg->lk_accum != 1 && cfg->lk_accum != 2) return ESVIO_FE_EINVAL;
  if (cfg->median_blur_kernel_size < 0) return ESVIO_FE_EINVAL;
  if (cfg->median_blur_kernel_size > kMaxMedianK) return ESVIO_FE_ENOTIMPL;  // ksize > 15
  if (cfg->equalize != 0 && cfg->equalize != 1) return ESVIO_FE_EINVAL;
  if (!(cfg->decay_ms > 0)) return ESVIO_FE_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ESVIO_FE_ENODEVICE;
  int dev = cfg->device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return ESVIO_FE_ENODEVICE;
  }
  if (dev >= ndev) return ESVIO_FE_ENODEVICE;
  if (hipSetDevice(dev) != hipSuccess) return ESVIO_FE_ENODEVICE;

  esvio_fe_ctx* c = new esvio_fe_ctx();
  c->cfg = *cfg;
  c->dev = dev;
  c->W = cfg->width;
  c->H = cfg->height;
  c->P = (uint32_t)c->W * c->H;
  c->invalid_key = 2 * c->P;
  c->key_bits = 1;
  while ((1ull << c->key_bits) <= (unsigned long long)c->invalid_key) c->key_bits++;
  c->hw = host::disc_halfwidths(cfg->min_dist);
  c->trace = getenv("ESVIO_FE_TRACE") != nullptr;
  if (const char* v = getenv("ESVIO_FE_SLOW_CALL_MS")) c->slow_call_ms = atof(v);
  c->mask_event.reset(c->W, c->H);

  auto bail = [&](int rc) {
    esvio_fe_destroy(c);
    return rc;
  };
  // the frame's own chain (LK, selection: few, latency-bound waves) outranks the prefetch stream's
  // wide kernels, which have a whole frame of slack
  {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) {
      (void)hipGetLastError();
      n_cu = 64;  // (unknown: assume a small device)
    }
    const int lk_blocks = (std::max(cfg->max_cnt, 1) + kLkPointsPerBlock - 1) / kLkPointsPerBlock;
    c->n_cu = n_cu;
    c->waits_fit_spec = lk_blocks + 2 <= n_cu;
    c->waits_fit_chain = 2 * lk_blocks + 2 <= n_cu;
  }
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (c->stream.create(hipStreamNonBlocking, prio_greatest) != hipSuccess ||
      c->stream2.create(hipStreamNonBlocking, prio_least) != hipSuccess ||
      c->stream3.create(hipStreamNonBlocking, prio_greatest) != hipSuccess ||
      c->stream4.create(hipStreamNonBlocking, prio_least) != hipSuccess)
    return bail(ESVIO_FE_EHIP);
  {
    const unsigned timed = c->trace ? 0 : hipEventDisableTiming;  // (the trace reads intervals off these)
    const std::pair<Event*, unsigned> evs[] = {
        {&c->ev_pts_ready, hipEventDisableTiming},  {&c->ev_spec_done, timed},
        {&c->ev_chain_done, timed},                 {&c->ev_dbg_sel_start, 0},
        {&c->ev_sel_host, timed},                   {&c->ev_lks_done[0], hipEventDisableTiming},
        {&c->ev_lks_done[1], hipEventDisableTiming}, {&c->ev_lknew_done, hipEventDisableTiming},
        {&c->ev_planes_free, hipEventDisableTiming}, {&c->ev_imgs_ready, hipEventDisableTiming},
        {&c->ev_arc_side, hipEventDisableTiming},   {&c->ev_sae_left, hipEventDisableTiming},
        {&c->ev_right_ready, hipEventDisableTiming}};
    for (const auto& ef : evs)
      if (ef.first->create(ef.second) != hipSuccess) return bail(ESVIO_FE_EHIP);
    for (int i = 0; i < kPrefetchDepth; i++)
      if (c->ev_lane_done[i].create(timed) != hipSuccess || c->ev_lane_arc[i].create() != hipSuccess)
        return bail(ESVIO_FE_EHIP);
  }
  const size_t M = cfg->max_cnt;
  const int Mc = cfg->max_cnt;
  int rc = 0;
  if ((rc = c->L2.alloc(c, (size_t)2 * c->P))) return bail(rc);
  if ((rc = c->S2.alloc(c, (size_t)2 * c->P))) return bail(rc);
  if ((rc = c->d_rejected.alloc(c, 1))) return bail(rc);
  if ((rc = c->d_res.alloc(c, res_layout(Mc).total))) return bail(rc);
  c->dres = res_view(c->d_res, Mc, 0);
  c->dres.mask = nullptr;
  {
    // (the speculative launch's block, then the chained launch's)
    uint8_t* z_spec = nullptr;
    const size_t bytes = kSpecBlocks * spec_layout(Mc).bytes;
    if ((rc = c->h_spec.alloc(c, bytes))) return bail(rc);
    if (hipHostGetDevicePointer((void**)&z_spec, c->h_spec, 0) != hipSuccess) return bail(ESVIO_FE_EHIP);
    std::memset(c->h_spec, 0, bytes);
    for (int b = 0; b < kSpecBlocks; b++) {
      c->hspec[b] = spec_view(c->h_spec, Mc, b);
      c->zspec[b] = spec_view(z_spec, Mc, b);
    }
  }
  if ((rc = c->d_chain.alloc(c, 2 * std::max<size_t>(M, 1)))) return bail(rc);
  if ((rc = c->d_lane_gate.alloc(c, 16))) return bail(rc);
  c->stage_threads = stager_threads_from_env();
  if (const char* v = getenv("ESVIO_FE_FAULT")) esvio_fe_debug_inject(c, atoi(v));
  if (const char* e = getenv("ESVIO_FE_STEREO_SPLIT")) c->stereo_split_env = atoi(e) != 0;  // (else: fe_track.cpp decides)
  c->chain_enabled = getenv("ESVIO_FE_NO_CHAIN") == nullptr;
  c->cam_split_enabled = getenv("ESVIO_FE_NO_CAMSPLIT") == nullptr;
  // (the per-pixel dedup of the Arc* candidates pays only where the selection digs deep into its list: fe_stages.cpp run_arc)
  c->dedup_enabled = getenv("ESVIO_FE_NO_DEDUP") == nullptr && (cfg->max_cnt > 500 || getenv("ESVIO_FE_DEDUP") != nullptr);
  c->fuse_ts_pyr = getenv("ESVIO_FE_NO_FUSE") == nullptr;
  if (const char* v = getenv("ESVIO_FE_CONVERT_PINNED_COPY")) c->cvt_pinned_copy = atoi(v) != 0 ? 1 : 0;
  if (const char* v = getenv("ESVIO_FE_RAW_PINNED_COPY")) c->rawdec.pinned_copy = atoi(v) != 0 ? 1 : 0;
  c->select_one_wave = getenv("ESVIO_FE_SELECT_SERIAL") != nullptr;
  if (const char* v = getenv("ESVIO_FE_SAE_EV_MIN")) c->sae_ev_min = (size_t)strtoull(v, nullptr, 10);
  c->tiled = make_tile_geom(c->W, c->H, &c->tgeom) && getenv("ESVIO_FE_SAE_SORT") == nullptr;
  for (int i = 0; i < kRightSlots; i++)
    if ((rc = c->d_first[i].alloc(c, (size_t)c->P))) return bail(rc);
  for (int i = 0; i < kRightSlots; i++) {
    const size_t words = arc_bitmap_words(c->W, c->H);
    if ((rc = c->d_cmap[i].alloc(c, words))) return bail(rc);
    if ((rc = c->d_touched[i].alloc(c, arc_flag_bytes(c->W, c->H)))) return bail(rc);
    if (hipMemsetAsync(c->d_cmap[i], 0, words * 4, cur_stream(c)) != hipSuccess ||
        hipMemsetAsync(c->d_touched[i], 0, arc_flag_bytes(c->W, c->H), cur_stream(c)) != hipSuccess)
      return bail(ESVIO_FE_EHIP);
  }
  if ((rc = c->d_pub_slots.alloc(c, std::max<size_t>(M, 1)))) return bail(rc);
  if ((rc = c->d_pub_done.alloc(c, 1))) return bail(rc);
  if (hipMemsetAsync(c->d_lane_gate, 0, 64, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->d_chain, 0, std::max<size_t>(M, 1) * 16, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->d_pub_slots, 0, std::max<size_t>(M, 1) * 8, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->d_pub_done, 0, 8, cur_stream(c)) != hipSuccess)
    return bail(ESVIO_FE_EHIP);
  if ((rc = c->d_ptsD.alloc(c, M))) return bail(rc);
  if ((rc = c->d_sel_idx.alloc(c, M))) return bail(rc);
  if ((rc = c->d_mask_bits.alloc(c, (size_t)c->H * ((c->W + 31) / 32)))) return bail(rc);
  for (PyrStore& ps : c->pyr)
    if ((rc = pyr_alloc(c, ps, c->W, c->H, 3))) return bail(rc);
  if (cfg->median_blur_kernel_size > 0)
    for (PyrStore& ps : c->med_tmp)
      if ((rc = pyr_alloc(c, ps, c->W, c->H, 0))) return bail(rc);
  if (cfg->equalize) {
    for (auto& rb : c->raw)
      for (PyrStore& ps : rb)
        if ((rc = pyr_alloc(c, ps, c->W, c->H, 0))) return bail(rc);
    if ((rc = c->d_lut.alloc(c, (size_t)2 * 64 * 256))) return bail(rc);
    // (CLAHE scratch: d_lut, d_minmax and d_eq_tmp are single buffers shared by the main stream and the
    // prefetch stream; rendering on one is ordered behind the other's through ev_planes_free /
    // ev_lane_done, like the SAE planes they are derived from)
    if ((rc = c->d_eq_tmp.alloc(c, (size_t)2 * c->P))) return bail(rc);
    if ((rc = c->d_minmax.alloc(c, 4))) return bail(rc);
  }
  {
    uint8_t* z_res = nullptr;
    if ((rc = c->h_pin.alloc(c, pin_bytes(Mc, cfg->width, cfg->height)))) return bail(rc);
    if (hipHostGetDevicePointer((void**)&z_res, c->h_pin, 0) != hipSuccess) return bail(ESVIO_FE_EHIP);
    std::memset(c->h_pin, 0, c->h_pin.cap);
    for (int s = 0; s < 2; s++) {
      c->pin[s] = res_view(c->h_pin, Mc, s);
      c->zpin[s] = res_view(z_res, Mc, s);
    }
  }
  if (hipMemsetAsync(c->L2, 0, (size_t)2 * c->P * 16, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->S2, 0, (size_t)2 * c->P * 16, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->d_rejected, 0, 8, cur_stream(c)) != hipSuccess ||
      hipMemsetAsync(c->dres.counts, 0, 64, cur_stream(c)) != hipSuccess ||
      hipStreamSynchronize(cur_stream(c)) != hipSuccess)
    return bail(ESVIO_FE_EHIP);
  // One kernel of this library on every stream, now: the runtime loads the code object with the first
  // launch from it and creates a stream's hardware queue with the stream's first use — 2.0-2.4 ms that
  // would otherwise sit inside the first esvio_fe_track_event call (profiles/r04_stall_forensics.md).
  const hipStream_t st[4] = {c->stream, c->stream2, c->stream3, c->stream4};
  for (hipStream_t s : st) {
    launch_fill_f64(s, (double*)c->d_rejected, 1, 0.0);
    if (hipStreamSynchronize(s) != hipSuccess) return bail(ESVIO_FE_EHIP);
  }
  // ... and a burst of launches chained across the streams by events, nothing of it awaited until the end.  What it
  // is for: in one cold bench process of ten ONE track call around frame 20 of the first timed pass took 1.6-4.7 ms,
  // inside a HIP launch call of the calling thread or in its wait for the launch thread — never a lost CPU, never an
  // allocation of ours (profiles/r05_stall_hunt.txt).  Read as the runtime growing a pool (completion signals,
  // command records) inside whichever launch needs one more than it has; the replay schedule keeps ~60 launches and
  // ~25 cross-stream waits in flight, this puts 4 x 96 launches and as many waits in flight at once — and 30 cold
  // processes then ran without one call above 0.6 ms (profiles/r05_stall_hunt_after.txt).
  {
    Event ev[4];  // (events of the warm-up's own: the handle's stay unrecorded until a frame records them)
    bool ok = true;
    for (int i = 0; i < 4; i++) ok = ok && ev[i].create() == hipSuccess;
    for (int r = 0; ok && r < 96; r++)
      for (int i = 0; ok && i < 4; i++) {
        launch_spin(st[i], r == 0 ? 20000 : 0);  // (the first round's kernels hold everything behind them for 200 us)
        ok = hipEventRecord(ev[i], st[i]) == hipSuccess && hipStreamWaitEvent(st[(i + 1) & 3], ev[i], 0) == hipSuccess;
      }
    for (int i = 0; i < 4; i++) ok = (hipStreamSynchronize(st[i]) == hipSuccess) && ok;
    if (!ok) return bail(ESVIO_FE_EHIP);
  }
  if ((rc = stereo_split_prepare(c))) return bail(rc);  // (ESVIO_FE_STEREO_SPLIT=1)
  // Which of these streams share a hardware queue?  The runtime hands out at most GPU_MAX_HW_QUEUES (4) queues per
  // priority level and process, then doubles up — and two streams on one queue run their kernels one after the
  // other (tools/queue_probe.hip), which for this schedule means a frame's prefetch behind another frame's waiting
  // LK launch.  Counted once per handle (a 100 us spin on one stream, an empty kernel on the other: ~1.2 ms for
  // the ten pairs), reported by esvio_fe_debug_counters and, with ESVIO_FE_QUEUE_PROBE=1, on stderr.
  if (getenv("ESVIO_FE_QUEUE_PROBE")) {
    const hipStream_t st[5] = {c->stream, c->stream2, c->stream3, c->stream4, c->stream6};  // (stream6: only where the handle splits)
    const char* nm[5] = {"main", "prefetch", "speculative", "stereo", "stereo-unpublished"};
    const int ns = c->stream6 ? 5 : 4;
    for (int a = 0; a < ns; a++)
      for (int b = 0; b < ns; b++) {
        if (a == b || st[a] == st[b]) continue;
        launch_spin(st[a], 10000);
        const auto t0 = std::chrono::steady_clock::now();
        launch_fill_f64(st[b], (double*)c->d_rejected, 1, 0.0);
        (void)hipStreamSynchronize(st[b]);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        (void)hipStreamSynchronize(st[a]);
        if (us > 60.0) {
          c->n_queue_conflicts++;
          fprintf(stderr, "[esvio_fe] streams '%s' and '%s' share a hardware queue (%.0f us behind a 100 us kernel)\n", nm[b], nm[a], us);
        }
      }
    if (!c->n_queue_conflicts) fprintf(stderr, "[esvio_fe] the handle's %d streams have a hardware queue each\n", ns);
  }
  // The greedy selections (Event_FeaturesToTrack, goodFeaturesToTrack's min-distance pass) keep
  // their one-bit-per-pixel map in LDS; above ~1.3 M pixels (the frame cameras of the shipped ESVIO
  // configs go up to 1920x1200) it lives in device memory instead (k_select_gbm)
  c->select_ok = select_lds_bytes(c) <= 160 * 1024;
  if (!c->select_ok && (rc = c->d_sel_bitmap.alloc(c, (size_t)c->H * ((c->W + 31) / 32) + 4))) return bail(rc);
  *out = c;
  return 0;
}

namespace {
int baf_clear(esvio_fe_ctx* c);  // the background-activity filter's planes back to `none` (below, with the stage)
int hot_clear(esvio_fe_ctx* c);  // hot-pixel learning: nothing counted (below, with the stage)
int baf_ensure(esvio_fe_ctx* c, size_t n, bool host_src, bool host_dst, bool fields_form);
void decode_state_reset(esvio_fe_ctx* c);  // every ingest stage's decoder / walker state: fresh (below, behind the stages)
void feed_empty(esvio_fe_ctx* c, bool streams_idle);  // the feed: no records, no windows (below, with the feed)
}  // namespace

int esvio_fe_reset(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  (void)launcher_drain(c);  // (whatever it was still issuing is discarded with the batches below)
  launcher_clear_error(c);
  HIPCHK(c, hipStreamSynchronize(c->stream3));
  HIPCHK(c, hipStreamSynchronize(c->stream4));
  if (c->stream6) HIPCHK(c, hipStreamSynchronize(c->stream6));
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  // (the main stream as well: a call that returned early in lazy mode, or one that failed half way,
  // may have kernels there that still raise the error flag or write into the pinned result words
  // cleared below)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->announced.clear();
  c->inflight.clear();
  stager_drain(c);
  c->cur_stage = -1;
  // (a call that failed with ESVIO_FE_EINTERNAL: the expired wait's flag, the sort's scratch words)
  c->pin[0].counts[3] = 0;
  if (c->hist) HIPCHK(c, hipMemsetAsync(c->hist, 0, c->hist.cap * 4, cur_stream(c)));
  std::memset(c->h_spec, 0, kSpecBlocks * spec_layout(c->cfg.max_cnt).bytes);
  c->spec_valid = false;
  c->chain_valid = false;
  c->chain_map_ok = false;
  c->pend.active = false;
  c->pend_right.active = false;
  HIPCHK(c, hipMemsetAsync(c->L2, 0, (size_t)2 * c->P * 16, cur_stream(c)));
  HIPCHK(c, hipMemsetAsync(c->S2, 0, (size_t)2 * c->P * 16, cur_stream(c)));
  if (c->evimg.on)  // the event images: zero (the setting is kept)
    if (int rc = evimg_zero(c, true)) return rc;
  if (int rc = baf_clear(c)) return rc;  // the background-activity filter's planes: none everywhere
  if (int rc = hot_clear(c)) return rc;  // hot-pixel learning: nothing counted (the address filter and the mask are settings: kept)
  decode_state_reset(c);  // the raw-stream and trigger decoders, the AEDAT and bag walkers (the topics are settings: kept)
  c->slice.st[0] = c->slice.st[1] = esvio_fe_ctx::Slice::State();  // the stream slicer: no event seen, no window closed
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  feed_empty(c, true);  // an open feed: no records, no windows (it stays open); every stream is idle here
  clear_tracker_state(c);
  return 0;
}

// esvio_fe_create_sae_stereo and its motion-compensated form (mc != nullptr) behind their argument checks
static int create_sae_stereo(esvio_fe_ctx* c, const esvio_fe_event* left, size_t nL, const esvio_fe_event* right,
                             size_t nR, int space, const McParams* mc, uint64_t* n_rejected) {
  if (nL + nR >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  if (!c->inflight.empty()) return fail(c, ESVIO_FE_EINVAL, "a prefetched batch is pending");
  HIPCHK(c, hipSetDevice(c->dev));
  c->ext_sae_pending = false;  // (the planes move on: a committed time-sliced batch is not "the next frame's" any more)
  const EventRec *dL, *dR;
  if (int rc = stage_events(c, left, nL, right, nR, space, &dL, &dR)) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_rejected, 0, 8, cur_stream(c)));
  c->evimg.fresh_cams = 0;  // (a stage call accumulates into the event images)
  if (int rc = sae_update(c, dL, (uint32_t)nL, dR, (uint32_t)nR, mc)) return rc;
  unsigned long long rej = 0;
  HIPCHK(c, hipMemcpyAsync(&rej, c->d_rejected, 8, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (int rc = lookback_expired(c)) return rc;
  if (n_rejected) *n_rejected = rej;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_create_sae_stereo(esvio_fe_handle c, const esvio_fe_event* left, size_t nL,
                               const esvio_fe_event* right, size_t nR, int space,
                               uint64_t* n_rejected) {
  if (!c || (nL && !left) || (nR && !right)) return ESVIO_FE_EINVAL;
  return create_sae_stereo(c, left, nL, right, nR, space, nullptr, n_rejected);
}

int esvio_fe_create_sae_stereo_mc(esvio_fe_handle c, const esvio_fe_event* left, size_t nL,
                                  const esvio_fe_event* right, size_t nR, int space,
                                  const esvio_fe_motion* motion, uint64_t* n_rejected) {
  if (!c || !motion || !nL || !left || (nR && !right)) return ESVIO_FE_EINVAL;
  const McParams mc = make_mc_params(motion);
  return create_sae_stereo(c, left, nL, right, nR, space, &mc, n_rejected);
}

// ---- one stream time-sliced across GPUs -----------------------------------------
namespace {
int slice_scratch(esvio_fe_ctx* c) {
  if (c->S2s) return 0;  // (the second of the two: both are there)
  if (int rc = c->L2s.alloc(c, (size_t)2 * c->P)) return rc;
  return c->S2s.alloc(c, (size_t)2 * c->P);
}
// device address of `k` consecutive plane sets given in `space` (host ones are staged)
int slice_planes_in(esvio_fe_ctx* c, const double* p, size_t sets, int space, const double** dev) {
  const size_t nd = sets * 4 * (size_t)c->P;
  if (space == ESVIO_FE_DEVICE || !nd) {
    *dev = p;
    return 0;
  }
  if (space != ESVIO_FE_HOST) return fail(c, ESVIO_FE_EINVAL, "bad memory space %d", space);
  if (nd > c->slice_stage.cap)
    if (int rc = c->slice_stage.alloc(c, nd)) return rc;
  HIPCHK(c, hipMemcpyAsync(c->slice_stage, p, nd * 8, hipMemcpyHostToDevice, cur_stream(c)));
  *dev = c->slice_stage;
  return 0;
}
int slice_planes_out(esvio_fe_ctx* c, const double2* src, double* out, int space) {
  const size_t bytes = (size_t)4 * c->P * 8;
  HIPCHK(c, hipMemcpyAsync(out, src, bytes, space == ESVIO_FE_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                           cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (int rc = lookback_expired(c)) return rc;
  return 0;
}
}  // namespace

size_t esvio_fe_sae_plane_doubles(esvio_fe_handle c) { return c ? (size_t)4 * c->P : 0; }

int esvio_fe_sae_slice_last(esvio_fe_handle c, const esvio_fe_event* left, size_t nL,
                            const esvio_fe_event* right, size_t nR, int space, double* last_out,
                            int out_space) {
  if (!c || !last_out || (nL && !left) || (nR && !right)) return ESVIO_FE_EINVAL;
  if (nL + nR >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "time-sliced SAE update cannot be mixed with esvio_fe_set_next_batch");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = slice_scratch(c)) return rc;
  // A rank that never tracks: the previous batch's commit simply IS its planes by now.  On a rank that
  // tracks, a committed batch must get its track call before the next batch's slices start — the call
  // would otherwise apply the batch to the planes a second time.
  if (c->ext_sae_pending && c->frame_no > 0)
    return fail(c, ESVIO_FE_EINVAL, "the committed batch has not been tracked yet (slice_last of the next batch "
                                    "comes after esvio_fe_track_event on a rank that tracks)");
  c->ext_sae_pending = false;
  const EventRec *dL, *dR;
  if (int rc = stage_events(c, left, nL, right, nR, space, &dL, &dR)) return rc;
  // L[p] is overwritten by every event whatever the carried-in state is (event_detector.cc:158), so
  // the slice's last event time per (pixel, polarity) is what the ordinary update leaves in planes
  // that start out as "nothing"
  launch_fill_f64(cur_stream(c), (double*)c->L2s, (size_t)4 * c->P, kSliceNone);
  launch_fill_f64(cur_stream(c), (double*)c->S2s, (size_t)4 * c->P, kSliceNone);
  if (int rc = sae_update(c, dL, (uint32_t)nL, dR, (uint32_t)nR, nullptr, c->L2s, c->S2s)) return rc;
  return slice_planes_out(c, c->L2s, last_out, out_space);
}

int esvio_fe_sae_slice_apply(esvio_fe_handle c, const esvio_fe_event* left, size_t nL,
                             const esvio_fe_event* right, size_t nR, int space,
                             const double* last_before, int n_before, int in_space, double* s_out,
                             int out_space) {
  if (!c || !s_out || n_before < 0 || (n_before && !last_before) || (nL && !left) || (nR && !right))
    return ESVIO_FE_EINVAL;
  if (nL + nR >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "time-sliced SAE update cannot be mixed with esvio_fe_set_next_batch");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = slice_scratch(c)) return rc;
  const size_t nd = (size_t)4 * c->P;
  // carried-in L = the planes before the batch overlaid with the earlier slices in stream order;
  // with it every pass decision of this slice is the sequential loop's (S never enters a decision)
  HIPCHK(c, hipMemcpyAsync(c->L2s, c->L2, nd * 8, hipMemcpyDeviceToDevice, cur_stream(c)));
  const double* dl = nullptr;
  if (int rc = slice_planes_in(c, last_before, (size_t)n_before, in_space, &dl)) return rc;
  for (int k = 0; k < n_before; k++)
    launch_overlay_f64(cur_stream(c), (double*)c->L2s, dl + (size_t)k * nd, nd, kSliceNone);
  launch_fill_f64(cur_stream(c), (double*)c->S2s, nd, kSliceNone);
  const EventRec *dL, *dR;
  if (int rc = stage_events(c, left, nL, right, nR, space, &dL, &dR)) return rc;
  if (int rc = sae_update(c, dL, (uint32_t)nL, dR, (uint32_t)nR, nullptr, c->L2s, c->S2s)) return rc;
  return slice_planes_out(c, c->S2s, s_out, out_space);
}

int esvio_fe_sae_slice_commit(esvio_fe_handle c, const double* last_all, const double* s_all, int n_slices,
                              int space) {
  if (!c || n_slices < 1 || !last_all || !s_all) return ESVIO_FE_EINVAL;
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "time-sliced SAE update cannot be mixed with esvio_fe_set_next_batch");
  HIPCHK(c, hipSetDevice(c->dev));
  const size_t nd = (size_t)4 * c->P;
  for (int pass = 0; pass < 2; pass++) {  // (one staging buffer: L first, then S)
    const double* dp = nullptr;
    if (int rc = slice_planes_in(c, pass ? s_all : last_all, (size_t)n_slices, space, &dp)) return rc;
    double* dst = pass ? (double*)c->S2 : (double*)c->L2;
    for (int k = 0; k < n_slices; k++) launch_overlay_f64(cur_stream(c), dst, dp + (size_t)k * nd, nd, kSliceNone);
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  }
  c->ext_sae_pending = true;
  return 0;
}

int esvio_fe_create_sae(esvio_fe_handle c, int cam, const esvio_fe_event* ev, size_t n, int space,
                        uint64_t* n_rejected) {
  if (cam == 0) return esvio_fe_create_sae_stereo(c, ev, n, nullptr, 0, space, n_rejected);
  if (cam == 1) return esvio_fe_create_sae_stereo(c, nullptr, 0, ev, n, space, n_rejected);
  return ESVIO_FE_EINVAL;
}

int esvio_fe_sae_to_time_surface(esvio_fe_handle c, int cam, double t_sync, uint8_t* out) {
  if (!c || (cam != 0 && cam != 1)) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->inflight.empty()) return fail(c, ESVIO_FE_EINVAL, "a prefetched batch is pending");
  render_lk_images(c, t_sync, cam ? 2 : 1, c->slot_curL, c->slot_curR, c->raw_cur);
  if (out) return copy_level0_out(c, raw_ts_desc(c, cam), out);
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_get_time_surface(esvio_fe_handle c, int cam, uint8_t* out) {
  if (!c || !out || (cam != 0 && cam != 1)) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  return copy_level0_out(c, raw_ts_desc(c, cam), out);
}

int esvio_fe_export_image(esvio_fe_handle c, int cam, uint8_t* dst, int space) {
  if (!c || !dst || (cam != 0 && cam != 1)) return ESVIO_FE_EINVAL;
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  const PyrDesc& d = cam ? c->pyr[c->slot_curR].d : c->pyr[c->slot_curL].d;
  if (space == ESVIO_FE_HOST) return copy_level0_out(c, d, dst);  // (staged: no 2-D copy over PCIe)
  const int stride = d.stride[0];
  HIPCHK(c, hipMemcpy2DAsync(dst, c->W, d.img[0] + (size_t)kPad * stride + kPad, stride, c->W, c->H,
                             hipMemcpyDeviceToDevice, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}

int esvio_fe_export_level(esvio_fe_handle c, int cam, int level, uint8_t* img, int16_t* deriv, int32_t* w,
                          int32_t* hgt, int32_t* levels) {
  if (!c || (cam != 0 && cam != 1)) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->announced.empty() || !c->inflight.empty()) return fail(c, ESVIO_FE_EINVAL, "a prefetched batch is pending");
  if (int rc = finalize_lazy(c)) return rc;
  const PyrDesc& d = cam ? c->pyr[c->slot_curR].d : c->pyr[c->slot_curL].d;
  if (level < 0 || level > d.levels) return fail(c, ESVIO_FE_EINVAL, "level %d of a pyramid of %d", level, d.levels + 1);
  if (w) *w = d.w[level];
  if (hgt) *hgt = d.h[level];
  if (levels) *levels = d.levels;
  // (the padded planes from their origin, without the bytes between the padded width and the row stride)
  const size_t pw = (size_t)d.w[level] + 2 * kPad, ph = (size_t)d.h[level] + 2 * kPad, stride = d.stride[level];
  if (img) HIPCHK(c, hipMemcpy2DAsync(img, pw, d.img[level], stride, pw, ph, hipMemcpyDeviceToHost, cur_stream(c)));
  if (deriv)
    HIPCHK(c, hipMemcpy2DAsync(deriv, pw * 4, d.deriv[level], stride * 4, pw * 4, ph, hipMemcpyDeviceToHost,
                               cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}

int esvio_fe_import_image(esvio_fe_handle c, int cam, const uint8_t* src, int space) {
  if (!c || !src) return ESVIO_FE_EINVAL;
  if (cam != 1) return fail(c, ESVIO_FE_EINVAL, "only the right camera's image can be imported");
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "import_image cannot be combined with set_next_batch");
  c->slot_curR = other_right_slot(c);  // next trackEvent's curR (its rotate_slots leaves it)
  const PyrDesc& d = c->pyr[c->slot_curR].d;
  const int stride = d.stride[0];
  if (space == ESVIO_FE_HOST) {  // (staged through pinned memory: src is free again on return)
    if (int rc = copy_level0_in(c, d, src)) return rc;
  } else {
    HIPCHK(c, hipMemcpy2DAsync(d.img[0] + (size_t)kPad * stride + kPad, stride, src, c->W, c->W, c->H,
                               hipMemcpyDeviceToDevice, cur_stream(c)));
  }
  c->ext_right_pending = true;
  return 0;
}

int esvio_fe_is_corner(esvio_fe_handle c, const esvio_fe_event* ev, size_t n, int space,
                       uint8_t* flags) {
  if (!c || (n && (!ev || !flags))) return ESVIO_FE_EINVAL;
  if (!n) return 0;
  HIPCHK(c, hipSetDevice(c->dev));
  const EventRec *dL, *dR;
  if (int rc = stage_events(c, ev, n, nullptr, 0, space, &dL, &dR)) return rc;
  if (int rc = ensure_arc_capacity(c, n, c->cand_cur)) return rc;
  run_arc(c, dL, (uint32_t)n, nullptr, false, true, false, c->cand_cur);
  HIPCHK(c, hipMemcpyAsync(flags, c->d_flags, n, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_features_to_track(esvio_fe_handle c, const esvio_fe_event* ev, size_t n, int space,
                               int max_corners, const uint8_t* mask, float* out_xy,
                               int32_t* out_idx, int32_t* n_out) {
  if (!c || !n_out || (n && !ev)) return ESVIO_FE_EINVAL;
  *n_out = 0;
  if (max_corners <= 0 || !n) return 0;
  if (max_corners > c->cfg.max_cnt) return fail(c, ESVIO_FE_EINVAL, "max_corners > max_cnt");
  if (!out_xy) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  const EventRec *dL, *dR;
  if (int rc = stage_events(c, ev, n, nullptr, 0, space, &dL, &dR)) return rc;
  if (int rc = ensure_arc_capacity(c, n, c->cand_cur)) return rc;
  const ResView& pin = c->pin[0];
  host::BitMask bm;
  bm.reset(c->W, c->H);
  if (mask) bm.from_bytes(mask);
  std::memcpy(pin.mask, bm.bits.data(), bm.bits.size() * 4);
  HIPCHK(c, hipMemcpyAsync(c->d_mask_bits, pin.mask, bm.bits.size() * 4, hipMemcpyHostToDevice,
                           cur_stream(c)));
  const PyrDesc ts = raw_ts_desc(c, 0);
  run_arc(c, dL, (uint32_t)n, &ts, true, false, true, c->cand_cur);
  compact_set(c, c->cand[c->cand_cur], ((uint32_t)n + kArcBlock - 1) / kArcBlock, true);
  run_select(c, c->cand_cur, max_corners, c->d_ptsD, 0, c->d_sel_idx);
  HIPCHK(c, hipMemcpyAsync(pin.counts, c->dres.counts, 8, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  const int k = pin.counts[0];
  if (k > 0) {
    HIPCHK(c, hipMemcpy(out_xy, c->d_ptsD, (size_t)k * 8, hipMemcpyDeviceToHost));
    if (out_idx) HIPCHK(c, hipMemcpy(out_idx, c->d_sel_idx, (size_t)k * 4, hipMemcpyDeviceToHost));
  }
  *n_out = k;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

static int planes_io(esvio_fe_handle c, int cam, double* L0, double* L1, double* S0, double* S1,
                     const double* iL0, const double* iL1, const double* iS0, const double* iS1,
                     bool set) {
  if (!c || (cam != 0 && cam != 1)) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  std::vector<double> l((size_t)2 * c->P), s((size_t)2 * c->P);
  if (set) {
    for (uint32_t i = 0; i < c->P; i++) {
      l[2 * i] = iL0[i];
      l[2 * i + 1] = iL1[i];
      s[2 * i] = iS0[i];
      s[2 * i + 1] = iS1[i];
    }
    HIPCHK(c, hipMemcpy(c->L2 + (size_t)cam * c->P, l.data(), (size_t)c->P * 16, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->S2 + (size_t)cam * c->P, s.data(), (size_t)c->P * 16, hipMemcpyHostToDevice));
  } else {
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
    HIPCHK(c, hipMemcpy(l.data(), c->L2 + (size_t)cam * c->P, (size_t)c->P * 16, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(s.data(), c->S2 + (size_t)cam * c->P, (size_t)c->P * 16, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < c->P; i++) {
      L0[i] = l[2 * i];
      L1[i] = l[2 * i + 1];
      S0[i] = s[2 * i];
      S1[i] = s[2 * i + 1];
    }
  }
  return 0;
}

int esvio_fe_get_sae(esvio_fe_handle c, int cam, double* L0, double* L1, double* S0, double* S1) {
  if (!L0 || !L1 || !S0 || !S1) return ESVIO_FE_EINVAL;
  return planes_io(c, cam, L0, L1, S0, S1, nullptr, nullptr, nullptr, nullptr, false);
}
int esvio_fe_set_sae(esvio_fe_handle c, int cam, const double* L0, const double* L1,
                     const double* S0, const double* S1) {
  if (!L0 || !L1 || !S0 || !S1) return ESVIO_FE_EINVAL;
  return planes_io(c, cam, nullptr, nullptr, nullptr, nullptr, L0, L1, S0, S1, true);
}

static int prep_tmp_pyr(esvio_fe_handle c, int slot, const uint8_t* img, int w, int hgt,
                        int max_level) {
  if (int rc = pyr_alloc(c, c->tmp_pyr[slot], w, hgt, max_level)) return rc;
  return copy_level0_in(c, c->tmp_pyr[slot].d, img);
}

int esvio_fe_calc_optical_flow_pyr_lk(esvio_fe_handle c, const uint8_t* prev_img,
                                      const uint8_t* next_img, int w, int hgt,
                                      const float* prev_pts, float* next_pts, uint8_t* status,
                                      int n, int max_level, int max_count, double eps, int flags) {
  if (!c || !prev_img || !next_img || n < 0 || (n && (!prev_pts || !next_pts || !status)))
    return ESVIO_FE_EINVAL;
  if (w < 2 * kLkWin || hgt < 2 * kLkWin || max_level < 0 || max_level >= kMaxLevels)
    return ESVIO_FE_EINVAL;
  if (n > c->cfg.max_cnt) return fail(c, ESVIO_FE_EINVAL, "n > max_cnt");
  if (!n) return 0;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = prep_tmp_pyr(c, 0, prev_img, w, hgt, max_level)) return rc;
  if (int rc = prep_tmp_pyr(c, 1, next_img, w, hgt, max_level)) return rc;
  PyrDesc two[2] = {c->tmp_pyr[0].d, c->tmp_pyr[1].d};
  pyr_build(c, two, 2);
  float2 *d_prev = (float2*)c->dres.A, *d_next = (float2*)c->dres.s1.fwd;
  uint8_t* d_st = c->dres.s1.st_fwd;
  HIPCHK(c, hipMemcpyAsync(d_prev, prev_pts, (size_t)n * 8, hipMemcpyHostToDevice, cur_stream(c)));
  if (flags & ESVIO_FE_LK_USE_INITIAL_FLOW)
    HIPCHK(c, hipMemcpyAsync(d_next, next_pts, (size_t)n * 8, hipMemcpyHostToDevice, cur_stream(c)));
  LkArgs f = make_lk(two[0], two[1], d_prev, d_next, d_next, d_st, nullptr, n, max_level, max_count, eps, flags);
  run_lk(c, f, nullptr, nullptr, nullptr);
  HIPCHK(c, hipMemcpyAsync(next_pts, d_next, (size_t)n * 8, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipMemcpyAsync(status, d_st, (size_t)n, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_build_pyramid(esvio_fe_handle c, const uint8_t* img, int w, int hgt, int max_level,
                           int level, uint8_t* out_img, int16_t* out_deriv, int32_t* lw,
                           int32_t* lh, int32_t* n_levels) {
  if (!c || !img || max_level < 0 || max_level >= kMaxLevels || w < 2 * kLkWin || hgt < 2 * kLkWin)
    return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = prep_tmp_pyr(c, 0, img, w, hgt, max_level)) return rc;
  const PyrDesc& d = c->tmp_pyr[0].d;
  pyr_build(c, &d, 1);
  if (n_levels) *n_levels = d.levels + 1;
  if (level < 0 || level > d.levels) {
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
    return level < 0 ? 0 : ESVIO_FE_EINVAL;
  }
  if (lw) *lw = d.w[level];
  if (lh) *lh = d.h[level];
  const int stride = d.stride[level];
  if (out_img)
    HIPCHK(c, hipMemcpy2DAsync(out_img, d.w[level], d.img[level] + (size_t)kPad * stride + kPad,
                               stride, d.w[level], d.h[level], hipMemcpyDeviceToHost, cur_stream(c)));
  if (out_deriv)
    HIPCHK(c, hipMemcpy2DAsync(out_deriv, (size_t)d.w[level] * 4,
                               d.deriv[level] + ((size_t)kPad * stride + kPad) * 2, (size_t)stride * 4,
                               (size_t)d.w[level] * 4, d.h[level], hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_find_fundamental_mat(const float* p1, const float* p2, int n, double thr, double conf,
                                  uint8_t* status, int32_t* n_inliers) {
  if (n < 0 || (n && (!p1 || !p2 || !status))) return ESVIO_FE_EINVAL;
  const int k = host::find_fundamental_mat(p1, p2, n, thr, conf, status);
  if (n_inliers) *n_inliers = k;
  return 0;
}

int esvio_fe_host_hypot(const double* x, const double* y, int n, double* out) {
  if (n < 0 || (n && (!x || !y || !out))) return ESVIO_FE_EINVAL;
  host::host_hypot(x, y, n, out);
  return ESVIO_FE_OK;
}

int esvio_fe_host_stage_copy(void* dst, const void* src, size_t len) {
  if (len && (!dst || !src)) return ESVIO_FE_EINVAL;
  stager_copy_bytes((uint8_t*)dst, (const uint8_t*)src, len);
  return ESVIO_FE_OK;
}

int esvio_fe_host_stage_pack(void* dst, const void* src, size_t len, uint32_t* base_sec) {
  uint32_t b = 0;
  if (len && (!dst || !src)) return ESVIO_FE_EINVAL;
  const bool ok = stager_pack_bytes((uint8_t*)dst, (const uint8_t*)src, len, &b);
  if (base_sec) *base_sec = b;
  return ok ? 1 : 0;
}

int esvio_fe_staging_counters(esvio_fe_handle c, uint64_t out4[4]) {
  if (!c || !out4) return ESVIO_FE_EINVAL;
  stager_counters(c, out4);
  return ESVIO_FE_OK;
}

int esvio_fe_host_nullspace(const double* systems, int n, int lanes, double* f12, int32_t* redone) {
  if (n < 0 || (n && (!systems || !f12))) return ESVIO_FE_EINVAL;
  const int r = host::host_nullspace(systems, n, lanes, f12);
  if (redone) *redone = r;
  return ESVIO_FE_OK;
}

int esvio_fe_ransac_stats(uint64_t* out6, int reset) {
  if (!out6) return ESVIO_FE_EINVAL;
  const host::RansacStats r = host::ransac_stats(reset != 0);
  out6[0] = r.calls;
  out6[1] = r.iterations;
  out6[2] = r.points;
  out6[3] = r.ns;
  out6[4] = r.lmeds_calls;
  out6[5] = r.lmeds_ns;
  return ESVIO_FE_OK;
}

int esvio_fe_find_fundamental_mat_mt(const float* p1, const float* p2, int n, double thr, double conf,
                                     int threads, uint8_t* status, int32_t* n_inliers) {
  if (n < 0 || (n && (!p1 || !p2 || !status)) || threads < 1 || threads > 16) return ESVIO_FE_EINVAL;
  host::RansacPool* pool = host::ransac_pool_create(threads - 1);
  const int k = host::find_fundamental_mat(p1, p2, n, thr, conf, status, pool);
  host::ransac_pool_destroy(pool);
  if (n_inliers) *n_inliers = k;
  return 0;
}

int esvio_fe_find_fundamental_mat_held(const float* p1, const float* p2, int n, double thr, double conf,
                                       int threads, int hold_mask, uint8_t* status, int32_t* n_inliers) {
  if (n < 0 || (n && (!p1 || !p2 || !status)) || threads < 2 || threads > 16 || hold_mask < 0 || hold_mask > 3)
    return ESVIO_FE_EINVAL;
  host::RansacPool* pool = host::ransac_pool_create(threads - 1);
  host::ransac_pool_hold(pool, hold_mask, true);
  const int k = host::find_fundamental_mat(p1, p2, n, thr, conf, status, pool);
  host::ransac_pool_hold(pool, hold_mask, false);
  host::ransac_pool_destroy(pool);
  if (n_inliers) *n_inliers = k;
  return 0;
}

namespace {
struct IdleTap {
  std::atomic<int> pending{0};
  std::atomic<uint64_t> calls{0}, done{0};
};
bool idle_tap_fn(void* arg) {  // what the staging hands the helpers: one unit of work, if there is one
  IdleTap* t = (IdleTap*)arg;
  t->calls.fetch_add(1, std::memory_order_relaxed);
  int v = t->pending.load(std::memory_order_acquire);
  while (v > 0)
    if (t->pending.compare_exchange_weak(v, v - 1, std::memory_order_acq_rel)) {
      const auto t0 = std::chrono::steady_clock::now();  // (a unit: ~5 us, a staging chunk's order of magnitude)
      while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(5)) {}
      t->done.fetch_add(1, std::memory_order_relaxed);
      return true;
    }
  return false;
}
}  // namespace

int esvio_fe_find_fundamental_mat_idle(const float* p1, const float* p2, int n, double thr, double conf,
                                       int threads, int repeats, int idle_units, uint8_t* status, int32_t* n_inliers,
                                       uint64_t out3[3]) {
  if (n < 0 || (n && (!p1 || !p2 || !status)) || threads < 2 || threads > 16 || repeats < 1 || idle_units < 0 || !out3)
    return ESVIO_FE_EINVAL;
  host::RansacPool* pool = host::ransac_pool_create(threads - 1);
  IdleTap tap;
  host::ransac_pool_set_idle_work(pool, &tap.pending, idle_tap_fn, &tap);
  int k = 0;
  for (int r = 0; r < repeats; r++) {
    tap.pending.fetch_add(idle_units, std::memory_order_acq_rel);  // (work arrives while the helpers spin)
    k = host::find_fundamental_mat(p1, p2, n, thr, conf, status, pool);
  }
  const auto t0 = std::chrono::steady_clock::now();  // what is left is taken while the helpers idle (bounded wait)
  while (tap.pending.load(std::memory_order_acquire) > 0 && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(2)) {}
  host::ransac_pool_set_idle_work(pool, nullptr, nullptr, nullptr);  // (returns once nobody is inside the hook)
  out3[0] = tap.calls.load();
  out3[1] = tap.done.load();
  out3[2] = (uint64_t)std::max(0, tap.pending.load());
  host::ransac_pool_destroy(pool);
  if (n_inliers) *n_inliers = k;
  return 0;
}

int esvio_fe_lift_projective(const esvio_fe_camera* cam, double u, double v, double* out3) {
  if (!cam || !out3) return ESVIO_FE_EINVAL;
  host::lift_projective(*cam, u, v, out3);
  return 0;
}

static int fill_tracks(esvio_fe_handle c, esvio_fe_tracks* out);
static int track_event_entry(esvio_fe_handle c, double cur_time, const esvio_fe_event* left,
                             size_t nL, const esvio_fe_event* right, size_t nR, int space,
                             int pub_this_frame, const esvio_fe_motion* motion,
                             esvio_fe_tracks* out) {
  if (!c) return ESVIO_FE_EINVAL;
  if (nL == 0 || !left) return fail(c, ESVIO_FE_EINVAL, "left batch must not be empty (node:150)");
  if (nR && !right) return ESVIO_FE_EINVAL;
  if (nL + nR >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = track_event_impl(c, cur_time, left, nL, right, nR, space, pub_this_frame != 0, motion))
    return rc;
  return fill_tracks(c, out);
}

// copy the result members (feature_tracker.h:126-138) into the caller's buffers
static int fill_tracks(esvio_fe_handle c, esvio_fe_tracks* out) {
  if (out) {
    out->n_left = (int32_t)c->ids.size();
    out->n_right = (int32_t)c->ids_right.size();
    const size_t nl = c->ids.size(), nr = c->ids_right.size();
    // (an empty vector's data() may be null, and memcpy's source must not be, whatever the size)
    auto put = [](void* dst, const void* src, size_t bytes) {
      if (dst && bytes) std::memcpy(dst, src, bytes);
    };
    put(out->ids, c->ids.data(), nl * 4);
    put(out->track_cnt, c->track_cnt.data(), nl * 4);
    put(out->cur_pts, c->cur_pts.data(), nl * 8);
    put(out->cur_un_pts, c->cur_un_pts.data(), nl * 8);
    put(out->pts_velocity, c->pts_velocity.data(), nl * 8);
    put(out->ids_right, c->ids_right.data(), nr * 4);
    put(out->cur_right_pts, c->cur_right_pts.data(), nr * 8);
    put(out->cur_un_right_pts, c->cur_un_right_pts.data(), nr * 8);
    put(out->right_pts_velocity, c->right_pts_velocity.data(), nr * 8);
  }
  return 0;
}

int esvio_fe_track_event(esvio_fe_handle c, double cur_time, const esvio_fe_event* left, size_t nL,
                         const esvio_fe_event* right, size_t nR, int space, int pub_this_frame,
                         esvio_fe_tracks* out) {
  return track_event_entry(c, cur_time, left, nL, right, nR, space, pub_this_frame, nullptr, out);
}

int esvio_fe_track_event_mc(esvio_fe_handle c, double cur_time, const esvio_fe_event* left,
                            size_t nL, const esvio_fe_event* right, size_t nR, int space,
                            int pub_this_frame, const esvio_fe_motion* motion,
                            esvio_fe_tracks* out) {
  if (!motion) return ESVIO_FE_EINVAL;
  return track_event_entry(c, cur_time, left, nL, right, nR, space, pub_this_frame, motion, out);
}

// ---- event layouts: caller-layout field arrays -> event records (esvio_fe_convert_events)
namespace {
struct FieldView {  // one field of the descriptor: where, how far apart, how wide
  const uint8_t* p;
  int32_t stride;
  int width;
  const char* name;
};
void field_views(const esvio_fe_event_fields& f, FieldView v[4]) {
  v[0] = {(const uint8_t*)f.x, f.x_stride, 2, "x"};
  v[1] = {(const uint8_t*)f.y, f.y_stride, 2, "y"};
  v[2] = {(const uint8_t*)f.t, f.t_stride, f.t_bits / 8, "t"};
  v[3] = {(const uint8_t*)f.p, f.p_stride, f.p_bits / 8, "p"};
}
size_t field_span(const FieldView& v, size_t n) { return (n - 1) * (size_t)v.stride + (size_t)v.width; }

int fields_check(esvio_fe_ctx* c, const esvio_fe_event_fields* f, size_t n, const char* who) {
  if (!f) return n ? fail(c, ESVIO_FE_EINVAL, "%s: no field descriptor", who) : 0;
  if (f->t_bits != 32 && f->t_bits != 64) return fail(c, ESVIO_FE_EINVAL, "%s: t_bits must be 32 or 64 (got %d)", who, f->t_bits);
  if (f->t_unit_ns != 1 && f->t_unit_ns != 1000)
    return fail(c, ESVIO_FE_EINVAL, "%s: t_unit_ns must be 1 or 1000 (got %d)", who, f->t_unit_ns);
  if (f->p_bits != 8 && f->p_bits != 16) return fail(c, ESVIO_FE_EINVAL, "%s: p_bits must be 8 or 16 (got %d)", who, f->p_bits);
  const int64_t lim = (int64_t)1 << 62;
  if (f->t_offset > lim || f->t_offset < -lim) return fail(c, ESVIO_FE_EINVAL, "%s: |t_offset| must be <= 2^62", who);
  FieldView v[4];
  field_views(*f, v);
  for (const FieldView& k : v) {
    if (k.stride < k.width)
      return fail(c, ESVIO_FE_EINVAL, "%s: %s_stride %d is below the field's width %d", who, k.name, k.stride, k.width);
    if (n && !k.p) return fail(c, ESVIO_FE_EINVAL, "%s: field %s is null", who, k.name);
  }
  return 0;
}

// [p, p + len) is page-locked memory the runtime knows and maps contiguously: its device-side address, else null
// (first AND last byte, as fe_evstage.cpp's test: a kernel reading beyond a mapping is a fatal queue error)
const uint8_t* pinned_device_ptr(const uint8_t* p, size_t len) {
  auto pinned = [](const void* q) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return a.type == hipMemoryTypeHost;
  };
  if (!len || !pinned(p) || !pinned(p + len - 1)) return nullptr;
  void *d0 = nullptr, *d1 = nullptr;
  if (hipHostGetDevicePointer(&d0, const_cast<uint8_t*>(p), 0) != hipSuccess || !d0 ||
      hipHostGetDevicePointer(&d1, const_cast<uint8_t*>(p) + len - 1, 0) != hipSuccess ||
      (uint8_t*)d1 != (uint8_t*)d0 + len - 1) {
    (void)hipGetLastError();
    return nullptr;
  }
  return (const uint8_t*)d0;
}

// Make the fields of n events (n > 0, checked descriptor) readable on the device, on the current stream: *a = what a
// kernel reads them with.  Device memory is read where it lies, page-locked host memory through its device-side
// address; a host source that is not read in place is copied into c->d_cvt_src first: every byte range the
// fields span once (the four fields of an AoS source overlap: one range), each at its source's address modulo 16,
// so that an aligned source stays aligned for the kernels' wide loads.  Shared by the conversion and the filter's
// fields form; c->d_cvt_src is reused in stream order.
int fields_on_device(esvio_fe_ctx* c, const esvio_fe_event_fields& f, size_t n, int src_space, FieldsArgs* a) {
  hipStream_t s = cur_stream(c);
  FieldView v[4];
  field_views(f, v);
  const uint8_t* dev[4] = {v[0].p, v[1].p, v[2].p, v[3].p};
  if (src_space == ESVIO_FE_HOST) {
    // Page-locked sources, measured both ways (KERNELS.md "Event layouts"): separate arrays are faster read in place
    // at both batch sizes; records (a stride above the field's width: 16 or 13 bytes per lane and event, a poor
    // shape for reads over PCIe) are faster in place at 167 k events and faster copied first at 3.3 M — the
    // crossover itself was not measured, the switch sits at 2^20 events.
    bool records = false;
    for (const FieldView& k : v) records = records || k.stride != k.width;
    bool in_place = c->cvt_pinned_copy < 0 ? !(records && n >= ((size_t)1 << 20)) : c->cvt_pinned_copy == 0;
    for (int k = 0; k < 4 && in_place; k++) {
      dev[k] = pinned_device_ptr(v[k].p, field_span(v[k], n));
      in_place = dev[k] != nullptr;
    }
    if (!in_place) {
      int order[4] = {0, 1, 2, 3};
      std::sort(order, order + 4, [&](int a, int b) { return v[a].p < v[b].p; });
      struct Range {
        const uint8_t *lo, *hi;
        size_t off;
      } rg[4];
      int nr = 0;
      for (int k : order) {
        const uint8_t *lo = v[k].p, *hi = lo + field_span(v[k], n);
        if (nr && lo <= rg[nr - 1].hi)
          rg[nr - 1].hi = std::max(rg[nr - 1].hi, hi);
        else
          rg[nr++] = {lo, hi, 0};
      }
      size_t total = 0;
      for (int r = 0; r < nr; r++) {
        rg[r].off = ((total + 15) & ~(size_t)15) + ((uintptr_t)rg[r].lo & 15);
        total = rg[r].off + (size_t)(rg[r].hi - rg[r].lo);
      }
      if (int rc = c->d_cvt_src.grow(c, total)) return rc;
      for (int r = 0; r < nr; r++)
        HIPCHK(c, hipMemcpyAsync(c->d_cvt_src + rg[r].off, rg[r].lo, (size_t)(rg[r].hi - rg[r].lo), hipMemcpyHostToDevice, s));
      for (int k = 0; k < 4; k++)
        for (int r = 0; r < nr; r++)
          if (v[k].p >= rg[r].lo && v[k].p < rg[r].hi) dev[k] = c->d_cvt_src + rg[r].off + (v[k].p - rg[r].lo);
    }
  }
  *a = FieldsArgs{};
  a->x = dev[0], a->y = dev[1], a->t = dev[2], a->p = dev[3];
  a->x_stride = f.x_stride, a->y_stride = f.y_stride, a->t_stride = f.t_stride, a->p_stride = f.p_stride;
  a->t_bits = f.t_bits, a->t_unit_ns = f.t_unit_ns, a->p_bits = f.p_bits, a->t_offset = f.t_offset;
  return 0;
}
size_t fields_bytes_per_event(const esvio_fe_event_fields& f) { return (size_t)(2 + 2 + f.t_bits / 8 + f.p_bits / 8); }

// Enqueue the conversion of n events (checked descriptor) into d_dst on the current stream; bad events are added to
// c->d_cvt_bad[slot] (one count per camera).
int convert_enqueue(esvio_fe_ctx* c, const esvio_fe_event_fields& f, size_t n, int src_space, EventRec* d_dst, int slot = 0) {
  if (!n) return 0;
  FieldsArgs a;
  if (int rc = fields_on_device(c, f, n, src_space, &a)) return rc;
  ScopedKernel k(c, K_EVENTS_FROM_FIELDS, n * (fields_bytes_per_event(f) + 16));
  launch_events_from_fields(cur_stream(c), a, n, d_dst, c->d_cvt_bad + slot);
  return 0;
}
int convert_begin(esvio_fe_ctx* c) {  // the bad-event counters, cleared in stream order
  if (!c->d_cvt_bad)
    if (int rc = c->d_cvt_bad.alloc(c, 2)) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_cvt_bad, 0, 2 * sizeof(unsigned long long), cur_stream(c)));
  return 0;
}
int convert_end(esvio_fe_ctx* c, unsigned long long* bad) {  // waits for the conversions enqueued since convert_begin
  HIPCHK(c, hipMemcpyAsync(bad, c->d_cvt_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}
}  // namespace

int esvio_fe_convert_events(esvio_fe_handle c, const esvio_fe_event_fields* src, size_t n, int src_space,
                            esvio_fe_event* dst, int dst_space, uint64_t* n_bad) {
  if (!c) return ESVIO_FE_EINVAL;
  if (n_bad) *n_bad = 0;
  if ((src_space != ESVIO_FE_HOST && src_space != ESVIO_FE_DEVICE) || (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE))
    return fail(c, ESVIO_FE_EINVAL, "convert_events: bad memory space");
  if (int rc = fields_check(c, src, n, "convert_events")) return rc;
  if (!n) return 0;
  if (!dst) return fail(c, ESVIO_FE_EINVAL, "convert_events: dst is null");
  if (dst_space == ESVIO_FE_DEVICE && ((uintptr_t)dst & 15) != 0)
    return fail(c, ESVIO_FE_EINVAL, "convert_events: a device dst must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->dev));
  EventRec* d_dst = (EventRec*)dst;
  if (dst_space == ESVIO_FE_HOST) {
    if (int rc = c->d_cvt_out.grow(c, n)) return rc;
    d_dst = c->d_cvt_out;
  }
  if (int rc = convert_begin(c)) return rc;
  if (int rc = convert_enqueue(c, *src, n, src_space, d_dst)) return rc;
  unsigned long long bad = 0;
  if (int rc = convert_end(c, &bad)) return rc;
  if (c->prof_on) resolve_profile(c);
  if (n_bad) *n_bad = bad;
  if (bad)
    return fail(c, ESVIO_FE_EINVAL, "convert_events: %llu of %zu events have a stamp outside [0, 2^32 s) (or a 64-bit t outside +-2^62)", bad, n);
  if (dst_space == ESVIO_FE_HOST) {
    HIPCHK(c, hipMemcpyAsync(dst, d_dst, n * sizeof(EventRec), hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  }
  return 0;
}

// The handle's two alternating pairs of record buffers [pair][camera] (include/esvio_fe.h: buffer lifetime), shared by
// the entry points that make the records they track.  cvt_pair_begin: room for (nL, nR) records in both pairs — the
// second call of a size allocates nothing — and the current pair's buffers, behind everything the pair's previous use
// (two calls back) left on the side streams: what it left on the main stream is in front of us there anyway.
// cvt_pair_track: the track call (plain, or motion-compensated with `motion`) on the pair's records; marks what it
// leaves on the side streams and hands the next call the other pair.
namespace {
int cvt_pair_begin(esvio_fe_ctx* c, size_t nL, size_t nR, EventRec** dL, EventRec** dR) {
  for (int p = 0; p < 2; p++) {
    if (int rc = c->d_cvt_ev[p][0].grow(c, nL)) return rc;
    if (int rc = c->d_cvt_ev[p][1].grow(c, nR)) return rc;
  }
  const int pair = c->cvt_pair;
  hipStream_t side[4] = {c->stream2, c->stream3, c->stream4, c->stream6};
  if (c->cvt_side_rec[pair])
    for (int k = 0; k < 4; k++)
      if (side[k]) HIPCHK(c, hipStreamWaitEvent(cur_stream(c), c->ev_cvt_side[pair][k], 0));
  *dL = c->d_cvt_ev[pair][0];
  *dR = c->d_cvt_ev[pair][1];
  return 0;
}
int cvt_pair_track(esvio_fe_ctx* c, double cur_time, const EventRec* dL, size_t nL, const EventRec* dR, size_t nR,
                   int pub_this_frame, const esvio_fe_motion* motion, esvio_fe_tracks* out) {
  const int pair = c->cvt_pair;
  hipStream_t side[4] = {c->stream2, c->stream3, c->stream4, c->stream6};
  const int rc = track_event_impl(c, cur_time, (const esvio_fe_event*)dL, nL, (const esvio_fe_event*)(nR ? dR : nullptr), nR,
                                  ESVIO_FE_DEVICE, pub_this_frame != 0, motion);
  for (int k = 0; k < 4; k++)
    if (side[k]) {
      if (!c->ev_cvt_side[pair][k]) HIPCHK(c, c->ev_cvt_side[pair][k].create());
      HIPCHK(c, hipEventRecord(c->ev_cvt_side[pair][k], side[k]));
    }
  c->cvt_side_rec[pair] = true;
  c->cvt_pair ^= 1;
  if (rc) return rc;
  return fill_tracks(c, out);
}
}  // namespace

// ---- background-activity + refractory filter of an event batch (the rule: include/esvio_fe.h)
namespace {
constexpr int64_t kBafMaxWindow = (int64_t)1 << 62;

// esvio_fe_filter_events' limits (min_support 1..8), its messages
int baf_params_check(esvio_fe_ctx* c, int64_t window_ns, int min_support, const char* who) {
  if (window_ns < 1 || window_ns > kBafMaxWindow) return fail(c, ESVIO_FE_EINVAL, "%s: window_ns must be in 1..2^62 (got %lld)", who, (long long)window_ns);
  if (min_support < 1 || min_support > 8) return fail(c, ESVIO_FE_EINVAL, "%s: min_support must be in 1..8 (got %d)", who, min_support);
  return 0;
}
// esvio_fe_filter_params' limits
int baf_prm_check(esvio_fe_ctx* c, const esvio_fe_filter_params* p, const char* who) {
  if (!p) return fail(c, ESVIO_FE_EINVAL, "%s: no filter parameters", who);
  if (p->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "%s: esvio_fe_filter_params.reserved must be 0", who);
  if (p->min_support < 0 || p->min_support > 8) return fail(c, ESVIO_FE_EINVAL, "%s: min_support must be in 0..8 (got %d)", who, p->min_support);
  if (p->min_support > 0 && (p->window_ns < 1 || p->window_ns > kBafMaxWindow))
    return fail(c, ESVIO_FE_EINVAL, "%s: window_ns must be in 1..2^62 (got %lld)", who, (long long)p->window_ns);
  if (p->refractory_ns < 0 || p->refractory_ns > kBafMaxWindow)
    return fail(c, ESVIO_FE_EINVAL, "%s: refractory_ns must be in 0..2^62 (got %lld)", who, (long long)p->refractory_ns);
  return 0;
}

// what the chain's keys kernels take of camera cam's address stage (on == 0: none set)
AddrArgs addr_args(const esvio_fe_ctx* c, int cam) {
  AddrArgs a{};
  if (!c->addr.on[cam]) return a;
  const esvio_fe_address_filter& f = c->addr.f[cam];
  a.x0 = f.roi_x0, a.y0 = f.roi_y0, a.x1 = f.roi_x1, a.y1 = f.roi_y1;
  a.polarity = f.polarity, a.on = 1;
  a.mask = f.use_mask ? c->addr.mask[cam].p : nullptr;  // (no mask set: use_mask rejects nothing)
  return a;
}

int baf_clear(esvio_fe_ctx* c) {  // every plane back to `none`, the sort's scratch words as a finished sort leaves them
  esvio_fe_ctx::Baf& f = c->baf;
  if (f.B) HIPCHK(c, hipMemsetAsync(f.B, 0xff, (size_t)2 * c->P * sizeof(long long), cur_stream(c)));
  if (f.sort) HIPCHK(c, hipMemsetAsync(f.sort, 0, (size_t)kSortHeadWords * 4, cur_stream(c)));
  return 0;
}

// the planes (first call) and the per-event scratch for calls of up to n events; host_src / host_dst: the record
// buffers of a host source / destination as well; fields_form: the stream-order stamps of the fields form (on its
// first use, as src and out: a handle that only filters records holds none; kept at the scratch's size from then on)
int baf_ensure(esvio_fe_ctx* c, size_t n, bool host_src, bool host_dst, bool fields_form) {
  esvio_fe_ctx::Baf& f = c->baf;
  if (!f.B) {
    if (int rc = f.head.alloc(c, c->P)) return rc;
    if (int rc = f.res.alloc(c, 2)) return rc;
    if (int rc = f.B.alloc(c, (size_t)2 * c->P)) return rc;
    // (f.B says "the stage's state exists": a plane or a head table that could not be cleared is not there)
    hipError_t e = hipMemsetAsync(f.head, 0, (size_t)c->P * 4, cur_stream(c));
    if (e == hipSuccess) e = hipMemsetAsync(f.B, 0xff, (size_t)2 * c->P * sizeof(long long), cur_stream(c));
    if (e != hipSuccess) {
      f.B.release();
      HIPCHK(c, e);
    }
  }
  if (n > f.cap) {
    const size_t cap = std::max<size_t>(n + n / 4, 1 << 16);
    f.cap = 0;
    for (int k = 0; k < 2; k++) {
      if (int rc = f.keys[k].alloc(c, cap)) return rc;
      if (int rc = f.vals[k].alloc(c, cap)) return rc;
    }
    if (int rc = f.tsort.alloc(c, cap)) return rc;
    if (int rc = f.flags.alloc(c, cap + 4)) return rc;
    if (int rc = f.blk_cnt.alloc(c, (size_t)baf_blocks((uint32_t)cap) + 1)) return rc;
    const size_t words = sort_scratch_words(cap);
    if (int rc = f.sort.alloc(c, words)) return rc;
    HIPCHK(c, hipMemsetAsync(f.sort, 0, words * 4, cur_stream(c)));
    f.cap = cap;
  }
  if (fields_form || f.tstream)
    if (int rc = f.tstream.grow(c, f.cap + 4)) return rc;
  if (host_src)
    if (int rc = f.src.grow(c, n)) return rc;
  if (host_dst)
    if (int rc = f.out.grow(c, n)) return rc;
  return 0;
}

// Enqueue camera cam's chain for n > 0 events — records at `ev` (a host source is copied into the stage's scratch
// first, as it is) or `fields` where they lie (fields_on_device) — into the device buffer d_dst, advancing the
// camera's plane.  Nothing is waited for: the chain's result block is c->baf.res[cam] (baf_fetch), and the per-event
// scratch is free for the next chain on the stream behind this one.
int baf_enqueue(esvio_fe_ctx* c, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields, size_t n, int space,
                const esvio_fe_filter_params& prm, EventRec* d_dst, const char* who) {
  esvio_fe_ctx::Baf& f = c->baf;
  hipStream_t s = cur_stream(c);
  int key_bits = 1;
  while (((uint64_t)1 << key_bits) <= c->P) key_bits++;  // keys 0..P, P = out of the sensor
  const int passes = (key_bits + 6) / 7, bits = (key_bits + passes - 1) / passes;
  if (passes > kRadixMaxPasses) return fail(c, ESVIO_FE_ENOTIMPL, "%s: the sensor has more pixels than the sort's %d digits hold", who, kRadixMaxPasses);
  const EventRec* d_ev = (const EventRec*)ev;
  FieldsArgs fa{};
  if (fields) {
    d_ev = nullptr;
    if (int rc = fields_on_device(c, *fields, n, space, &fa)) return rc;
  } else if (space == ESVIO_FE_HOST) {
    HIPCHK(c, hipMemcpyAsync(f.src, ev, n * sizeof(EventRec), hipMemcpyHostToDevice, s));
    d_ev = f.src;
  }
  BafResult* res = f.res + cam;
  HIPCHK(c, hipMemsetAsync(res, 0, sizeof(BafResult), s));
  const uint32_t n32 = (uint32_t)n;
  const SortScratch sc = sort_scratch(f.sort);
  const size_t pass_words = (size_t)radix_blocks(n32) << bits;
  uint8_t* res_bytes = (uint8_t*)res;
  const uint64_t fb = fields ? fields_bytes_per_event(*fields) : 0;
  const AddrArgs ad = addr_args(c, cam);
  // booked: what each launch has to move at least (keys, indices and stamps once; per neighbour a head and a stamp);
  // the emits' share for the kept records is booked as if all were kept
  if (fields) {
    ScopedKernel k(c, K_BAF_KEYS_FIELDS, (uint64_t)n * (fb + 4 + 4 + 8));
    launch_baf_keys_fields(s, fa, n32, c->W, c->H, f.keys[0], f.vals[0], f.tstream, res, passes, bits, sc.ghist, sc.lookback,
                           (uint32_t)(passes * pass_words), ad);
  } else if (ad.on) {  // step 1a: the stage's keys kernel in k_sae_keys' place (one mask word more per event)
    ScopedKernel k(c, K_BAF_KEYS_ADDR, (uint64_t)n * 28);
    launch_baf_keys_addr(s, d_ev, n32, c->W, c->H, f.keys[0], f.vals[0], res, passes, bits, sc.ghist, sc.lookback,
                         (uint32_t)(passes * pass_words), ad);
  } else {
    ScopedKernel k(c, K_SAE_KEYS, (uint64_t)n * 24);
    launch_sae_keys(s, d_ev, n32, nullptr, 0, c->W, c->H, f.keys[0], f.vals[0], c->P,
                    (unsigned long long*)(res_bytes + offsetof(BafResult, n_rejected)), passes, bits, sc.ghist, sc.lookback,
                    (uint32_t)(passes * pass_words), nullptr);
  }
  int cur = 0;
  for (int p = 0; p < passes; p++) {
    ScopedKernel k(c, K_RADIX_PASS, (uint64_t)n * 16);
    launch_radix_pass(s, f.keys[cur], f.vals[cur], n32, p * bits, bits, sc.ghist + ((size_t)p << bits),
                      sc.lookback + p * pass_words, sc.tickets + p, f.keys[cur ^ 1], f.vals[cur ^ 1],
                      (int*)(res_bytes + offsetof(BafResult, err)), c->lim.lookback);
    cur ^= 1;
  }
  BafArgs a{};
  a.ev = d_ev, a.tstream = fields ? f.tstream.p : nullptr, a.n = n32, a.P = c->P, a.W = c->W, a.H = c->H;
  a.keys = f.keys[cur], a.vals = f.vals[cur], a.head = f.head, a.tsort = f.tsort;
  a.B = f.B + (size_t)cam * c->P;
  a.window_ns = prm.window_ns, a.min_support = prm.min_support, a.refractory_ns = prm.refractory_ns;
  a.flags = f.flags, a.blk_cnt = f.blk_cnt, a.dst = d_dst, a.res = res;
  a.sort_scratch = f.sort, a.sort_head_words = sc.head_words;
  a.flatten = ad.on ? c->addr.f[cam].flatten : 0;
  {
    ScopedKernel k(c, K_BAF_HEADS, (uint64_t)n * (fields ? 24 : 32));
    launch_baf_heads(s, a);
  }
  {
    ScopedKernel k(c, K_BAF_FILTER, (uint64_t)n * (16 + (prm.min_support ? 8 * 12 : 0) + (prm.refractory_ns ? 12 : 0) + 1));
    launch_baf_filter(s, a);
  }
  {
    ScopedKernel k(c, K_BAF_COUNT, (uint64_t)n * (1 + 4 + 8));
    launch_baf_count(s, a);
  }
  {
    ScopedKernel k(c, K_BAF_SCAN, (uint64_t)baf_blocks(n32) * 8);
    launch_baf_scan(s, a);
  }
  if (fields) {
    ScopedKernel k(c, K_BAF_EMIT_FIELDS, (uint64_t)n * (1 + fb + 16));
    launch_baf_emit_fields(s, a, fa);
  } else {
    ScopedKernel k(c, K_BAF_EMIT, (uint64_t)n * 33);
    launch_baf_emit(s, a);
  }
  return 0;
}
// the copies that bring camera cam's result block (and, if asked for, the n flags) to the host, behind its chain
int baf_fetch(esvio_fe_ctx* c, int cam, BafResult* r, uint8_t* flags, size_t n) {
  HIPCHK(c, hipMemcpyAsync(r, c->baf.res + cam, sizeof(BafResult), hipMemcpyDeviceToHost, cur_stream(c)));
  if (flags) HIPCHK(c, hipMemcpyAsync(flags, c->baf.flags, n, hipMemcpyDeviceToHost, cur_stream(c)));
  return 0;
}
// a waited-for result block: the sort's bounded wait
int baf_result_check(esvio_fe_ctx* c, const BafResult& r, const char* who) {
  if (!r.err) return 0;
  // (the sort did not finish: its scratch words are cleared again; the plane is what the chain made of it)
  HIPCHK(c, hipMemsetAsync(c->baf.sort, 0, c->baf.sort.cap * 4, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return fail(c, ESVIO_FE_EINTERNAL, "%s: radix sort look-back spin expired (esvio_fe_filter_reset before the next call)", who);
}
const char* const kBadStampText = "have a stamp outside [0, 2^32 s) (or a 64-bit t outside +-2^62)";

// The filter stage behind esvio_fe_filter_events and esvio_fe_filter_batch: the arguments checked before any device
// work, camera cam's chain, one wait, the results.
int baf_stage(esvio_fe_ctx* c, const char* who, bool takes_fields, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields, size_t n,
              int space, const esvio_fe_filter_params* prm, esvio_fe_event* dst, int dst_space, uint64_t* n_kept, uint8_t* flags,
              esvio_fe_event* last_kept, uint64_t* n_rejected, uint64_t* n_bad) {
  if (n_kept) *n_kept = 0;
  if (n_rejected) *n_rejected = 0;
  if (n_bad) *n_bad = 0;
  if (fields)
    if (int rc = fields_check(c, fields, n, who)) return rc;
  if (int rc = baf_prm_check(c, prm, who)) return rc;
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if ((space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) || (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE))
    return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (!n) return 0;
  if (n >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "%s: batch too large", who);
  if (!ev && !fields) return fail(c, ESVIO_FE_EINVAL, takes_fields ? "%s: neither ev nor fields is given" : "%s: ev is null", who);
  if (ev && fields) return fail(c, ESVIO_FE_EINVAL, "%s: both ev and fields are given", who);
  if (!dst) return fail(c, ESVIO_FE_EINVAL, "%s: dst is null", who);
  if (dst_space == ESVIO_FE_DEVICE && ((uintptr_t)dst & 15) != 0)
    return fail(c, ESVIO_FE_EINVAL, "%s: a device dst must be 16-byte aligned", who);
  {  // (one address space: a range of one is the same memory under the other name)
    const uintptr_t b0 = (uintptr_t)dst, len = n * sizeof(EventRec);
    if (ev) {
      const uintptr_t a0 = (uintptr_t)ev;
      if (a0 < b0 + len && b0 < a0 + len) return fail(c, ESVIO_FE_EINVAL, "%s: dst overlaps ev", who);
    } else {
      FieldView v[4];
      field_views(*fields, v);
      for (const FieldView& k : v) {
        const uintptr_t a0 = (uintptr_t)k.p, alen = field_span(k, n);
        if (a0 < b0 + len && b0 < a0 + alen) return fail(c, ESVIO_FE_EINVAL, "%s: dst overlaps field %s", who, k.name);
      }
    }
  }
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = baf_ensure(c, n, ev && space == ESVIO_FE_HOST, dst_space == ESVIO_FE_HOST, fields != nullptr)) return rc;
  EventRec* d_dst = dst_space == ESVIO_FE_HOST ? c->baf.out.p : (EventRec*)dst;
  BafResult r{};
  if (int rc = baf_enqueue(c, cam, ev, fields, n, space, *prm, d_dst, who)) return rc;
  if (int rc = baf_fetch(c, cam, &r, flags, n)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  if (int rc = baf_result_check(c, r, who)) return rc;
  if (n_bad) *n_bad = r.n_bad;
  if (r.n_bad)
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events %s; the camera's plane is as it was", who, r.n_bad, n, kBadStampText);
  if (dst_space == ESVIO_FE_HOST && r.n_kept) {
    HIPCHK(c, hipMemcpyAsync(dst, d_dst, (size_t)r.n_kept * sizeof(EventRec), hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  }
  if (n_kept) *n_kept = r.n_kept;
  if (n_rejected) *n_rejected = r.n_rejected;
  if (last_kept && r.n_kept) std::memcpy(last_kept, &r.last, sizeof(EventRec));
  return 0;
}
}  // namespace

int esvio_fe_filter_events(esvio_fe_handle c, int cam, const esvio_fe_event* ev, size_t n, int space, int64_t window_ns,
                           int min_support, esvio_fe_event* dst, int dst_space, uint64_t* n_kept, uint8_t* flags,
                           esvio_fe_event* last_kept, uint64_t* n_rejected) {
  if (!c) return ESVIO_FE_EINVAL;
  if (n_kept) *n_kept = 0;
  if (n_rejected) *n_rejected = 0;
  if (int rc = baf_params_check(c, window_ns, min_support, "filter_events")) return rc;
  const esvio_fe_filter_params prm{window_ns, min_support, 0, 0};
  return baf_stage(c, "filter_events", false, cam, ev, nullptr, n, space, &prm, dst, dst_space, n_kept, flags, last_kept, n_rejected, nullptr);
}

int esvio_fe_filter_batch(esvio_fe_handle c, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields, size_t n,
                          int space, const esvio_fe_filter_params* prm, esvio_fe_event* dst, int dst_space, uint64_t* n_kept,
                          uint8_t* flags, esvio_fe_event* last_kept, uint64_t* n_rejected, uint64_t* n_bad) {
  if (!c) return ESVIO_FE_EINVAL;
  return baf_stage(c, "filter_batch", true, cam, ev, fields, n, space, prm, dst, dst_space, n_kept, flags, last_kept, n_rejected, n_bad);
}

int esvio_fe_filter_reset(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = baf_clear(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}

// ---- the address stage's settings and hot-pixel learning (the rule: include/esvio_fe.h)
namespace {
size_t mask_words(const esvio_fe_ctx* c) { return ((size_t)c->P + 31) / 32; }

int hot_clear(esvio_fe_ctx* c) {
  esvio_fe_ctx::Hot& h = c->hot;
  h.h_st[0] = h.h_st[1] = HotState{};
  if (h.C) {
    HIPCHK(c, hipMemsetAsync(h.C, 0, (size_t)2 * c->P * 4, cur_stream(c)));
    HIPCHK(c, hipMemsetAsync(h.st, 0, 2 * sizeof(HotState), cur_stream(c)));
  }
  return 0;
}
int hot_ensure(esvio_fe_ctx* c) {  // the count planes and the cameras' states, on first use: nothing counted
  esvio_fe_ctx::Hot& h = c->hot;
  if (h.C) return 0;
  if (int rc = h.st.alloc(c, 2)) return rc;
  if (int rc = h.C.alloc(c, (size_t)2 * c->P)) return rc;
  hipError_t e = hipMemsetAsync(h.st, 0, 2 * sizeof(HotState), cur_stream(c));
  if (e == hipSuccess) e = hipMemsetAsync(h.C, 0, (size_t)2 * c->P * 4, cur_stream(c));
  if (e != hipSuccess) {
    h.C.release();
    HIPCHK(c, e);
  }
  return 0;
}
int mask_ensure(esvio_fe_ctx* c, int cam) {  // camera cam's mask words, on first use: no pixel set
  DevBuf<uint32_t>& m = c->addr.mask[cam];
  if (m) return 0;
  if (int rc = m.alloc(c, mask_words(c))) return rc;
  const hipError_t e = hipMemsetAsync(m, 0, mask_words(c) * 4, cur_stream(c));
  if (e != hipSuccess) {
    m.release();
    HIPCHK(c, e);
  }
  return 0;
}
}  // namespace

int esvio_fe_set_address_filter(esvio_fe_handle c, int cam, const esvio_fe_address_filter* a) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "set_address_filter";
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (a) {
    if (a->roi_x0 > a->roi_x1 || a->roi_y0 > a->roi_y1 || (int)a->roi_x1 >= c->W || (int)a->roi_y1 >= c->H)
      return fail(c, ESVIO_FE_EINVAL, "%s: the ROI (%u,%u)-(%u,%u) is inverted or leaves the %d x %d sensor", who, a->roi_x0, a->roi_y0,
                  a->roi_x1, a->roi_y1, c->W, c->H);
    if (a->polarity < 0 || a->polarity > 2) return fail(c, ESVIO_FE_EINVAL, "%s: polarity must be in 0..2 (got %d)", who, a->polarity);
    if (a->flatten < 0 || a->flatten > 2) return fail(c, ESVIO_FE_EINVAL, "%s: flatten must be in 0..2 (got %d)", who, a->flatten);
    if (a->use_mask < 0 || a->use_mask > 1) return fail(c, ESVIO_FE_EINVAL, "%s: use_mask must be 0 or 1 (got %d)", who, a->use_mask);
    if (a->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "%s: esvio_fe_address_filter.reserved must be 0", who);
    c->addr.f[cam] = *a;
  }
  c->addr.on[cam] = a != nullptr;
  return 0;
}

int esvio_fe_set_pixel_mask(esvio_fe_handle c, int cam, const uint16_t* xy, size_t n) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "set_pixel_mask";
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (n && !xy) return fail(c, ESVIO_FE_EINVAL, "%s: xy is null", who);
  for (size_t k = 0; k < n; k++)
    if ((int)xy[2 * k] >= c->W || (int)xy[2 * k + 1] >= c->H)
      return fail(c, ESVIO_FE_EINVAL, "%s: pair %zu (%u,%u) lies outside the %d x %d sensor", who, k, xy[2 * k], xy[2 * k + 1], c->W, c->H);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = mask_ensure(c, cam)) return rc;
  std::vector<uint32_t> words(mask_words(c), 0u);
  for (size_t k = 0; k < n; k++) {
    const uint32_t pix = (uint32_t)xy[2 * k + 1] * (uint32_t)c->W + xy[2 * k];
    words[pix >> 5] |= 1u << (pix & 31u);
  }
  // (behind every chain that reads the old words; the copy has left `words` when the wait returns)
  HIPCHK(c, hipMemcpyAsync(c->addr.mask[cam], words.data(), words.size() * 4, hipMemcpyHostToDevice, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}

int esvio_fe_get_pixel_mask(esvio_fe_handle c, int cam, uint16_t* xy, size_t cap, size_t* n) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "get_pixel_mask";
  if (n) *n = 0;
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (cap && !xy) return fail(c, ESVIO_FE_EINVAL, "%s: xy is null", who);
  if (!c->addr.mask[cam]) return 0;  // no mask set
  HIPCHK(c, hipSetDevice(c->dev));
  std::vector<uint32_t> words(mask_words(c), 0u);
  HIPCHK(c, hipMemcpyAsync(words.data(), c->addr.mask[cam], words.size() * 4, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  size_t set = 0;
  for (uint32_t pix = 0; pix < c->P; pix++)
    if ((words[pix >> 5] >> (pix & 31u)) & 1u) {
      if (set < cap) xy[2 * set] = (uint16_t)(pix % (uint32_t)c->W), xy[2 * set + 1] = (uint16_t)(pix / (uint32_t)c->W);
      set++;
    }
  if (n) *n = set;
  if (set > cap) return fail(c, ESVIO_FE_EINVAL, "%s: the mask holds %zu pixels, xy has room for %zu", who, set, cap);
  return 0;
}

int esvio_fe_hot_learn(esvio_fe_handle c, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields, size_t n,
                       int space, uint64_t* n_bad) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "hot_learn";
  if (n_bad) *n_bad = 0;
  if (fields)
    if (int rc = fields_check(c, fields, n, who)) return rc;
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (!n) return 0;
  if (n >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "%s: batch too large", who);
  if (!ev && !fields) return fail(c, ESVIO_FE_EINVAL, "%s: neither ev nor fields is given", who);
  if (ev && fields) return fail(c, ESVIO_FE_EINVAL, "%s: both ev and fields are given", who);
  esvio_fe_ctx::Hot& h = c->hot;
  if (h.h_st[cam].n + n >= (1ull << 32))
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu events are counted, %zu more would reach 2^32 (esvio_fe_hot_reset)", who, h.h_st[cam].n, n);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = hot_ensure(c)) return rc;
  hipStream_t s = cur_stream(c);
  HotState* st = h.st + cam;
  uint32_t* plane = h.C + (size_t)cam * c->P;
  HIPCHK(c, hipMemsetAsync((uint8_t*)st + offsetof(HotState, n_bad), 0, 8, s));
  if (fields) {
    FieldsArgs fa{};
    if (int rc = fields_on_device(c, *fields, n, space, &fa)) return rc;
    ScopedKernel k(c, K_HOT_COUNT, (uint64_t)n * (fields_bytes_per_event(*fields) + 4));
    launch_hot_count_fields(s, fa, (uint32_t)n, c->W, c->H, plane, st);
  } else {
    const EventRec* d_ev = (const EventRec*)ev;
    if (space == ESVIO_FE_HOST) {
      if (int rc = h.src.grow(c, n)) return rc;
      HIPCHK(c, hipMemcpyAsync(h.src, ev, n * sizeof(EventRec), hipMemcpyHostToDevice, s));
      d_ev = h.src;
    }
    ScopedKernel k(c, K_HOT_COUNT, (uint64_t)n * 20);
    launch_hot_count(s, d_ev, (uint32_t)n, c->W, c->H, plane, st);
  }
  HotState got{};
  HIPCHK(c, hipMemcpyAsync(&got, st, sizeof(HotState), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  h.h_st[cam] = got;
  if (n_bad) *n_bad = got.n_bad;
  if (got.n_bad)
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events %s; they are not counted, the others are", who, got.n_bad, n, kBadStampText);
  return 0;
}

int esvio_fe_hot_select(esvio_fe_handle c, int cam, const esvio_fe_hot_params* prm, uint16_t* xy, uint32_t* counts, size_t cap,
                        esvio_fe_hot_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "hot_select";
  if (info) *info = esvio_fe_hot_info{};
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (!prm) return fail(c, ESVIO_FE_EINVAL, "%s: no parameters", who);
  if (prm->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "%s: esvio_fe_hot_params.reserved must be 0", who);
  if (prm->max_pixels < 1 || prm->max_pixels > kHotMaxPixels)
    return fail(c, ESVIO_FE_EINVAL, "%s: max_pixels must be in 1..%u (got %u)", who, kHotMaxPixels, prm->max_pixels);
  if (prm->min_count < 1) return fail(c, ESVIO_FE_EINVAL, "%s: min_count must be at least 1", who);
  if (prm->min_rate_hz > (1u << 20) || prm->mean_factor > (1u << 20))
    return fail(c, ESVIO_FE_EINVAL, "%s: min_rate_hz and mean_factor must not exceed 2^20", who);
  esvio_fe_ctx::Hot& h = c->hot;
  const HotState& st = h.h_st[cam];
  const uint64_t N = st.n, span = N ? st.tmax - ~st.not_tmin : 0;
  if (prm->min_rate_hz && span > ((uint64_t)1 << 42))
    return fail(c, ESVIO_FE_EINVAL, "%s: the counted events span %llu ns, above the 2^42 a rate threshold takes", who, (unsigned long long)span);
  uint64_t T = prm->min_count;  // (2^20 * 2^42 and 2^20 * 2^32 stay inside 64 bits)
  if (prm->min_rate_hz) T = std::max<uint64_t>(T, ((uint64_t)prm->min_rate_hz * span + 999999999ull) / 1000000000ull);
  if (prm->mean_factor) T = std::max<uint64_t>(T, ((uint64_t)prm->mean_factor * N + c->P - 1) / c->P);
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = hot_ensure(c)) return rc;
  const uint32_t P = c->P;
  if (!h.sort) {  // the selection's scratch, on first use
    for (int k = 0; k < 2; k++) {
      if (int rc = h.keys[k].alloc(c, P)) return rc;
      if (int rc = h.vals[k].alloc(c, P)) return rc;
    }
    if (int rc = h.xy.alloc(c, 2 * kHotMaxPixels)) return rc;
    if (int rc = h.counts.alloc(c, kHotMaxPixels)) return rc;
    if (int rc = h.res.alloc(c, 1)) return rc;
    if (int rc = h.sort.alloc(c, sort_scratch_words(P))) return rc;
  }
  if (prm->install)
    if (int rc = mask_ensure(c, cam)) return rc;
  hipStream_t s = cur_stream(c);
  HIPCHK(c, hipMemsetAsync(h.res, 0, sizeof(HotResult), s));
  HIPCHK(c, hipMemsetAsync(h.sort, 0, h.sort.cap * 4, s));  // digit histograms, tickets and look-back words
  const SortScratch sc = sort_scratch(h.sort);
  const size_t pass_words = (size_t)radix_blocks(P) << kRadixMaxBits;
  HotResult* res = h.res;
  {
    ScopedKernel k(c, K_HOT_KEYS, (uint64_t)P * 12);
    // (a threshold above every possible count: no pixel reaches it)
    launch_hot_keys(s, h.C + (size_t)cam * P, P, (uint32_t)std::min<uint64_t>(T, 0xffffffffull), h.keys[0], h.vals[0], sc.ghist, res);
  }
  int cur = 0;
  for (int p = 0; p < kRadixMaxPasses; p++) {
    ScopedKernel k(c, K_RADIX_PASS, (uint64_t)P * 16);
    launch_radix_pass(s, h.keys[cur], h.vals[cur], P, p * kRadixMaxBits, kRadixMaxBits, sc.ghist + ((size_t)p << kRadixMaxBits),
                      sc.lookback + p * pass_words, sc.tickets + p, h.keys[cur ^ 1], h.vals[cur ^ 1],
                      (int*)((uint8_t*)res + offsetof(HotResult, err)), c->lim.lookback);
    cur ^= 1;
  }
  const bool wants_list = xy || counts;
  {
    ScopedKernel k(c, K_HOT_PICK, (uint64_t)prm->max_pixels * 16);
    launch_hot_pick(s, h.keys[cur], h.vals[cur], c->W, P, prm->max_pixels,
                    wants_list ? (uint32_t)std::min<size_t>(cap, kHotMaxPixels) : kHotMaxPixels, h.xy, h.counts,
                    prm->install ? c->addr.mask[cam].p : nullptr, (uint32_t)mask_words(c), res);
  }
  HotResult r{};
  HIPCHK(c, hipMemcpyAsync(&r, res, sizeof(HotResult), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  if (r.err) return fail(c, ESVIO_FE_EINTERNAL, "%s: radix sort look-back spin expired; nothing selected or installed", who);
  if (info) info->events = N, info->span_ns = span, info->threshold = T, info->above = r.above, info->selected = r.selected;
  if (wants_list && r.selected > cap)
    return fail(c, ESVIO_FE_EINVAL, "%s: %u pixels are selected, the lists have room for %zu; nothing installed", who, r.selected, cap);
  if (r.selected) {
    if (xy) HIPCHK(c, hipMemcpyAsync(xy, h.xy, (size_t)r.selected * 4, hipMemcpyDeviceToHost, s));
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, h.counts, (size_t)r.selected * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  return 0;
}

int esvio_fe_hot_reset(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = hot_clear(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}

// ---- the batch call: records or fields per camera, filtered or not, plain or motion-compensated
namespace {
// own_memory: what the message tells a caller to do instead while batches are announced
int track_batch_body(esvio_fe_ctx* c, const char* who, const char* own_memory, const esvio_fe_batch& b, esvio_fe_tracks* out,
                     esvio_fe_batch_info* info_out) {
  esvio_fe_batch_info info{};
  if (info_out) *info_out = info;
  const size_t n[2] = {b.nL, b.nR};
  const esvio_fe_event* ev[2] = {b.left, b.right};
  const esvio_fe_event_fields* fl[2] = {b.left_fields, b.right_fields};
  if (b.space != ESVIO_FE_HOST && b.space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (b.reserved != 0) return fail(c, ESVIO_FE_EINVAL, "%s: esvio_fe_batch.reserved must be 0", who);
  for (int cam = 0; cam < 2; cam++) {
    const char* side = cam ? "right" : "left";
    if (n[cam] && !ev[cam] && !fl[cam]) return fail(c, ESVIO_FE_EINVAL, "%s: the %s batch has events and neither records nor fields", who, side);
    if (n[cam] && ev[cam] && fl[cam]) return fail(c, ESVIO_FE_EINVAL, "%s: the %s batch has both records and fields", who, side);
    if (fl[cam]) {
      char w[96];
      snprintf(w, sizeof w, "%s (%s)", who, side);
      if (int rc = fields_check(c, fl[cam], n[cam], w)) return rc;
    }
    if (!n[cam]) ev[cam] = nullptr, fl[cam] = nullptr;
  }
  if (b.filter)
    if (int rc = baf_prm_check(c, b.filter, who)) return rc;
  if (n[0] + n[1] >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  hipStream_t s = cur_stream(c);
  EventRec last{};
  if (!fl[0] && !fl[1] && !b.filter) {  // records as they are: the track call itself, announced batches included
    if (n[0] == 0 || !ev[0]) return fail(c, ESVIO_FE_EINVAL, "left batch must not be empty (node:150)");
    double cur_time = b.cur_time;
    if (b.cur_time_from_batch) {
      if (b.space == ESVIO_FE_HOST) {
        std::memcpy(&last, ev[0] + (n[0] - 1), sizeof(EventRec));
      } else {
        HIPCHK(c, hipSetDevice(c->dev));
        HIPCHK(c, hipMemcpyAsync(&last, ev[0] + (n[0] - 1), sizeof(EventRec), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
      }
      cur_time = (double)last.sec + 1e-9 * (double)last.nsec;
    }
    info.kept[0] = n[0], info.kept[1] = n[1], info.cur_time = cur_time;
    const int rc = track_event_entry(c, cur_time, ev[0], n[0], ev[1], n[1], b.space, b.pub_this_frame, b.motion, out);
    info.tracked = rc == 0;
    if (info_out) *info_out = info;
    return rc;
  }
  if (!b.filter && n[0] == 0) return fail(c, ESVIO_FE_EINVAL, "left batch must not be empty (node:150)");
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "%s: batches are announced on this handle (%s into memory of your own)", who, own_memory);
  HIPCHK(c, hipSetDevice(c->dev));
  EventRec* d[2] = {nullptr, nullptr};
  if (int rc = cvt_pair_begin(c, n[0], n[1], &d[0], &d[1])) return rc;
  if (b.filter) {
    const bool host_records = b.space == ESVIO_FE_HOST && (ev[0] || ev[1]);
    if (int rc = baf_ensure(c, std::max(n[0], n[1]), host_records, false, fl[0] || fl[1])) return rc;
  } else if (int rc = convert_begin(c)) {
    return rc;
  }
  // both cameras' conversion / filter chains, one behind the other on the stream; then ONE wait for everything the
  // host reads before it tracks: the result blocks or the bad counts, and the last left record where it is the stamp
  for (int cam = 0; cam < 2; cam++) {
    if (!n[cam]) continue;
    if (b.filter) {
      char w[96];
      snprintf(w, sizeof w, "%s (%s)", who, cam ? "right" : "left");
      if (int rc = baf_enqueue(c, cam, ev[cam], fl[cam], n[cam], b.space, *b.filter, d[cam], w)) return rc;
    } else if (fl[cam]) {
      if (int rc = convert_enqueue(c, *fl[cam], n[cam], b.space, d[cam], cam)) return rc;
    } else {  // records beside the other camera's fields: into the pair as they are
      HIPCHK(c, hipMemcpyAsync(d[cam], ev[cam], n[cam] * sizeof(EventRec),
                               b.space == ESVIO_FE_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    }
  }
  BafResult r[2] = {};
  unsigned long long bad[2] = {0, 0};
  if (b.filter) {
    for (int cam = 0; cam < 2; cam++)
      if (n[cam])
        if (int rc = baf_fetch(c, cam, &r[cam], nullptr, 0)) return rc;
  } else {
    HIPCHK(c, hipMemcpyAsync(bad, c->d_cvt_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    if (b.cur_time_from_batch) HIPCHK(c, hipMemcpyAsync(&last, d[0] + (n[0] - 1), sizeof(EventRec), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  for (int cam = 0; cam < 2; cam++) {
    if (b.filter) {
      if (int rc = baf_result_check(c, r[cam], who)) return rc;
      bad[cam] = r[cam].n_bad;
      info.rejected[cam] = r[cam].n_rejected;
    }
    info.bad[cam] = bad[cam];
    info.kept[cam] = b.filter ? r[cam].n_kept : n[cam];
  }
  if (bad[0] || bad[1]) {
    info.kept[0] = info.kept[1] = 0;
    if (info_out) *info_out = info;
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events %s%s", who, bad[0] + bad[1], n[0] + n[1], kBadStampText,
                b.filter ? "; the plane of a camera with such an event is as it was, whether the other camera's has advanced is unspecified" : "");
  }
  if (info_out) *info_out = info;
  if (!info.kept[0]) return 0;  // node:150: an empty left message is not tracked (the pair stays this call's: nothing reads it)
  if (b.filter) last = r[0].last;
  info.cur_time = b.cur_time_from_batch ? (double)last.sec + 1e-9 * (double)last.nsec : b.cur_time;
  const int rc = cvt_pair_track(c, info.cur_time, d[0], info.kept[0], d[1], info.kept[1], b.pub_this_frame, b.motion, out);
  info.tracked = rc == 0;
  if (info_out) *info_out = info;
  return rc;
}
}  // namespace

int esvio_fe_track_batch(esvio_fe_handle c, const esvio_fe_batch* b, esvio_fe_tracks* out, esvio_fe_batch_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (!b) return fail(c, ESVIO_FE_EINVAL, "track_batch: no batch");
  return track_batch_body(c, "track_batch", "convert and filter", *b, out, info);
}

int esvio_fe_track_event_fields(esvio_fe_handle c, double cur_time, const esvio_fe_event_fields* left, size_t nL,
                                const esvio_fe_event_fields* right, size_t nR, int src_space, int pub_this_frame,
                                esvio_fe_tracks* out) {
  if (!c) return ESVIO_FE_EINVAL;
  if (src_space != ESVIO_FE_HOST && src_space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "track_event_fields: bad memory space");
  if (nL == 0 || !left) return fail(c, ESVIO_FE_EINVAL, "left batch must not be empty (node:150)");
  if (nL + nR >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  esvio_fe_batch b{};
  b.left_fields = left, b.right_fields = right, b.nL = nL, b.nR = nR, b.space = src_space, b.pub_this_frame = pub_this_frame;
  b.cur_time = cur_time;
  return track_batch_body(c, "track_event_fields", "convert", b, out, nullptr);
}

int esvio_fe_track_event_filtered(esvio_fe_handle c, const esvio_fe_event* left, size_t nL, const esvio_fe_event* right,
                                  size_t nR, int space, int64_t window_ns, int min_support, int pub_this_frame,
                                  esvio_fe_tracks* out, uint64_t kept[2], double* cur_time_out) {
  if (!c) return ESVIO_FE_EINVAL;
  if (kept) kept[0] = kept[1] = 0;
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "track_event_filtered: bad memory space");
  if (int rc = baf_params_check(c, window_ns, min_support, "track_event_filtered")) return rc;
  if ((nL && !left) || (nR && !right)) return fail(c, ESVIO_FE_EINVAL, "track_event_filtered: a batch with events and no pointer");
  const esvio_fe_filter_params prm{window_ns, min_support, 0, 0};
  esvio_fe_batch b{};
  b.left = left, b.right = right, b.nL = nL, b.nR = nR, b.space = space, b.pub_this_frame = pub_this_frame;
  b.filter = &prm, b.cur_time_from_batch = 1;
  esvio_fe_batch_info info{};
  const int rc = track_batch_body(c, "track_event_filtered", "filter", b, out, &info);
  if (kept) kept[0] = info.kept[0], kept[1] = info.kept[1];
  if (info.tracked && cur_time_out) *cur_time_out = info.cur_time;
  return rc;
}

// ---- ingest: what the stream formats' stages share.  A stage decodes a chunk in one "run" (raw_run, aedat_run, bag_run:
// the chain enqueued, waited for and booked, the host's own corrections).  The run asks a placement where each camera's
// records go (DecodedCam::d, cap: the caller's device dst, the decode scratch, the convert pair, the feed's room), fills
// in the rest and leaves the state behind the chunk in the job.  The consumer refuses (BAD stamps first, then lack of
// room) or takes the records, and takes the state over itself when the whole call has succeeded.
namespace {
struct DecodedCam {  // one camera's decoded records behind the wait
  EventRec* d = nullptr;  // where they lie ...
  size_t cap = 0;         // ... and the room there
  size_t events = 0;      // (more than cap: nothing was stored)
  unsigned long long bad = 0;
  uint32_t sec = 0, nsec = 0;  // the last record's stamp (events > 0, bad == 0)
};
// an event dst: its memory space, null with room, the alignment of a device dst
int dst_check(esvio_fe_ctx* c, const char* who, const char* name, const void* dst, size_t room, int space) {
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (room && !dst) return fail(c, ESVIO_FE_EINVAL, "%s: %s is null", who, name);
  if (space == ESVIO_FE_DEVICE && ((uintptr_t)dst & 15) != 0) return fail(c, ESVIO_FE_EINVAL, "%s: a device dst must be 16-byte aligned", who);
  return 0;
}
// placement: the decode scratch — behind a host dst, in front of a filter, for the feed's bag push
int dec_scratch(esvio_fe_ctx* c, int cam, size_t records, DecodedCam* dc) {
  if (int rc = c->rawdec.dec[cam].grow(c, records)) return rc;
  dc->d = c->rawdec.dec[cam], dc->cap = c->rawdec.dec[cam].cap;
  return 0;
}
// placement for "decode and track": the current convert pair, or, in front of a filter, the decode scratch
int track_place(esvio_fe_ctx* c, bool filtered, const size_t want[2], DecodedCam dc[2]) {
  if (filtered) {
    for (int cam = 0; cam < 2; cam++)
      if (int rc = dec_scratch(c, cam, std::max<size_t>(want[cam], 1), &dc[cam])) return rc;
    return 0;
  }
  const int pair = c->cvt_pair;
  if (int rc = cvt_pair_begin(c, want[0], want[1], &dc[0].d, &dc[1].d)) return rc;
  dc[0].cap = c->d_cvt_ev[pair][0].cap, dc[1].cap = c->d_cvt_ev[pair][1].cap;
  return 0;
}
// the records of n cameras to their host dst: the copies, one wait
int deliver_host(esvio_fe_ctx* c, int n, void* const dst[], const DecodedCam dc[]) {
  bool any = false;
  for (int k = 0; k < n; k++) {
    if (!dc[k].events) continue;
    HIPCHK(c, hipMemcpyAsync(dst[k], dc[k].d, dc[k].events * sizeof(EventRec), hipMemcpyDeviceToHost, cur_stream(c)));
    any = true;
  }
  if (any) HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  return 0;
}
// "Decode and track" from the BAD-stamp refusal on: dc[0], dc[1] are the cameras' records — in the decode scratch when
// there is a filter, which then writes the kept ones into the convert pair, else in the pair —, states: how the refusal
// names what stays.  commit() takes the decoders' states over; they move only when the whole call succeeds: a filter or
// track body that fails leaves them as they were.
extern "C++" template <class Commit>  // (this file is one extern "C" block)
int track_decoded(esvio_fe_ctx* c, const char* who, const char* states, const DecodedCam dc[2], const esvio_fe_filter_params* filter,
                  const esvio_fe_motion* motion, int pub_this_frame, esvio_fe_tracks* out, esvio_fe_batch_info* info_out, Commit commit) {
  esvio_fe_batch_info info{};
  info.bad[0] = dc[0].bad, info.bad[1] = dc[1].bad;
  if (dc[0].bad || dc[1].bad) {
    if (info_out) *info_out = info;
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events have a stamp outside [0, 2^32 s); both cameras' %s are as they were", who,
                dc[0].bad + dc[1].bad, dc[0].events + dc[1].events, states);
  }
  auto done = [&](int rc) {
    if (rc == 0) commit();
    return rc;
  };
  if (filter) {  // the body esvio_fe_track_batch has for device records with a filter: into the pair, stamped by the last kept left record
    esvio_fe_batch b{};
    b.left = (const esvio_fe_event*)dc[0].d, b.right = (const esvio_fe_event*)dc[1].d;
    b.nL = dc[0].events, b.nR = dc[1].events, b.space = ESVIO_FE_DEVICE, b.pub_this_frame = pub_this_frame;
    b.filter = filter, b.motion = motion, b.cur_time_from_batch = 1;
    return done(track_batch_body(c, who, "decode and filter", b, out, info_out));
  }
  info.kept[0] = dc[0].events, info.kept[1] = dc[1].events;
  if (info_out) *info_out = info;
  if (!dc[0].events) return done(0);  // node:150: an empty left message is not tracked
  info.cur_time = (double)dc[0].sec + 1e-9 * (double)dc[0].nsec;
  const int rc = cvt_pair_track(c, info.cur_time, dc[0].d, dc[0].events, dc[1].d, dc[1].events, pub_this_frame, motion, out);
  info.tracked = rc == 0;
  if (info_out) *info_out = info;
  return done(rc);
}
}  // namespace

// ---- raw sensor streams: EVT3 / EVT2 words -> event records (the rule: include/esvio_fe.h; the chain: fe_kernels.h)
namespace {
constexpr size_t kRawMaxBytes = (size_t)1 << 28;
// Page-locked sources, measured both ways on prefixes of one stream (KERNELS.md "Raw streams"): the chain reads every
// word twice, so read in place they cross PCIe twice.  In place is faster at 4 .. 256 KiB (by 1.5 - 7 us of a 35 - 58 us
// call), copied first at 512 KiB and beyond (by 5 us there, 220 us at 11.8 MB): the switch sits behind the last size at
// which in place won.
constexpr size_t kRawPinnedInPlaceBytes = (size_t)256 << 10;
struct RawJob {  // one camera's part of a call
  const void* words = nullptr;
  size_t n_bytes = 0;
};

size_t raw_word_bytes(int format) { return format == ESVIO_FE_RAW_EVT3 ? 2 : format == ESVIO_FE_RAW_EVT21 ? 8 : 4; }
int raw_args_check(esvio_fe_ctx* c, const char* who, int format, const void* words, size_t n_bytes, int space, int64_t t_offset_us) {
  if (format != ESVIO_FE_RAW_EVT2 && format != ESVIO_FE_RAW_EVT3 && format != ESVIO_FE_RAW_EVT21)
    return fail(c, ESVIO_FE_EINVAL, "%s: format must be ESVIO_FE_RAW_EVT2, ESVIO_FE_RAW_EVT3 or ESVIO_FE_RAW_EVT21 (got %d)", who, format);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  const int64_t lim = (int64_t)1 << 62;
  if (t_offset_us > lim || t_offset_us < -lim) return fail(c, ESVIO_FE_EINVAL, "%s: |t_offset_us| must be <= 2^62", who);
  const size_t wb = raw_word_bytes(format);
  if (n_bytes % wb) return fail(c, ESVIO_FE_EINVAL, "%s: %zu bytes are no whole number of %zu-byte words", who, n_bytes, wb);
  if (n_bytes > kRawMaxBytes) return fail(c, ESVIO_FE_EINVAL, "%s: a chunk holds at most 2^28 bytes", who);
  if (n_bytes && !words) return fail(c, ESVIO_FE_EINVAL, "%s: words is null", who);
  return 0;
}
size_t raw_bound(int format, size_t n_bytes) {  // the records n_bytes of words can stand for at most
  return format == ESVIO_FE_RAW_EVT3 ? n_bytes / 2 * 12 : format == ESVIO_FE_RAW_EVT21 ? n_bytes * 4 : n_bytes / 4;
}
uint32_t raw_tiles(size_t n_bytes) { return (uint32_t)((n_bytes + kRawTileBytes - 1) / kRawTileBytes); }

int raw_ensure(esvio_fe_ctx* c, int cam, size_t n_bytes, bool copied_src) {
  esvio_fe_ctx::Raw& r = c->rawdec;
  r.used = true;
  if (!r.res)
    if (int rc = r.res.alloc(c, 2)) return rc;
  if (int rc = r.sums[cam].grow(c, raw_tiles(n_bytes))) return rc;
  return copied_src ? r.src[cam].grow(c, n_bytes) : 0;
}
// esvio_fe_reserve for a handle that decodes raw streams: per camera the scratch of a stream of up to 8 bytes per event (include/esvio_fe.h)
int raw_reserve(esvio_fe_ctx* c, const size_t events[2], bool host_batches) {
  for (int cam = 0; cam < 2 && c->rawdec.used; cam++)
    if (int rc = raw_ensure(c, cam, events[cam] * 8, host_batches)) return rc;
  return 0;
}
void raw_state_reset(esvio_fe_ctx* c) {  // the event decoder's and the trigger decoder's
  c->rawdec.st[0] = c->rawdec.st[1] = c->rawdec.trig_st[0] = c->rawdec.trig_st[1] = esvio_fe_ctx::Raw::State();
}

// Enqueue the decode chain of one camera (job[1].n_bytes == 0) or of both on the current stream, and the copies that
// bring the result blocks to the host; nothing is waited for.  dc[k].d, cap: where job[k]'s records go.  *args: what the
// emit launch can be repeated with.
// trig: the trigger chain — the cameras' trigger-decoder states, its own reduce and emit launches around the same scan.
int raw_enqueue(esvio_fe_ctx* c, int format, int space, int64_t t_offset_us, const RawJob job[2], const DecodedCam dc[2], const int cam_of[2],
                RawArgs* args, RawResult res[2], bool trig) {
  esvio_fe_ctx::Raw& r = c->rawdec;
  hipStream_t s = cur_stream(c);
  RawArgs a{};
  a.format = format;
  uint64_t bytes = 0, cap_bytes = 0;
  for (int k = 0; k < 2; k++) {
    if (!job[k].n_bytes) continue;
    const int cam = cam_of[k];
    const uint8_t* d_words = (const uint8_t*)job[k].words;
    if (space == ESVIO_FE_HOST) {
      const bool in_place = r.pinned_copy < 0 ? job[k].n_bytes <= kRawPinnedInPlaceBytes : r.pinned_copy == 0;
      d_words = in_place ? pinned_device_ptr((const uint8_t*)job[k].words, job[k].n_bytes) : nullptr;
      if (!d_words) {
        if (int rc = raw_ensure(c, cam, job[k].n_bytes, true)) return rc;
        HIPCHK(c, hipMemcpyAsync(r.src[cam], job[k].words, job[k].n_bytes, hipMemcpyHostToDevice, s));
        d_words = r.src[cam];
      }
    }
    if (int rc = raw_ensure(c, cam, job[k].n_bytes, false)) return rc;
    const esvio_fe_ctx::Raw::State& st = trig ? r.trig_st[cam] : r.st[cam];
    RawCam& rc = a.cam[k];
    rc.words = d_words, rc.n_bytes = (uint32_t)job[k].n_bytes, rc.tiles = raw_tiles(job[k].n_bytes);
    rc.seed = RawXf{st.th, st.th, 0, (st.seen ? kRawHasTh : 0u) | kRawHasTl | kRawHasY | kRawHasBx | (st.bp ? kRawBp : 0u) |
                                        st.tl << kRawTlShift | st.y << kRawYShift,
                    st.bx, 0, 0, 0};
    rc.wraps_base = st.wraps, rc.t_offset = t_offset_us;
    rc.sums = r.sums[cam], rc.dst = dc[k].d, rc.dst_cap = (uint32_t)std::min<size_t>(dc[k].cap, 0xffffffffu);
    rc.res = r.res + cam;
    bytes += job[k].n_bytes;
    cap_bytes += std::min(dc[k].cap, trig ? job[k].n_bytes / raw_word_bytes(format) : raw_bound(format, job[k].n_bytes)) * 16;
  }
  {
    ScopedKernel k(c, trig ? K_TRIG_REDUCE : K_RAW_REDUCE, bytes + (uint64_t)(a.cam[0].tiles + a.cam[1].tiles) * sizeof(RawXf));
    if (trig)
      launch_trig_reduce(s, a);
    else
      launch_raw_reduce(s, a);
  }
  {
    ScopedKernel k(c, K_RAW_SCAN, (uint64_t)(a.cam[0].tiles + a.cam[1].tiles) * 2 * sizeof(RawXf));
    launch_raw_scan(s, a);
  }
  {  // (booked as if every record the buffers have room for were written: the count is not known here)
    ScopedKernel k(c, trig ? K_TRIG_EMIT : K_RAW_EMIT, bytes + cap_bytes);
    if (trig)
      launch_trig_emit(s, a);
    else
      launch_raw_emit(s, a);
  }
  for (int k = 0; k < 2; k++)
    if (job[k].n_bytes) HIPCHK(c, hipMemcpyAsync(&res[k], a.cam[k].res, sizeof(RawResult), hipMemcpyDeviceToHost, s));
  *args = a;
  return 0;
}
// the emit launch again, into buffers that have room now (the tiles' prefixes are still where the scan left them)
int raw_emit_again(esvio_fe_ctx* c, RawArgs* a, const RawJob job[2], const DecodedCam dc[2], RawResult res[2], bool trig) {
  hipStream_t s = cur_stream(c);
  for (int k = 0; k < 2; k++) {
    if (!job[k].n_bytes) continue;
    a->cam[k].dst = dc[k].d, a->cam[k].dst_cap = (uint32_t)std::min<size_t>(dc[k].cap, 0xffffffffu);
    HIPCHK(c, hipMemsetAsync((uint8_t*)a->cam[k].res + offsetof(RawResult, bad), 0, sizeof(unsigned long long), s));
  }
  {
    ScopedKernel k(c, trig ? K_TRIG_EMIT : K_RAW_EMIT, (uint64_t)(res[0].events + res[1].events) * 16);
    if (trig)
      launch_trig_emit(s, *a);
    else
      launch_raw_emit(s, *a);
  }
  for (int k = 0; k < 2; k++)
    if (job[k].n_bytes) HIPCHK(c, hipMemcpyAsync(&res[k], a->cam[k].res, sizeof(RawResult), hipMemcpyDeviceToHost, s));
  return 0;
}
void raw_info_fill(esvio_fe_raw_info* info, const RawResult& r, uint64_t wraps) {
  if (!info) return;
  info->events = r.events, info->untimed = r.untimed, info->other = r.other, info->bad = r.bad, info->wraps = wraps;
  if (r.events) info->first_t_us = r.first_t, info->last_t_us = r.last_t;
}
void raw_info_clear(esvio_fe_raw_info* info, uint64_t wraps) {
  if (!info) return;
  info->events = info->untimed = info->other = info->bad = 0;
  info->wraps = wraps;
}
// a call that succeeded: the camera's state is what the scan composed (the trigger decoder's: the time base alone)
void raw_commit(esvio_fe_ctx* c, int cam, const RawResult& r, bool trig = false) {
  esvio_fe_ctx::Raw::State& st = trig ? c->rawdec.trig_st[cam] : c->rawdec.st[cam];
  const RawXf& x = r.state;
  st.seen = x.flags & kRawHasTh ? 1 : 0, st.th = x.th_last, st.wraps += x.wraps;
  st.tl = (x.flags >> kRawTlShift) & 0xfffu;
  if (trig) return;
  st.y = (x.flags >> kRawYShift) & 0x7ffu;
  st.bx = x.bx, st.bp = x.flags & kRawBp ? 1 : 0;
}
// The decode step of one camera (job[1].n_bytes == 0) or of both.  place(want, repeat, dc) says where job[k]'s records go
// and how many fit there: one per word to begin with.  The chain runs and is waited for; when the reduce pass reports
// more records than a buffer holds, no stamp is BAD and every count stays within repeat_up_to (kRawNoRepeat: the records
// lie where they cannot be given more room; SIZE_MAX: whatever comes), place(counts, true, dc) makes room and the emit
// launch is repeated.  r[k], dc[k]: the
// result block and the records of job[k]; the cameras' states are as they were (raw_commit).
constexpr size_t kRawNoRepeat = 0;
extern "C++" template <class Place>
int raw_run(esvio_fe_ctx* c, int format, int space, int64_t t_offset_us, const RawJob job[2], const int cam_of[2], bool trig,
            size_t repeat_up_to, Place place, RawResult r[2], DecodedCam dc[2]) {
  const size_t wb = raw_word_bytes(format);
  const size_t first[2] = {job[0].n_bytes / wb, job[1].n_bytes / wb};
  if (int rc = place(first, false, dc)) return rc;
  RawArgs a;
  if (int rc = raw_enqueue(c, format, space, t_offset_us, job, dc, cam_of, &a, r, trig)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (!r[0].bad && !r[1].bad && (r[0].events > dc[0].cap || r[1].events > dc[1].cap) && r[0].events <= repeat_up_to &&
      r[1].events <= repeat_up_to) {
    const size_t need[2] = {r[0].events, r[1].events};
    if (int rc = place(need, true, dc)) return rc;
    if (int rc = raw_emit_again(c, &a, job, dc, r, trig)) return rc;
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  }
  if (c->prof_on) resolve_profile(c);
  for (int k = 0; k < 2; k++) {
    const uint64_t ticks = r[k].events ? (uint64_t)r[k].last_t : 0;  // microseconds
    dc[k].events = r[k].events, dc[k].bad = r[k].bad;
    dc[k].sec = (uint32_t)(ticks / 1000000u), dc[k].nsec = (uint32_t)(ticks % 1000000u * 1000u);
  }
  return 0;
}

// esvio_fe_decode_raw, and esvio_fe_decode_triggers (trig: the trigger chain, the camera's trigger-decoder state, one
// record per word at the most, a dst that is always the host's) behind the null-handle check
int raw_decode(esvio_fe_ctx* c, bool trig, int cam, int format, const void* words, size_t n_bytes, int space, int64_t t_offset_us,
               void* dst, size_t dst_cap, int dst_space, esvio_fe_raw_info* info) {
  const char* who = trig ? "decode_triggers" : "decode_raw";
  const char* noun = trig ? "triggers" : "events";
  const char* state = trig ? "trigger-decoder state" : "decoder state";
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  const esvio_fe_ctx::Raw::State& st = trig ? c->rawdec.trig_st[cam] : c->rawdec.st[cam];
  raw_info_clear(info, st.wraps);
  if (int rc = raw_args_check(c, who, format, words, n_bytes, space, t_offset_us)) return rc;
  if (int rc = dst_check(c, who, "dst", dst, dst_cap, dst_space)) return rc;
  if (!n_bytes) return 0;
  HIPCHK(c, hipSetDevice(c->dev));
  const size_t per_word = n_bytes / raw_word_bytes(format), bound = trig ? per_word : raw_bound(format, n_bytes);
  const size_t room = std::min(dst_cap, bound);
  RawJob job[2];
  job[0].words = words, job[0].n_bytes = n_bytes;
  // The records behind a host dst lie in the decode scratch, never more than dst has room for.  Events: as many as the
  // scratch holds, one per word at least; triggers (they are few): 4096 at the most to begin with
  auto place = [&](const size_t want[2], bool repeat, DecodedCam dc[2]) -> int {
    if (dst_space == ESVIO_FE_DEVICE) {  // the caller's own buffer, as it is
      dc[0].d = (EventRec*)dst, dc[0].cap = room;
      return 0;
    }
    size_t n = want[0];
    if (!repeat) n = trig ? std::max<size_t>(std::min<size_t>(room, 4096), 1) : std::min(room, std::max(c->rawdec.dec[cam].cap, per_word));
    if (int rc = dec_scratch(c, cam, n, &dc[0])) return rc;
    if (!repeat) dc[0].cap = std::min(dc[0].cap, room);
    return 0;
  };
  const int cam_of[2] = {cam, cam};
  RawResult r[2] = {};
  DecodedCam dc[2];
  // (a repeat is for the scratch alone, and only for counts dst has room for: more are refused below, unrepeated)
  const size_t repeat_up_to = dst_space == ESVIO_FE_HOST ? dst_cap : kRawNoRepeat;
  if (int rc = raw_run(c, format, space, t_offset_us, job, cam_of, trig, repeat_up_to, place, r, dc)) return rc;
  raw_info_fill(info, r[0], st.wraps);
  if (dc[0].bad)
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu %s have a stamp outside [0, 2^32 s); the camera's %s is as it was", who, dc[0].bad,
                dc[0].events, noun, state);
  if (dc[0].events > dst_cap)
    return fail(c, ESVIO_FE_EINVAL, "%s: the chunk holds %zu %s, dst has room for %zu; the camera's %s is as it was", who, dc[0].events, noun,
                dst_cap, state);
  if (dst_space == ESVIO_FE_HOST)
    if (int rc = deliver_host(c, 1, &dst, dc)) return rc;
  raw_commit(c, cam, r[0], trig);
  if (info) info->wraps = st.wraps;
  return 0;
}
}  // namespace

int esvio_fe_raw_tile_bytes(void) { return (int)kRawTileBytes; }

int esvio_fe_decode_raw(esvio_fe_handle c, int cam, int format, const void* words, size_t n_bytes, int space,
                        int64_t t_offset_us, esvio_fe_event* dst, size_t dst_cap, int dst_space, esvio_fe_raw_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  return raw_decode(c, false, cam, format, words, n_bytes, space, t_offset_us, dst, dst_cap, dst_space, info);
}

// ---- external triggers: the decode chain with the trigger classifier, the camera's trigger-decoder state (include/esvio_fe.h)
static_assert(sizeof(esvio_fe_trigger) == sizeof(EventRec), "trigger records travel through the decode chain's 16-byte slots");
int esvio_fe_decode_triggers(esvio_fe_handle c, int cam, int format, const void* words, size_t n_bytes, int space,
                             int64_t t_offset_us, esvio_fe_trigger* dst, size_t dst_cap, esvio_fe_trigger_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  esvio_fe_raw_info ri{};  // (a trigger word counts as one "event" of the chain)
  const int rc = raw_decode(c, true, cam, format, words, n_bytes, space, t_offset_us, dst, dst_cap, ESVIO_FE_HOST, info ? &ri : nullptr);
  if (info && (cam == 0 || cam == 1)) {
    info->triggers = ri.events, info->untimed = ri.untimed, info->bad = ri.bad, info->wraps = ri.wraps;
    if (ri.events) info->first_t_us = ri.first_t_us, info->last_t_us = ri.last_t_us;
  }
  return rc;
}

// ---- the .raw file's ASCII header (include/esvio_fe.h has the rule): host only
namespace {
// the text of a header line behind '%' and blanks, in front of "\n" / "\r\n"
bool hdr_key(const char*& p, const char* end, const char* key) {
  const size_t k = strlen(key);
  if ((size_t)(end - p) < k || memcmp(p, key, k) != 0) return false;
  if ((size_t)(end - p) > k && p[k] != ' ' && p[k] != '\t') return false;
  p += k;
  while (p < end && (*p == ' ' || *p == '\t')) p++;
  return true;
}
int hdr_format(const char* p, const char* end) {  // "EVT2" / "EVT21" / "EVT3", "2.0" / "2.1" / "3.0": the whole token
  const std::string t(p, end);
  if (t == "EVT2" || t == "2.0") return ESVIO_FE_RAW_EVT2;
  if (t == "EVT21" || t == "2.1") return ESVIO_FE_RAW_EVT21;
  if (t == "EVT3" || t == "3.0") return ESVIO_FE_RAW_EVT3;
  return 0;
}
bool hdr_int(const char* p, const char* end, int32_t* out) {  // decimal digits only, 1 .. 2^30
  if (p == end) return false;
  int64_t v = 0;
  for (; p < end; p++) {
    if (*p < '0' || *p > '9') return false;
    v = v * 10 + (*p - '0');
    if (v > (1 << 30)) return false;
  }
  *out = (int32_t)v;
  return v > 0;
}
}  // namespace

int esvio_fe_raw_header(const void* bytes, size_t n, esvio_fe_raw_header_info* out) {
  if (!out || (n && !bytes)) return ESVIO_FE_EINVAL;
  *out = esvio_fe_raw_header_info{};
  const char* b = (const char*)bytes;
  int evt_format = 0, fmt_format = 0;
  size_t pos = 0;
  bool ended = false;
  while (!ended) {
    if (pos == n) break;                   // behind a whole line that is not "% end" (or no byte at all): not known yet
    if (b[pos] != '%') { ended = true; break; }
    const char* nl = (const char*)memchr(b + pos, '\n', n - pos);
    if (!nl) break;                        // inside a header line
    const char* p = b + pos + 1;
    const char* end = nl;
    if (end > p && end[-1] == '\r') end--;
    while (p < end && (*p == ' ' || *p == '\t')) p++;
    while (end > p && (end[-1] == ' ' || end[-1] == '\t')) end--;
    pos = (size_t)(nl - b) + 1;
    if (end - p == 3 && memcmp(p, "end", 3) == 0) {
      ended = true;
    } else if (hdr_key(p, end, "evt")) {
      if (int f = hdr_format(p, end)) evt_format = f;
    } else if (hdr_key(p, end, "format")) {
      const char* semi = (const char*)memchr(p, ';', (size_t)(end - p));
      if (int f = hdr_format(p, semi ? semi : end)) fmt_format = f;
      while (semi) {  // ;key=value
        const char* k = semi + 1;
        semi = (const char*)memchr(k, ';', (size_t)(end - k));
        const char* ke = semi ? semi : end;
        const char* eq = (const char*)memchr(k, '=', (size_t)(ke - k));
        if (!eq) continue;
        const std::string key(k, eq);
        int32_t v;
        if (key == "width" && hdr_int(eq + 1, ke, &v)) out->width = v;
        if (key == "height" && hdr_int(eq + 1, ke, &v)) out->height = v;
      }
    } else if (hdr_key(p, end, "geometry")) {
      const char* x = (const char*)memchr(p, 'x', (size_t)(end - p));
      int32_t w, h;
      if (x && hdr_int(p, x, &w) && hdr_int(x + 1, end, &h)) out->width = w, out->height = h;
    }
  }
  out->payload_offset = pos;
  out->format = fmt_format ? fmt_format : evt_format;
  out->complete = ended ? 1 : 0;
  return 0;
}

int esvio_fe_track_raw(esvio_fe_handle c, int format, const void* left, size_t left_bytes, const void* right,
                       size_t right_bytes, int space, int64_t t_offset_us, int pub_this_frame,
                       const esvio_fe_filter_params* filter, const esvio_fe_motion* motion, esvio_fe_tracks* out,
                       esvio_fe_batch_info* info_out, esvio_fe_raw_info raw[2]) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info_out) *info_out = esvio_fe_batch_info{};
  const void* words[2] = {left, right};
  const size_t nb[2] = {left_bytes, right_bytes};
  for (int cam = 0; cam < 2; cam++) {
    if (raw) raw_info_clear(&raw[cam], c->rawdec.st[cam].wraps);
    if (int rc = raw_args_check(c, cam ? "track_raw (right)" : "track_raw (left)", format, words[cam], nb[cam], space, t_offset_us)) return rc;
  }
  if (filter)
    if (int rc = baf_prm_check(c, filter, "track_raw")) return rc;
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "track_raw: batches are announced on this handle (decode into memory of your own)");
  if (!nb[0] && !nb[1]) return 0;  // nothing to decode: no left event, nothing tracked
  HIPCHK(c, hipSetDevice(c->dev));
  RawJob job[2];
  for (int cam = 0; cam < 2; cam++) job[cam].words = words[cam], job[cam].n_bytes = nb[cam];
  auto place = [&](const size_t want[2], bool, DecodedCam dc[2]) { return track_place(c, filter != nullptr, want, dc); };
  const int cam_of[2] = {0, 1};
  RawResult r[2] = {};
  DecodedCam dc[2];
  if (int rc = raw_run(c, format, space, t_offset_us, job, cam_of, false, SIZE_MAX, place, r, dc)) return rc;
  for (int cam = 0; cam < 2; cam++)
    if (raw && nb[cam]) raw_info_fill(&raw[cam], r[cam], c->rawdec.st[cam].wraps);
  return track_decoded(c, "track_raw", "decoder states", dc, filter, motion, pub_this_frame, out, info_out, [&] {
    for (int cam = 0; cam < 2; cam++)
      if (nb[cam]) {
        raw_commit(c, cam, r[cam]);
        if (raw) raw[cam].wraps = c->rawdec.st[cam].wraps;
      }
  });
}

// ---- text event files (the rule: include/esvio_fe.h; the classifier and the carry step: fe_text.h; the chain: fe_kernels.h)
namespace {
namespace tx = esvio::text;
static_assert(sizeof(tx::ImuSample) == sizeof(esvio_fe_imu_sample) && offsetof(tx::ImuSample, gyr) == offsetof(esvio_fe_imu_sample, gyr),
              "fe_text.h writes esvio_fe_imu_sample's bytes");
static_assert(ESVIO_FE_TEXT_TXYP == tx::kTxyp && ESVIO_FE_TEXT_XYPT == tx::kXypt && ESVIO_FE_TEXT_SEC_DECIMAL == tx::kSecDecimal &&
                  ESVIO_FE_TEXT_INT_US == tx::kIntUs && ESVIO_FE_TEXT_INT_NS == tx::kIntNs && ESVIO_FE_TEXT_END == tx::kEnd &&
                  ESVIO_FE_TEXT_SKIP_MALFORMED == tx::kSkipMalformed,
              "fe_text.h's constants are the header's");
struct TextJob {  // one camera's part of a call
  const void* bytes = nullptr;
  size_t n_bytes = 0;
  bool active = false;
  tx::State st{};  // the camera's state behind the chunk: taken over when the call succeeds
};

int text_args_check(esvio_fe_ctx* c, const char* who, const esvio_fe_text_format* fmt, const void* bytes, size_t n_bytes, int space,
                    int64_t t_offset_ns) {
  if (!fmt) return fail(c, ESVIO_FE_EINVAL, "%s: fmt is null", who);
  if (fmt->order != ESVIO_FE_TEXT_TXYP && fmt->order != ESVIO_FE_TEXT_XYPT)
    return fail(c, ESVIO_FE_EINVAL, "%s: order must be ESVIO_FE_TEXT_TXYP or ESVIO_FE_TEXT_XYPT (got %d)", who, fmt->order);
  if (fmt->time != ESVIO_FE_TEXT_SEC_DECIMAL && fmt->time != ESVIO_FE_TEXT_INT_US && fmt->time != ESVIO_FE_TEXT_INT_NS)
    return fail(c, ESVIO_FE_EINVAL, "%s: time must be ESVIO_FE_TEXT_SEC_DECIMAL, _INT_US or _INT_NS (got %d)", who, fmt->time);
  if (fmt->flags & ~(ESVIO_FE_TEXT_END | ESVIO_FE_TEXT_SKIP_MALFORMED)) return fail(c, ESVIO_FE_EINVAL, "%s: unknown bits in flags (0x%x)", who, fmt->flags);
  if (fmt->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "%s: reserved must be 0", who);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  const int64_t lim = (int64_t)1 << 62;
  if (t_offset_ns > lim || t_offset_ns < -lim) return fail(c, ESVIO_FE_EINVAL, "%s: |t_offset_ns| must be <= 2^62", who);
  if (n_bytes > kRawMaxBytes) return fail(c, ESVIO_FE_EINVAL, "%s: a chunk holds at most 2^28 bytes", who);
  if (n_bytes && !bytes) return fail(c, ESVIO_FE_EINVAL, "%s: bytes is null", who);
  return 0;
}
size_t text_bound(size_t n_bytes) { return (n_bytes + tx::kMaxTail) / 8 + 1; }  // the shortest event line is 8 bytes
uint32_t text_tiles(size_t virt_bytes) { return (uint32_t)std::max<size_t>((virt_bytes + kTextTileBytes - 1) / kTextTileBytes, 1); }
// has the call anything to do?  Bytes, or with END a state that is not fresh
bool text_active(const esvio_fe_ctx* c, int cam, const esvio_fe_text_format& fmt, size_t n_bytes) {
  return n_bytes || ((fmt.flags & ESVIO_FE_TEXT_END) && (c->text.st[cam].len || c->text.st[cam].skip));
}

int text_ensure(esvio_fe_ctx* c, int cam, size_t n_bytes, bool copied_src) {
  esvio_fe_ctx::Text& t = c->text;
  t.used = true;
  if (!t.res)
    if (int rc = t.res.alloc(c, 2)) return rc;
  if (int rc = t.sums[cam].grow(c, text_tiles(n_bytes + tx::kMaxTail))) return rc;
  return copied_src ? t.src[cam].grow(c, std::max<size_t>(n_bytes, 1)) : 0;
}
// esvio_fe_reserve for a handle that decodes text: per camera the scratch of a file of up to 16 bytes per event (include/esvio_fe.h)
int text_reserve(esvio_fe_ctx* c, const size_t events[2], bool host_batches) {
  for (int cam = 0; cam < 2 && c->text.used; cam++)
    if (int rc = text_ensure(c, cam, events[cam] * 16, host_batches)) return rc;
  return 0;
}
void text_state_reset(esvio_fe_ctx* c) { c->text.st[0] = c->text.st[1] = tx::State(); }

TextCarry text_carry_of(const tx::State& st) {
  TextCarry k{};
  memcpy(k.tail_w, st.tail, st.len);
  k.len = st.len, k.skip = st.skip, k.skip_len = st.skip_len;
  return k;
}
void text_state_of(const TextCarry& k, tx::State* st) {
  *st = tx::State();
  st->len = std::min<uint32_t>(k.len, tx::kMaxTail), st->skip = k.skip ? 1 : 0, st->skip_len = k.skip_len;
  memcpy(st->tail, k.tail_w, st->len);
}
void text_info_clear(esvio_fe_text_info* info, const tx::State& st) {
  if (!info) return;
  info->events = info->lines = info->comments = info->blank = info->malformed = info->bad = 0;
  info->carried = st.len, info->reserved = 0;
}
void text_info_fill(esvio_fe_text_info* info, const TextResult& r) {  // the counts: exact whether the call succeeds or not
  if (!info) return;
  info->events = r.events, info->comments = r.comments, info->blank = r.blank, info->malformed = r.malformed, info->bad = r.bad;
  info->lines = r.events + r.comments + r.blank + r.malformed;
  if (r.malformed) info->first_malformed = r.first_malformed;
}
void text_info_done(esvio_fe_text_info* info, const TextResult& r, const tx::State& st) {  // what a call that succeeded adds
  if (!info) return;
  if (r.events) info->first_t_ns = r.first_t, info->last_t_ns = r.last_t;
  info->carried = st.len;
}

// The decode step of one camera (job[1].active == false) or of both: place(want, dc) says where job[k]'s records go —
// want[k] is the bound, so no emit is ever repeated —, the chain runs on the current stream and is waited for.  r[k],
// dc[k]: the result block and the records of job[k]; job[k].st: the state behind the chunk; the cameras' states are as
// they were.
extern "C++" template <class Place>
int text_run(esvio_fe_ctx* c, const esvio_fe_text_format& fmt, int space, int64_t t_offset_ns, TextJob job[2], const int cam_of[2],
             Place place, TextResult r[2], DecodedCam dc[2]) {
  esvio_fe_ctx::Text& t = c->text;
  const size_t want[2] = {job[0].active ? text_bound(job[0].n_bytes) : 0, job[1].active ? text_bound(job[1].n_bytes) : 0};
  if (int rc = place(want, dc)) return rc;
  hipStream_t s = cur_stream(c);
  TextArgs a{};
  a.order = fmt.order, a.time = fmt.time;
  uint64_t bytes = 0, cap_bytes = 0;
  for (int k = 0; k < 2; k++) {
    if (!job[k].active) continue;
    const int cam = cam_of[k];
    const uint8_t* d_bytes = (const uint8_t*)job[k].bytes;
    if (space == ESVIO_FE_HOST && job[k].n_bytes) {
      const bool in_place = c->rawdec.pinned_copy < 0 ? job[k].n_bytes <= kRawPinnedInPlaceBytes : c->rawdec.pinned_copy == 0;
      d_bytes = in_place ? pinned_device_ptr((const uint8_t*)job[k].bytes, job[k].n_bytes) : nullptr;
      if (!d_bytes) {
        if (int rc = text_ensure(c, cam, job[k].n_bytes, true)) return rc;
        HIPCHK(c, hipMemcpyAsync(t.src[cam], job[k].bytes, job[k].n_bytes, hipMemcpyHostToDevice, s));
        d_bytes = t.src[cam];
      }
    }
    if (int rc = text_ensure(c, cam, job[k].n_bytes, false)) return rc;
    TextCam& tc = a.cam[k];
    tc.bytes = d_bytes, tc.n_bytes = (uint32_t)job[k].n_bytes;
    tc.carry = text_carry_of(t.st[cam]);
    tc.tiles = text_tiles((size_t)tc.carry.len + job[k].n_bytes);
    tc.end = fmt.flags & ESVIO_FE_TEXT_END ? 1u : 0u, tc.t_offset = t_offset_ns;
    tc.sums = t.sums[cam], tc.dst = dc[k].d, tc.dst_cap = (uint32_t)std::min<size_t>(dc[k].cap, 0xffffffffu);
    tc.res = t.res + cam;
    bytes += tc.carry.len + job[k].n_bytes;
    cap_bytes += std::min(dc[k].cap, want[k]) * 16;
  }
  const uint64_t tile_bytes = (uint64_t)(a.cam[0].tiles + a.cam[1].tiles) * sizeof(TextTile);
  {
    ScopedKernel k(c, K_TEXT_COUNT, bytes + tile_bytes);
    launch_text_count(s, a);
  }
  {
    ScopedKernel k(c, K_TEXT_PLACE, 2 * tile_bytes);
    launch_text_place(s, a);
  }
  {  // (booked as if every record the buffers have room for were written: the count is not known here)
    ScopedKernel k(c, K_TEXT_EMIT, bytes + cap_bytes);
    launch_text_emit(s, a);
  }
  for (int k = 0; k < 2; k++)
    if (job[k].active) HIPCHK(c, hipMemcpyAsync(&r[k], a.cam[k].res, sizeof(TextResult), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  for (int k = 0; k < 2; k++) {
    if (!job[k].active) continue;
    dc[k].events = (size_t)r[k].events, dc[k].bad = r[k].bad;
    dc[k].sec = r[k].last_sec, dc[k].nsec = r[k].last_nsec;
    if (fmt.flags & ESVIO_FE_TEXT_END) {
      job[k].st = tx::State();
    } else if (space == ESVIO_FE_HOST) {  // the host can read the chunk: the carry step
      job[k].st = t.st[cam_of[k]];
      tx::carry(&job[k].st, (const uint8_t*)job[k].bytes, job[k].n_bytes);
    } else {
      text_state_of(r[k].state, &job[k].st);
    }
  }
  return 0;
}
// a malformed line without SKIP_MALFORMED refuses the call
int text_malformed_check(esvio_fe_ctx* c, const char* who, const esvio_fe_text_format& fmt, const TextResult r[2], int n, const char* states) {
  if (fmt.flags & ESVIO_FE_TEXT_SKIP_MALFORMED) return 0;
  for (int k = 0; k < n; k++)
    if (r[k].malformed)
      return fail(c, ESVIO_FE_EINVAL, "%s: %llu malformed line(s)%s, the first at byte offset %lld of the chunk; %s as before the call", who,
                  r[k].malformed, n > 1 ? (k ? " in the right camera" : " in the left camera") : "", r[k].first_malformed, states);
  return 0;
}
}  // namespace

int esvio_fe_decode_text(esvio_fe_handle c, int cam, const esvio_fe_text_format* fmt, const void* bytes, size_t n_bytes, int space,
                         int64_t t_offset_ns, esvio_fe_event* dst, size_t dst_cap, int dst_space, esvio_fe_text_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "decode_text";
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  text_info_clear(info, c->text.st[cam]);
  if (int rc = text_args_check(c, who, fmt, bytes, n_bytes, space, t_offset_ns)) return rc;
  if (int rc = dst_check(c, who, "dst", dst, dst_cap, dst_space)) return rc;
  if (!text_active(c, cam, *fmt, n_bytes)) return 0;
  HIPCHK(c, hipSetDevice(c->dev));
  TextJob job[2];
  job[0].bytes = bytes, job[0].n_bytes = n_bytes, job[0].active = true;
  auto place = [&](const size_t want[2], DecodedCam dc[2]) -> int {
    const size_t room = std::min(dst_cap, want[0]);
    if (dst_space == ESVIO_FE_DEVICE) {  // the caller's own buffer, as it is
      dc[0].d = (EventRec*)dst, dc[0].cap = room;
      return 0;
    }
    if (int rc = dec_scratch(c, cam, std::max<size_t>(room, 1), &dc[0])) return rc;
    dc[0].cap = room;
    return 0;
  };
  const int cam_of[2] = {cam, cam};
  TextResult r[2] = {};
  DecodedCam dc[2];
  if (int rc = text_run(c, *fmt, space, t_offset_ns, job, cam_of, place, r, dc)) return rc;
  text_info_fill(info, r[0]);
  if (int rc = text_malformed_check(c, who, *fmt, r, 1, "the camera's state is")) return rc;
  if (dc[0].bad)
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events have a stamp outside [0, 2^32 s); the camera's state is as it was", who, dc[0].bad,
                dc[0].events);
  if (dc[0].events > dst_cap)
    return fail(c, ESVIO_FE_EINVAL, "%s: the chunk holds %zu events, dst has room for %zu; the camera's state is as it was", who, dc[0].events,
                dst_cap);
  if (dst_space == ESVIO_FE_HOST) {
    void* to = dst;
    if (int rc = deliver_host(c, 1, &to, dc)) return rc;
  }
  c->text.st[cam] = job[0].st;
  text_info_done(info, r[0], job[0].st);
  return 0;
}

int esvio_fe_track_text(esvio_fe_handle c, const esvio_fe_text_format* fmt, const void* left, size_t left_bytes, const void* right,
                        size_t right_bytes, int space, int64_t t_offset_ns, int pub_this_frame, const esvio_fe_filter_params* filter,
                        const esvio_fe_motion* motion, esvio_fe_tracks* out, esvio_fe_batch_info* info_out, esvio_fe_text_info text[2]) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info_out) *info_out = esvio_fe_batch_info{};
  const void* src[2] = {left, right};
  const size_t nb[2] = {left_bytes, right_bytes};
  for (int cam = 0; cam < 2; cam++) {
    if (text) text_info_clear(&text[cam], c->text.st[cam]);
    if (int rc = text_args_check(c, cam ? "track_text (right)" : "track_text (left)", fmt, src[cam], nb[cam], space, t_offset_ns)) return rc;
  }
  if (filter)
    if (int rc = baf_prm_check(c, filter, "track_text")) return rc;
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "track_text: batches are announced on this handle (decode into memory of your own)");
  TextJob job[2];
  for (int cam = 0; cam < 2; cam++) job[cam].bytes = src[cam], job[cam].n_bytes = nb[cam], job[cam].active = text_active(c, cam, *fmt, nb[cam]);
  if (!job[0].active && !job[1].active) return 0;  // nothing to decode: no left event, nothing tracked
  HIPCHK(c, hipSetDevice(c->dev));
  auto place = [&](const size_t want[2], DecodedCam dc[2]) { return track_place(c, filter != nullptr, want, dc); };
  const int cam_of[2] = {0, 1};
  TextResult r[2] = {};
  DecodedCam dc[2];
  if (int rc = text_run(c, *fmt, space, t_offset_ns, job, cam_of, place, r, dc)) return rc;
  for (int cam = 0; cam < 2; cam++)
    if (text && job[cam].active) text_info_fill(&text[cam], r[cam]);
  if (int rc = text_malformed_check(c, "track_text", *fmt, r, 2, "nothing was tracked, both cameras' states are")) return rc;
  return track_decoded(c, "track_text", "text states", dc, filter, motion, pub_this_frame, out, info_out, [&] {
    for (int cam = 0; cam < 2; cam++)
      if (job[cam].active) {
        c->text.st[cam] = job[cam].st;
        if (text) text_info_done(&text[cam], r[cam], job[cam].st);
      }
  });
}

int esvio_fe_text_imu(const void* bytes, size_t n, int64_t t_offset_ns, esvio_fe_imu_sample* out, size_t cap, size_t* n_out) {
  const int64_t lim = (int64_t)1 << 62;
  if (!n_out || (n && !bytes) || (cap && !out) || t_offset_ns > lim || t_offset_ns < -lim) return ESVIO_FE_EINVAL;
  return tx::parse_imu((const uint8_t*)bytes, n, t_offset_ns, (tx::ImuSample*)out, cap, n_out) ? ESVIO_FE_EINVAL : ESVIO_FE_OK;
}
int esvio_fe_text_images(const void* bytes, size_t n, int64_t t_offset_ns, int64_t* stamps_ns, uint64_t* path_off, uint32_t* path_len,
                         size_t cap, size_t* n_out) {
  const int64_t lim = (int64_t)1 << 62;
  if (!n_out || (n && !bytes) || (cap && (!stamps_ns || !path_off || !path_len)) || t_offset_ns > lim || t_offset_ns < -lim) return ESVIO_FE_EINVAL;
  return tx::parse_images((const uint8_t*)bytes, n, t_offset_ns, stamps_ns, path_off, path_len, cap, n_out) ? ESVIO_FE_EINVAL : ESVIO_FE_OK;
}
int esvio_fe_text_limits(esvio_fe_text_limits_info* out) {
  if (!out) return ESVIO_FE_EINVAL;
  *out = esvio_fe_text_limits_info{(int32_t)kTextTileBytes, (int32_t)tx::kMaxBody, (int32_t)tx::kMaxTail, 0};
  return 0;
}
int esvio_fe_scan_lanes(esvio_fe_scan_lanes_info* out) {
  if (!out) return ESVIO_FE_EINVAL;
  *out = esvio_fe_scan_lanes_info{(int32_t)kRawScanLanes,   (int32_t)kAedatScanLanes, (int32_t)kTextScanLanes, (int32_t)kSliceScanLanes,
                                  (int32_t)kBafScanThreads, (int32_t)kVocScanLanes,   (int32_t)kBafBlock,      (int32_t)kVocScanTile};
  return 0;
}
// the shared sort alone, in device memory of the call's own (include/esvio_fe_test.h); the driver is radix_sort_pairs as it is
int esvio_fe_sort_pairs(esvio_fe_handle c, const uint32_t* keys, const uint32_t* vals, int64_t n, int passes, int bits,
                        int64_t n_dev, uint32_t* out_keys, uint32_t* out_vals, int32_t* out_err, uint32_t* out_tickets) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "sort_pairs";
  if (bits < 1 || bits > kRadixMaxBits || passes < 1 || passes > kRadixMaxPasses)
    return fail(c, ESVIO_FE_EINVAL, "%s: bits must be in 1..%d and passes in 1..%d (got %d, %d)", who, kRadixMaxBits, kRadixMaxPasses, bits, passes);
  if (n < 0 || n >= ((int64_t)1 << 30) || n_dev < -1 || n_dev > 0xffffffffll)
    return fail(c, ESVIO_FE_EINVAL, "%s: n must be in 0..2^30 - 1 and n_dev -1 or a 32-bit count (got %lld, %lld)", who, (long long)n, (long long)n_dev);
  if (!out_err || !out_tickets || (n && (!keys || !vals || !out_keys || !out_vals))) return fail(c, ESVIO_FE_EINVAL, "%s: a null array", who);
  HIPCHK(c, hipSetDevice(c->dev));
  hipStream_t s = cur_stream(c);
  const uint32_t n32 = (uint32_t)n, m = n_dev < 0 ? n32 : (uint32_t)std::min<int64_t>(n, n_dev);  // the pairs that take part
  DevBuf<uint32_t> dk[2], dv[2], scratch, count;
  for (int k = 0; k < 2; k++) {
    if (int rc = dk[k].alloc(c, n32)) return rc;
    if (int rc = dv[k].alloc(c, n32)) return rc;
  }
  const size_t words = sort_scratch_words(n32);
  if (int rc = scratch.alloc(c, words)) return rc;
  if (int rc = count.alloc(c, 1)) return rc;
  std::vector<uint32_t> h(words, 0u);  // the digit counts of the pairs that take part; tickets and look-back words clear
  for (int p = 0; p < passes; p++)
    for (uint32_t i = 0; i < m; i++) h[((size_t)p << bits) + ((keys[i] >> (p * bits)) & ((1u << bits) - 1u))]++;
  HIPCHK(c, hipMemcpyAsync(scratch, h.data(), words * 4, hipMemcpyHostToDevice, s));
  if (n32) {
    // the first buffer of each pair holds the whole input, the second the caller's out_*: a position no pass writes keeps
    // what it held
    HIPCHK(c, hipMemcpyAsync(dk[0], keys, (size_t)n32 * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dv[0], vals, (size_t)n32 * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dk[1], out_keys, (size_t)n32 * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dv[1], out_vals, (size_t)n32 * 4, hipMemcpyHostToDevice, s));
  }
  const uint32_t count_value = (uint32_t)std::max<int64_t>(n_dev, 0);
  HIPCHK(c, hipMemcpyAsync(count, &count_value, 4, hipMemcpyHostToDevice, s));
  const int32_t err_before = c->pin[0].counts[3];  // (the passes raise the handle's word: given back as it was)
  c->pin[0].counts[3] = 0;
  const int cur = radix_sort_pairs(c, SortBufs{{dk[0], dk[1]}, {dv[0], dv[1]}, scratch, n_dev < 0 ? nullptr : count.p}, n32, passes, bits, false);
  if (n32) {
    HIPCHK(c, hipMemcpyAsync(out_keys, dk[cur], (size_t)n32 * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(out_vals, dv[cur], (size_t)n32 * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipMemcpyAsync(out_tickets, sort_scratch(scratch).tickets, (size_t)passes * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  *out_err = c->pin[0].counts[3];
  c->pin[0].counts[3] = err_before;
  return 0;
}
int esvio_fe_text_kernel_count(void) { return kTextKernels; }
const char* esvio_fe_text_kernel_name(int which) { return which >= 0 && which < kTextKernels ? kTextKernelNames[which] : ""; }
int esvio_fe_text_kernel_stats(esvio_fe_handle c, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c || which < 0 || which >= kTextKernels) return ESVIO_FE_EINVAL;
  if (c->prof_on) resolve_profile(c);
  const KStat& s = c->stats[K_TEXT_COUNT + which];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}

// ---- libcaer / AEDAT 3.1 packet streams (the rule: include/esvio_fe.h; the host walk: fe_aedat.h; the chain: fe_kernels.h)
namespace {
namespace ae = esvio::aedat;
static_assert(sizeof(ae::Run) == sizeof(AedatRun), "the walk's run table is the kernels'");
struct AedatJob {  // one camera's part of a call
  const void* bytes = nullptr;
  size_t n_bytes = 0;
  ae::Walk st{};   // the camera's state behind the chunk: taken over when the call succeeds
  ae::Out cnt;     // what the counting walk found: n_events, n_runs, the packets
};

int aedat_args_check(esvio_fe_ctx* c, const char* who, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags) {
  if (flags & ~(uint32_t)ESVIO_FE_AEDAT_KEEP_INVALID) return fail(c, ESVIO_FE_EINVAL, "%s: unknown bits in flags (0x%x)", who, flags);
  const int64_t lim = (int64_t)1 << 62;
  if (t_offset_ns > lim || t_offset_ns < -lim) return fail(c, ESVIO_FE_EINVAL, "%s: |t_offset_ns| must be <= 2^62", who);
  if (n_bytes > kRawMaxBytes) return fail(c, ESVIO_FE_EINVAL, "%s: a chunk holds at most 2^28 bytes", who);
  if (n_bytes && !bytes) return fail(c, ESVIO_FE_EINVAL, "%s: bytes is null", who);
  return 0;
}
// the counting walk: every header of the chunk checked, the records and runs counted, nothing stored, no state moved
int aedat_count_walk(esvio_fe_ctx* c, const char* who, int cam, AedatJob* j) {
  ae::Walk probe = c->aedat.ev_st[cam];
  j->cnt = ae::Out();
  if (!ae::walk(&probe, ae::kEvents, (const uint8_t*)j->bytes, j->n_bytes, 0, 0, &j->cnt))
    return fail(c, ESVIO_FE_EINVAL, "%s: malformed packet header (%s); the camera's state is as it was", who, j->cnt.why);
  return 0;
}
void aedat_info_packets(esvio_fe_aedat_info* info, const ae::Out& o) {
  if (info) info->polarity_packets = o.polarity_packets, info->other_packets = o.other_packets;
}
uint32_t aedat_tiles(size_t n) { return (uint32_t)((n + kAedatTile - 1) / kAedatTile); }
size_t aedat_runs_offset(size_t n_events) { return (n_events * 8 + 15) & ~(size_t)15; }
int aedat_ensure(esvio_fe_ctx* c, int cam, size_t n_events, size_t n_runs) {
  esvio_fe_ctx::Aedat& A = c->aedat;
  A.used = true;
  if (!A.res)
    if (int rc = A.res.alloc(c, 2)) return rc;
  const size_t bytes = aedat_runs_offset(n_events) + n_runs * sizeof(AedatRun);
  if (int rc = A.sums[cam].grow(c, aedat_tiles(n_events))) return rc;
  if (int rc = A.h_pack[cam].grow(c, bytes)) return rc;
  return A.d_pack[cam].grow(c, bytes);
}
// esvio_fe_reserve for a handle that decodes AEDAT streams: per camera the scratch of a chunk of max_events polarity records, each a run
int aedat_reserve(esvio_fe_ctx* c, const size_t events[2]) {
  for (int cam = 0; cam < 2 && c->aedat.used; cam++)
    if (int rc = aedat_ensure(c, cam, events[cam], events[cam])) return rc;
  return 0;
}
void aedat_state_reset(esvio_fe_ctx* c) {
  for (int cam = 0; cam < 2; cam++) c->aedat.ev_st[cam] = c->aedat.side_st[cam] = c->aedat.frame_st[cam] = ae::Walk{};
}
// The gathering walk and the chain of one camera (job[1].n_bytes == 0) or of both on the current stream, and the copies
// that bring the result blocks to the host; nothing is waited for.  dc[k].d, cap: where job[k]'s records go.  A camera
// whose chunk completes no polarity record takes no part on the device.
int aedat_enqueue(esvio_fe_ctx* c, int64_t t_offset_ns, uint32_t flags, AedatJob job[2], const DecodedCam dc[2], const int cam_of[2],
                  AedatResult res[2]) {
  esvio_fe_ctx::Aedat& A = c->aedat;
  hipStream_t s = cur_stream(c);
  const bool keep = (flags & ESVIO_FE_AEDAT_KEEP_INVALID) != 0;
  AedatArgs a{};
  uint64_t n_all = 0, cap_all = 0;
  for (int k = 0; k < 2; k++) {
    if (!job[k].n_bytes) continue;
    const int cam = cam_of[k];
    const size_t n = (size_t)job[k].cnt.n_events, n_runs = (size_t)job[k].cnt.n_runs, roff = aedat_runs_offset(n);
    job[k].st = A.ev_st[cam];
    ae::Out o;
    if (n) {
      if (int rc = aedat_ensure(c, cam, n, n_runs)) return rc;
      o.payload = A.h_pack[cam], o.events_cap = n;
      o.runs = (ae::Run*)(A.h_pack[cam] + roff), o.runs_cap = n_runs;
    }
    ae::walk(&job[k].st, ae::kEvents, (const uint8_t*)job[k].bytes, job[k].n_bytes, 0, 0, &o);  // (checked by the counting walk)
    if (!n) continue;
    HIPCHK(c, hipMemcpyAsync(A.d_pack[cam], A.h_pack[cam], roff + n_runs * sizeof(AedatRun), hipMemcpyHostToDevice, s));
    AedatCam& ac = a.cam[k];
    ac.rec = (const uint2*)A.d_pack[cam].p, ac.n = (uint32_t)n, ac.tiles = aedat_tiles(n);
    ac.runs = (const AedatRun*)(A.d_pack[cam].p + roff), ac.n_runs = (uint32_t)n_runs;
    ac.keep_invalid = keep, ac.t_offset = t_offset_ns, ac.sums = A.sums[cam];
    ac.dst = dc[k].d, ac.dst_cap = (uint32_t)std::min<size_t>(dc[k].cap, 0xffffffffu);
    ac.res = A.res + cam;
    n_all += n, cap_all += std::min(dc[k].cap, n);
    if (keep) HIPCHK(c, hipMemsetAsync(ac.res, 0, sizeof(AedatResult), s));  // (events = n: the host's own knowledge)
  }
  if (!n_all) return 0;
  const uint64_t tiles = a.cam[0].tiles + a.cam[1].tiles;
  if (!keep) {
    {
      ScopedKernel k(c, K_AEDAT_COUNT, n_all * 8 + tiles * 4);
      launch_aedat_count(s, a);
    }
    {
      ScopedKernel k(c, K_AEDAT_SCAN, tiles * 8);
      launch_aedat_scan(s, a);
    }
  }
  {  // (booked as if every record the buffers have room for were written: the count is not known here)
    ScopedKernel k(c, K_AEDAT_EMIT, n_all * 8 + cap_all * 16);
    launch_aedat_emit(s, a);
  }
  for (int k = 0; k < 2; k++)
    if (a.cam[k].tiles) HIPCHK(c, hipMemcpyAsync(&res[k], a.cam[k].res, sizeof(AedatResult), hipMemcpyDeviceToHost, s));
  return 0;
}
// behind the wait: what the host knows itself
void aedat_result_fix(const AedatJob& j, uint32_t flags, AedatResult* r) {
  if ((flags & ESVIO_FE_AEDAT_KEEP_INVALID) && j.cnt.n_events) r->events = (uint32_t)j.cnt.n_events, r->invalid = 0;
}
void aedat_info_fill(esvio_fe_aedat_info* info, const AedatResult& r) {
  if (!info) return;
  info->events = r.events, info->invalid = r.invalid, info->bad = r.bad;
  if (r.events && !r.bad) info->first_t_us = (int64_t)(r.first_t / 1000u), info->last_t_us = (int64_t)(r.last_t / 1000u);
}
void aedat_info_clear(esvio_fe_aedat_info* info) {
  if (info) info->events = info->invalid = info->bad = info->polarity_packets = info->other_packets = 0;
}
// The decode step of one camera (job[1].n_bytes == 0) or of both, behind their counting walks.  place(want, dc) says
// where job[k]'s records go: want[k] is the host-known count of the chunk's records, so nothing is repeated.  The
// gathering walk and the chain run and are waited for, and the host adds what it knows itself.  r[k], dc[k]: the result
// block and the records of job[k]; job[k].st: the walker behind the chunk, which the consumer takes over.
extern "C++" template <class Place>
int aedat_run(esvio_fe_ctx* c, int64_t t_offset_ns, uint32_t flags, AedatJob job[2], const int cam_of[2], Place place, AedatResult r[2],
              DecodedCam dc[2]) {
  const size_t want[2] = {(size_t)job[0].cnt.n_events, (size_t)job[1].cnt.n_events};
  if (int rc = place(want, dc)) return rc;
  if (int rc = aedat_enqueue(c, t_offset_ns, flags, job, dc, cam_of, r)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  for (int k = 0; k < 2; k++) {
    aedat_result_fix(job[k], flags, &r[k]);
    const uint64_t ticks = r[k].events ? r[k].last_t : 0;  // nanoseconds
    dc[k].events = r[k].events, dc[k].bad = r[k].bad;
    dc[k].sec = (uint32_t)(ticks / 1000000000u), dc[k].nsec = (uint32_t)(ticks % 1000000000u);
  }
  return 0;
}
}  // namespace

int esvio_fe_aedat_tile_events(void) { return (int)kAedatTile; }

int esvio_fe_aedat_header(const void* bytes, size_t n, esvio_fe_aedat_header_info* out) { return ae::file_header(bytes, n, out); }

int esvio_fe_decode_aedat(esvio_fe_handle c, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                          esvio_fe_event* dst, size_t dst_cap, int dst_space, esvio_fe_aedat_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  aedat_info_clear(info);
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "decode_aedat: cam must be 0 or 1 (got %d)", cam);
  if (int rc = aedat_args_check(c, "decode_aedat", bytes, n_bytes, t_offset_ns, flags)) return rc;
  if (int rc = dst_check(c, "decode_aedat", "dst", dst, dst_cap, dst_space)) return rc;
  if (!n_bytes) return 0;
  AedatJob job[2];
  job[0].bytes = bytes, job[0].n_bytes = n_bytes;
  if (int rc = aedat_count_walk(c, "decode_aedat", cam, &job[0])) return rc;
  aedat_info_packets(info, job[0].cnt);
  HIPCHK(c, hipSetDevice(c->dev));
  auto place = [&](const size_t want[2], DecodedCam dc[2]) -> int {
    const size_t room = std::min(dst_cap, want[0]);
    dc[0].d = (EventRec*)dst;
    if (dst_space == ESVIO_FE_HOST && room)  // the records behind a host dst: as many as it has room for
      if (int rc = dec_scratch(c, cam, room, &dc[0])) return rc;
    dc[0].cap = room;
    return 0;
  };
  const int cam_of[2] = {cam, cam};
  AedatResult r[2] = {};
  DecodedCam dc[2];
  if (int rc = aedat_run(c, t_offset_ns, flags, job, cam_of, place, r, dc)) return rc;
  aedat_info_fill(info, r[0]);
  if (dc[0].bad)
    return fail(c, ESVIO_FE_EINVAL, "decode_aedat: %llu of %zu events have a stamp outside [0, 2^32 s); the camera's state is as it was",
                dc[0].bad, dc[0].events);
  if (dc[0].events > dst_cap)
    return fail(c, ESVIO_FE_EINVAL, "decode_aedat: the chunk holds %zu events, dst has room for %zu; the camera's state is as it was",
                dc[0].events, dst_cap);
  void* const host_dst = dst;
  if (dst_space == ESVIO_FE_HOST)
    if (int rc = deliver_host(c, 1, &host_dst, dc)) return rc;
  c->aedat.ev_st[cam] = job[0].st;
  return 0;
}

int esvio_fe_aedat_side(esvio_fe_handle c, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                        esvio_fe_imu_sample* imu, size_t imu_cap, esvio_fe_trigger* trig, size_t trig_cap,
                        esvio_fe_aedat_side_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info) *info = esvio_fe_aedat_side_info{};
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "aedat_side: cam must be 0 or 1 (got %d)", cam);
  if (int rc = aedat_args_check(c, "aedat_side", bytes, n_bytes, t_offset_ns, flags)) return rc;
  if (imu_cap && !imu) return fail(c, ESVIO_FE_EINVAL, "aedat_side: imu is null");
  if (trig_cap && !trig) return fail(c, ESVIO_FE_EINVAL, "aedat_side: trig is null");
  if (!n_bytes) return 0;
  ae::Walk st = c->aedat.side_st[cam];
  ae::Out o;
  o.imu = imu, o.imu_cap = imu_cap, o.trig = trig, o.trig_cap = trig_cap;
  if (!ae::walk(&st, ae::kSide, (const uint8_t*)bytes, n_bytes, t_offset_ns, flags, &o))
    return fail(c, ESVIO_FE_EINVAL, "aedat_side: malformed packet header (%s); the camera's state is as it was", o.why);
  if (info) {
    info->imu = o.n_imu, info->triggers = o.n_trig, info->resets = o.resets, info->other_specials = o.other_specials;
    info->invalid = o.invalid, info->bad = o.bad;
    info->special_packets = o.special_packets, info->imu_packets = o.imu_packets, info->other_packets = o.other_packets;
  }
  if (o.bad)
    return fail(c, ESVIO_FE_EINVAL, "aedat_side: %llu samples or triggers have a stamp outside [0, 2^32 s); the camera's state is as it was",
                (unsigned long long)o.bad);
  if (o.n_imu > imu_cap || o.n_trig > trig_cap)
    return fail(c, ESVIO_FE_EINVAL, "aedat_side: the chunk holds %llu samples and %llu triggers, there is room for %zu and %zu; the camera's state is as it was",
                (unsigned long long)o.n_imu, (unsigned long long)o.n_trig, imu_cap, trig_cap);
  c->aedat.side_st[cam] = st;
  return 0;
}

int esvio_fe_track_aedat(esvio_fe_handle c, const void* left, size_t left_bytes, const void* right, size_t right_bytes,
                         int64_t t_offset_ns, uint32_t flags, int pub_this_frame, const esvio_fe_filter_params* filter,
                         const esvio_fe_motion* motion, esvio_fe_tracks* out, esvio_fe_batch_info* info_out,
                         esvio_fe_aedat_info aedat[2]) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info_out) *info_out = esvio_fe_batch_info{};
  AedatJob job[2];
  job[0].bytes = left, job[0].n_bytes = left_bytes, job[1].bytes = right, job[1].n_bytes = right_bytes;
  for (int cam = 0; cam < 2; cam++) {
    if (aedat) aedat_info_clear(&aedat[cam]);
    if (int rc = aedat_args_check(c, cam ? "track_aedat (right)" : "track_aedat (left)", job[cam].bytes, job[cam].n_bytes, t_offset_ns, flags))
      return rc;
  }
  if (filter)
    if (int rc = baf_prm_check(c, filter, "track_aedat")) return rc;
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "track_aedat: batches are announced on this handle (decode into memory of your own)");
  if (!left_bytes && !right_bytes) return 0;  // nothing to decode: no left event, nothing tracked
  for (int cam = 0; cam < 2; cam++) {
    if (int rc = aedat_count_walk(c, cam ? "track_aedat (right)" : "track_aedat (left)", cam, &job[cam])) return rc;
    if (aedat) aedat_info_packets(&aedat[cam], job[cam].cnt);
  }
  HIPCHK(c, hipSetDevice(c->dev));
  auto place = [&](const size_t want[2], DecodedCam dc[2]) { return track_place(c, filter != nullptr, want, dc); };
  const int cam_of[2] = {0, 1};
  AedatResult r[2] = {};
  DecodedCam dc[2];
  if (int rc = aedat_run(c, t_offset_ns, flags, job, cam_of, place, r, dc)) return rc;
  for (int cam = 0; cam < 2; cam++)
    if (aedat && job[cam].n_bytes) aedat_info_fill(&aedat[cam], r[cam]);
  return track_decoded(c, "track_aedat", "states", dc, filter, motion, pub_this_frame, out, info_out, [&] {
    for (int cam = 0; cam < 2; cam++)
      if (job[cam].n_bytes) c->aedat.ev_st[cam] = job[cam].st;
  });
}

// the walk tap (include/esvio_fe_test.h): the host walk alone, no handle, no device
int esvio_fe_aedat_walk_tap(void* state, size_t state_bytes, const void* bytes, size_t n_bytes, uint32_t* runs, size_t runs_cap,
                            uint8_t* payload, size_t events_cap, uint64_t counts[4]) {
  if (!state || state_bytes != sizeof(ae::Walk) || (n_bytes && !bytes) || !counts) return ESVIO_FE_EINVAL;
  ae::Walk st;
  memcpy(&st, state, sizeof st);
  ae::Out o;
  o.runs = (ae::Run*)runs, o.runs_cap = runs ? runs_cap : 0, o.payload = payload, o.events_cap = payload ? events_cap : 0;
  const bool ok = ae::walk(&st, ae::kEvents, (const uint8_t*)bytes, n_bytes, 0, 0, &o);
  counts[0] = o.n_events, counts[1] = o.n_runs, counts[2] = o.polarity_packets, counts[3] = o.other_packets;
  if (!ok) return ESVIO_FE_EINVAL;  // (the caller's state is as it was)
  memcpy(state, &st, sizeof st);
  return 0;
}
int esvio_fe_aedat_walk_state_bytes(void) { return (int)sizeof(ae::Walk); }

// ---- rosbag v2.0 recordings (the rule: include/esvio_fe.h; the host walk: fe_bag.h; the kernel: fe_kernels.h)
namespace {
namespace bg = esvio::bag;
static_assert(bg::kEventBytes == kBagEventBytes, "the walk's wire event is the kernel's");
struct BagCall {  // one call's walk and device work
  bg::Walk st{};   // the state behind the chunk: taken over when the call succeeds
  bg::Out cnt;     // what the counting walk found
  BagResult r[2] = {};
};

int bag_args_check(esvio_fe_ctx* c, const char* who, const void* bytes, size_t n_bytes, uint32_t flags) {
  if (flags) return fail(c, ESVIO_FE_EINVAL, "%s: unknown bits in flags (0x%x)", who, flags);
  if (n_bytes > kRawMaxBytes) return fail(c, ESVIO_FE_EINVAL, "%s: a chunk holds at most 2^28 bytes", who);
  if (n_bytes && !bytes) return fail(c, ESVIO_FE_EINVAL, "%s: bytes is null", who);
  return 0;
}
// the counting walk: everything in the chunk checked, the events and messages counted, nothing stored, no state moved
int bag_count_walk(esvio_fe_ctx* c, const char* who, const void* bytes, size_t n_bytes, BagCall* b) {
  bg::Walk probe = c->bag.ev_st;
  if (!bg::walk(&probe, c->bag.topics, bg::kEvents, (const uint8_t*)bytes, n_bytes, &b->cnt))
    return fail(c, ESVIO_FE_EINVAL, "%s: malformed bag (%s); the walker's state is as it was", who, b->cnt.why);
  return 0;
}
size_t bag_right_offset(size_t n_left) { return (n_left * kBagEventBytes + 15) & ~(size_t)15; }
uint32_t bag_tiles(size_t n) { return (uint32_t)((n + kBagTile - 1) / kBagTile); }
int bag_ensure(esvio_fe_ctx* c, size_t n_left, size_t n_right) {
  esvio_fe_ctx::Bag& B = c->bag;
  B.used = true;
  if (!B.res)
    if (int rc = B.res.alloc(c, 2)) return rc;
  const size_t bytes = bag_right_offset(n_left) + bag_right_offset(n_right);  // (each camera's part readable up to a multiple of 16)
  if (int rc = B.h_pack.grow(c, bytes)) return rc;
  return B.d_pack.grow(c, bytes);
}
// esvio_fe_reserve for a handle that decodes bags: the scratch of a chunk of max_left and max_right events
int bag_reserve(esvio_fe_ctx* c, const size_t events[2]) { return c->bag.used ? bag_ensure(c, events[0], events[1]) : 0; }
void bag_state_reset(esvio_fe_ctx* c) { c->bag.ev_st = c->bag.side_st = bg::Walk{}; }  // the event and the side walker
// The gathering walk, the copy, the launch and the copies that bring the result blocks to the host, on the current
// stream; nothing is waited for.  dc[cam].d, cap: where the camera's records go.  A camera without an event in the chunk
// takes no part on the device.
int bag_enqueue(esvio_fe_ctx* c, const void* bytes, size_t n_bytes, BagCall* b, const DecodedCam dc[2], esvio_fe_bag_message* msgs, size_t msgs_cap) {
  esvio_fe_ctx::Bag& B = c->bag;
  hipStream_t s = cur_stream(c);
  const size_t n[2] = {(size_t)b->cnt.n_events[0], (size_t)b->cnt.n_events[1]}, off1 = bag_right_offset(n[0]);
  if (n[0] + n[1])
    if (int rc = bag_ensure(c, n[0], n[1])) return rc;
  bg::Out o;
  if (n[0] + n[1]) o.payload[0] = B.h_pack, o.payload[1] = B.h_pack + off1, o.events_cap[0] = n[0], o.events_cap[1] = n[1];
  o.msgs = msgs, o.msgs_cap = msgs ? msgs_cap : 0;
  b->st = B.ev_st;
  bg::walk(&b->st, B.topics, bg::kEvents, (const uint8_t*)bytes, n_bytes, &o);  // (checked by the counting walk)
  if (!(n[0] + n[1])) return 0;
  HIPCHK(c, hipMemcpyAsync(B.d_pack, B.h_pack, off1 + n[1] * kBagEventBytes, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(B.res, 0, 2 * sizeof(BagResult), s));
  BagArgs a{};
  uint64_t stored = 0;
  for (int cam = 0; cam < 2; cam++) {
    BagCam& bc = a.cam[cam];
    bc.src = B.d_pack.p + (cam ? off1 : 0), bc.n = (uint32_t)n[cam], bc.tiles = bag_tiles(n[cam]);
    bc.dst = dc[cam].d, bc.dst_cap = (uint32_t)std::min<size_t>(dc[cam].cap, 0xffffffffu), bc.res = B.res + cam;
    if (n[cam] <= dc[cam].cap) stored += n[cam];
  }
  {
    ScopedKernel k(c, K_BAG_EMIT, (n[0] + n[1]) * kBagEventBytes + stored * 16);
    launch_bag_emit(s, a);
  }
  for (int cam = 0; cam < 2; cam++)
    if (n[cam]) HIPCHK(c, hipMemcpyAsync(&b->r[cam], B.res + cam, sizeof(BagResult), hipMemcpyDeviceToHost, s));
  return 0;
}
// The decode step of a chunk behind its counting walk: place(n, dc) says where each camera's n[cam] records go, the
// gathering walk and the launch run and are waited for.  b->r[cam], dc[cam]: the result block and the records; b->st:
// the walker behind the chunk, which the consumer takes over.
extern "C++" template <class Place>
int bag_run(esvio_fe_ctx* c, const void* bytes, size_t n_bytes, BagCall* b, esvio_fe_bag_message* msgs, size_t msgs_cap, Place place,
            DecodedCam dc[2]) {
  const size_t n[2] = {(size_t)b->cnt.n_events[0], (size_t)b->cnt.n_events[1]};
  if (int rc = place(n, dc)) return rc;
  if (int rc = bag_enqueue(c, bytes, n_bytes, b, dc, msgs, msgs_cap)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  for (int cam = 0; cam < 2; cam++)
    dc[cam].events = n[cam], dc[cam].bad = b->r[cam].bad, dc[cam].sec = b->r[cam].last_sec, dc[cam].nsec = b->r[cam].last_nsec;
  return 0;
}
void bag_info_clear(esvio_fe_bag_info* info) {
  if (!info) return;
  for (int cam = 0; cam < 2; cam++) info->cam[cam].events = info->cam[cam].bad = info->cam[cam].messages = 0;
  info->other_messages = info->other_records = info->chunks = info->connections = 0;
}
void bag_info_host(esvio_fe_bag_info* info, const bg::Out& o) {
  if (!info) return;
  for (int cam = 0; cam < 2; cam++) info->cam[cam].events = o.n_events[cam], info->cam[cam].messages = o.n_cam_msgs[cam];
  info->other_messages = o.other_messages, info->other_records = o.other_records, info->chunks = o.chunks, info->connections = o.connections;
}
void bag_info_device(esvio_fe_bag_info* info, const BagCall& b) {
  if (!info) return;
  for (int cam = 0; cam < 2; cam++) {
    const BagResult& r = b.r[cam];
    info->cam[cam].bad = r.bad;
    if (b.cnt.n_events[cam] && !r.bad)
      info->cam[cam].first_sec = r.first_sec, info->cam[cam].first_nsec = r.first_nsec, info->cam[cam].last_sec = r.last_sec, info->cam[cam].last_nsec = r.last_nsec;
  }
}
}  // namespace

int esvio_fe_bag_tile_events(void) { return (int)kBagTile; }

int esvio_fe_bag_header(const void* bytes, size_t n, esvio_fe_bag_header_info* out) { return bg::file_header(bytes, n, out); }

int esvio_fe_bag_set_topics(esvio_fe_handle c, const esvio_fe_bag_topics* topics) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* why = nullptr;
  if (!bg::set_topics(topics, &c->bag.topics, &why)) return fail(c, ESVIO_FE_EINVAL, "bag_set_topics: %s", why);
  bag_state_reset(c);
  return 0;
}

int esvio_fe_decode_bag(esvio_fe_handle c, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_event* const dst[2],
                        const size_t dst_cap[2], int dst_space, esvio_fe_bag_message* msgs, size_t msgs_cap, esvio_fe_bag_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  bag_info_clear(info);
  if (int rc = bag_args_check(c, "decode_bag", bytes, n_bytes, flags)) return rc;
  const size_t room[2] = {dst && dst_cap ? dst_cap[0] : 0, dst && dst_cap ? dst_cap[1] : 0};
  void* d[2] = {room[0] ? dst[0] : nullptr, room[1] ? dst[1] : nullptr};  // (a dst without room is not looked at)
  for (int cam = 0; cam < 2; cam++)
    if (int rc = dst_check(c, "decode_bag", cam ? "dst[1]" : "dst[0]", d[cam], room[cam], dst_space)) return rc;
  if (msgs_cap && !msgs) return fail(c, ESVIO_FE_EINVAL, "decode_bag: msgs is null");
  if (!n_bytes) return 0;
  BagCall b;
  if (int rc = bag_count_walk(c, "decode_bag", bytes, n_bytes, &b)) return rc;
  bag_info_host(info, b.cnt);
  HIPCHK(c, hipSetDevice(c->dev));
  auto place = [&](const size_t n[2], DecodedCam dc[2]) -> int {
    for (int cam = 0; cam < 2; cam++) {
      const size_t fit = std::min(room[cam], n[cam]);
      dc[cam].d = (EventRec*)d[cam];
      if (dst_space == ESVIO_FE_HOST && fit)  // the records behind a host dst: as many as it has room for
        if (int rc = dec_scratch(c, cam, fit, &dc[cam])) return rc;
      dc[cam].cap = fit;
    }
    return 0;
  };
  DecodedCam dc[2];
  if (int rc = bag_run(c, bytes, n_bytes, &b, msgs, msgs_cap, place, dc)) return rc;
  bag_info_device(info, b);
  if (dc[0].bad || dc[1].bad)
    return fail(c, ESVIO_FE_EINVAL, "decode_bag: %llu of %zu events have nsec >= 10^9; the walker's state is as it was", dc[0].bad + dc[1].bad,
                dc[0].events + dc[1].events);
  if (dc[0].events > room[0] || dc[1].events > room[1])
    return fail(c, ESVIO_FE_EINVAL, "decode_bag: the chunk holds %zu left and %zu right events, dst has room for %zu and %zu; the walker's state is as it was",
                dc[0].events, dc[1].events, room[0], room[1]);
  if (b.cnt.n_msgs > msgs_cap)
    return fail(c, ESVIO_FE_EINVAL, "decode_bag: the chunk completes %llu event messages, msgs has room for %zu; the walker's state is as it was",
                (unsigned long long)b.cnt.n_msgs, msgs_cap);
  if (dst_space == ESVIO_FE_HOST)
    if (int rc = deliver_host(c, 2, d, dc)) return rc;
  c->bag.ev_st = b.st;
  return 0;
}

int esvio_fe_bag_side(esvio_fe_handle c, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_imu_sample* imu, size_t imu_cap,
                      esvio_fe_bag_side_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info) *info = esvio_fe_bag_side_info{};
  if (int rc = bag_args_check(c, "bag_side", bytes, n_bytes, flags)) return rc;
  if (imu_cap && !imu) return fail(c, ESVIO_FE_EINVAL, "bag_side: imu is null");
  if (!n_bytes) return 0;
  bg::Walk st = c->bag.side_st;
  bg::Out o;
  o.imu = imu, o.imu_cap = imu_cap;
  if (!bg::walk(&st, c->bag.topics, bg::kSide, (const uint8_t*)bytes, n_bytes, &o))
    return fail(c, ESVIO_FE_EINVAL, "bag_side: malformed bag (%s); the walker's state is as it was", o.why);
  if (info) {
    info->imu = o.n_imu, info->bad = o.bad;
    info->other_messages = o.other_messages, info->other_records = o.other_records, info->chunks = o.chunks, info->connections = o.connections;
  }
  if (o.bad)
    return fail(c, ESVIO_FE_EINVAL, "bag_side: %llu samples have a stamp with nsec >= 10^9; the walker's state is as it was", (unsigned long long)o.bad);
  if (o.n_imu > imu_cap)
    return fail(c, ESVIO_FE_EINVAL, "bag_side: the chunk holds %llu samples, there is room for %zu; the walker's state is as it was",
                (unsigned long long)o.n_imu, imu_cap);
  c->bag.side_st = st;
  return 0;
}

// the walk tap (include/esvio_fe_test.h): the host walk alone, no handle, no device
int esvio_fe_bag_walk_tap(void* state, size_t state_bytes, const esvio_fe_bag_topics* topics, int side, const void* bytes, size_t n_bytes,
                          uint8_t* const payload[2], const size_t events_cap[2], esvio_fe_bag_message* msgs, size_t msgs_cap,
                          esvio_fe_imu_sample* imu, size_t imu_cap, uint64_t counts[12], char* why, size_t why_cap) {
  if (why && why_cap) why[0] = 0;
  if (!state || state_bytes != sizeof(bg::Walk) || (n_bytes && !bytes) || !counts) return ESVIO_FE_EINVAL;
  bg::Topics t;
  const char* bad_topics = nullptr;
  if (!bg::set_topics(topics, &t, &bad_topics)) return ESVIO_FE_EINVAL;
  bg::Walk st;
  memcpy(&st, state, sizeof st);
  bg::Out o;
  if (payload && events_cap)
    for (int cam = 0; cam < 2; cam++) o.payload[cam] = payload[cam], o.events_cap[cam] = payload[cam] ? events_cap[cam] : 0;
  o.msgs = msgs, o.msgs_cap = msgs ? msgs_cap : 0, o.imu = imu, o.imu_cap = imu ? imu_cap : 0;
  const bool ok = bg::walk(&st, t, side ? bg::kSide : bg::kEvents, (const uint8_t*)bytes, n_bytes, &o);
  const uint64_t v[12] = {o.n_events[0], o.n_events[1], o.n_cam_msgs[0], o.n_cam_msgs[1], o.n_msgs, o.n_imu,
                          o.bad, o.other_messages, o.other_records, o.chunks, o.connections, 0};
  memcpy(counts, v, sizeof v);
  if (!ok) {  // (the caller's state is as it was)
    if (why && why_cap) snprintf(why, why_cap, "%s", o.why);
    return ESVIO_FE_EINVAL;
  }
  memcpy(state, &st, sizeof st);
  return 0;
}
int esvio_fe_bag_walk_state_bytes(void) { return (int)sizeof(bg::Walk); }

// (the rosbag image stage and the AEDAT frame stage stand at the end of the file)
namespace {
int bag_image_reserve(esvio_fe_ctx* c);
int aedat_frame_reserve(esvio_fe_ctx* c);
void bag_image_state_reset(esvio_fe_ctx* c);
void decode_state_reset(esvio_fe_ctx* c) { raw_state_reset(c), aedat_state_reset(c), bag_state_reset(c), bag_image_state_reset(c), text_state_reset(c); }
}  // namespace

int esvio_fe_decode_reset(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  decode_state_reset(c);
  return 0;
}

// ---- stream slicing: a record stream cut into fixed-rate windows (the rule: include/esvio_fe.h; the chain: fe_kernels.h)
namespace {
using SliceState = esvio_fe_ctx::Slice::State;
using SliceBound = esvio_fe_ctx::Slice::Bound;
constexpr size_t kSliceMaxEvents = (size_t)1 << 30;
constexpr size_t kSliceTable = 4 * (kSliceMaxWindows + 1);  // boundaries the table holds: a call needs kSliceMaxWindows + 1 of them
constexpr uint32_t kSliceInlineCuts = 60;                   // cut entries that arrive with the result block (one 256-byte copy)

inline double slice_to_sec(uint64_t sec, uint32_t nsec) { return (double)sec + 1e-9 * (double)nsec; }
// ros::Time::fromSec, restated (include/esvio_fe.h)
inline SliceBound slice_time(double d) {
  const double fl = std::floor(d);
  uint64_t sec = (uint64_t)fl;
  uint64_t nsec = (uint64_t)std::round((d - fl) * 1e9);
  if (nsec >= 1000000000ull) sec += 1, nsec -= 1000000000ull;
  return SliceBound{sec, (uint32_t)nsec};
}
inline bool slice_same_chain(const SliceState& a, const SliceState& b) {
  return a.seen && b.seen && a.frequency == b.frequency && a.o_sec == b.o_sec && a.o_nsec == b.o_nsec;
}

// The camera's table covers E_m .. E_{m + kSliceMaxWindows} of st's chain (or ends in front of that with a boundary that
// leaves 32 bits); *n_bounds: the entries from E_m on a call may search.  Recomputed — from E_0 for a new chain, else
// from the entry for m, which the table always holds — and sent to the device when it does not.
int slice_table(esvio_fe_ctx* c, int cam, const SliceState& st, uint32_t* n_bounds, hipStream_t s) {
  esvio_fe_ctx::Slice& sl = c->slice;
  std::vector<SliceBound>& E = sl.E[cam];
  const double period = 1.0 / st.frequency;
  const bool same = slice_same_chain(sl.tab_for[cam], st) && st.m >= sl.tb[cam] && st.m - sl.tb[cam] < E.size();
  auto covers = [&] {
    const size_t at = (size_t)(st.m - sl.tb[cam]);
    return E.size() - at > kSliceMaxWindows || (E.back().sec >> 32) != 0;
  };
  if (!same || !covers()) {
    SliceBound e;
    if (same) {
      e = E[(size_t)(st.m - sl.tb[cam])];
    } else {  // (a fresh chain has closed nothing: m == 0)
      if (st.m != 0) return fail(c, ESVIO_FE_EINTERNAL, "slice: the boundary table does not belong to the camera's state");
      e = slice_time(slice_to_sec(st.o_sec, st.o_nsec) + period);
    }
    E.clear();
    E.push_back(e);
    while (E.size() < kSliceTable && (E.back().sec >> 32) == 0) E.push_back(slice_time(slice_to_sec(E.back().sec, E.back().nsec) + period));
    sl.tb[cam] = st.m;
    sl.tab_for[cam] = st;
    if (!sl.bounds[cam])
      if (int rc = sl.bounds[cam].alloc(c, kSliceTable)) return rc;
    if (!sl.h_bounds[cam])
      if (int rc = sl.h_bounds[cam].alloc(c, kSliceTable)) return rc;
    for (size_t k = 0; k < E.size(); k++) sl.h_bounds[cam][k] = slice_to_sec(E[k].sec, E[k].nsec);
    HIPCHK(c, hipMemcpyAsync(sl.bounds[cam], sl.h_bounds[cam], E.size() * sizeof(double), hipMemcpyHostToDevice, s));
  }
  *n_bounds = (uint32_t)std::min<size_t>(E.size() - (size_t)(st.m - sl.tb[cam]), kSliceMaxWindows + 1);
  return 0;
}
SliceBound slice_bound(const esvio_fe_ctx* c, int cam, uint64_t k) { return c->slice.E[cam][(size_t)(k - c->slice.tb[cam])]; }

void slice_info_state(esvio_fe_slice_info* info, const SliceState& st) {
  if (!info) return;
  info->closed = 0, info->first_window = info->count = st.m, info->open_events = st.open;
}
int slice_cam_check(esvio_fe_ctx* c, const char* who, int cam) {
  return cam == 0 || cam == 1 ? 0 : fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
}
}  // namespace

int esvio_fe_slice_tile_events(void) { return (int)kSliceTile; }

namespace {
int slice_feed_check(esvio_fe_ctx* c, const char* who) {  // an open feed keeps its windows in the cameras' slicer states
  return c->feed.open ? fail(c, ESVIO_FE_EINVAL, "%s: a feed is open on this handle and owns the slicer (esvio_fe_feed_close first)", who) : 0;
}
int slice_events_impl(esvio_fe_ctx* c, int cam, const esvio_fe_event* ev, size_t n, int space, const esvio_fe_slice_params* prm,
                      uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info);
int slice_events_at_impl(esvio_fe_ctx* c, int cam, const esvio_fe_event* ev, size_t n, int space, const esvio_fe_event* bounds,
                         size_t n_bounds, uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info);
}  // namespace

int esvio_fe_slice_events(esvio_fe_handle c, int cam, const esvio_fe_event* ev, size_t n, int space,
                          const esvio_fe_slice_params* prm, uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = slice_feed_check(c, "slice_events")) return rc;
  return slice_events_impl(c, cam, ev, n, space, prm, cuts, cuts_cap, info);
}

int esvio_fe_slice_events_at(esvio_fe_handle c, int cam, const esvio_fe_event* ev, size_t n, int space,
                             const esvio_fe_event* bounds, size_t n_bounds, uint64_t* cuts, size_t cuts_cap,
                             esvio_fe_slice_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = slice_feed_check(c, "slice_events_at")) return rc;
  return slice_events_at_impl(c, cam, ev, n, space, bounds, n_bounds, cuts, cuts_cap, info);
}

namespace {
// Windows at given stamps (include/esvio_fe.h): the fixed-rate call's three launches over a table of the caller's
// stamps.  The kernels read c == n_bounds as "at or beyond the range's last boundary" and fail the call; here an event
// behind the last given boundary is no failure, so the table ends in one more entry that no stamp reaches (+inf: a
// record's stamp is finite) and a count never gets there.
int slice_events_at_impl(esvio_fe_ctx* c, int cam, const esvio_fe_event* ev, size_t n, int space, const esvio_fe_event* bounds,
                         size_t n_bounds, uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info) {
  if (int rc = slice_cam_check(c, "slice_events_at", cam)) return rc;
  esvio_fe_ctx::Slice& sl = c->slice;
  const SliceState& cur = sl.st[cam];
  slice_info_state(info, cur);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "slice_events_at: bad memory space");
  if (n_bounds > kSliceMaxWindows)
    return fail(c, ESVIO_FE_EINVAL, "slice_events_at: a call takes at most %u boundaries (got %zu)", kSliceMaxWindows, n_bounds);
  if (n_bounds && !bounds) return fail(c, ESVIO_FE_EINVAL, "slice_events_at: bounds is null");
  for (size_t k = 1; k < n_bounds; k++)
    if (slice_to_sec(bounds[k].sec, bounds[k].nsec) < slice_to_sec(bounds[k - 1].sec, bounds[k - 1].nsec))
      return fail(c, ESVIO_FE_EINVAL, "slice_events_at: boundary %zu lies in front of boundary %zu: the stamps must not decrease", k, k - 1);
  if (n && !ev) return fail(c, ESVIO_FE_EINVAL, "slice_events_at: ev is null");
  if (n > kSliceMaxEvents) return fail(c, ESVIO_FE_EINVAL, "slice_events_at: a call takes at most 2^30 events");
  if (space == ESVIO_FE_DEVICE && ((uintptr_t)ev & 15) != 0)
    return fail(c, ESVIO_FE_EINVAL, "slice_events_at: device events must be 16-byte aligned");
  if (cuts_cap && !cuts) return fail(c, ESVIO_FE_EINVAL, "slice_events_at: cuts is null");
  if (!n) return 0;
  if (cur.seen && !cur.at)
    return fail(c, ESVIO_FE_EINVAL, "slice_events_at: the camera's first call fixed fixed-rate windows (esvio_fe_slice_reset first)");
  HIPCHK(c, hipSetDevice(c->dev));
  hipStream_t s = cur_stream(c);
  SliceState st = cur;
  st.seen = true, st.at = true;
  // the table: the camera's own, which then belongs to no fixed-rate chain any more
  sl.tab_for[cam] = SliceState();
  sl.E[cam].clear();
  if (!sl.bounds[cam])
    if (int rc = sl.bounds[cam].alloc(c, kSliceTable)) return rc;
  if (!sl.h_bounds[cam])
    if (int rc = sl.h_bounds[cam].alloc(c, kSliceTable)) return rc;
  for (size_t k = 0; k < n_bounds; k++) sl.h_bounds[cam][k] = slice_to_sec(bounds[k].sec, bounds[k].nsec);
  sl.h_bounds[cam][n_bounds] = std::numeric_limits<double>::infinity();
  HIPCHK(c, hipMemcpyAsync(sl.bounds[cam], sl.h_bounds[cam], (n_bounds + 1) * sizeof(double), hipMemcpyHostToDevice, s));
  const uint32_t tiles = (uint32_t)((n + kSliceTile - 1) / kSliceTile);
  if (!sl.res)
    if (int rc = sl.res.alloc(c, 2 * kSliceResWords)) return rc;
  if (!sl.h_res)
    if (int rc = sl.h_res.alloc(c, 2 * kSliceResWords)) return rc;
  if (int rc = sl.tmax[cam].grow(c, tiles)) return rc;
  const EventRec* d_ev = (const EventRec*)ev;
  if (space == ESVIO_FE_HOST) {
    if (int rc = sl.src[cam].grow(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(sl.src[cam], ev, n * sizeof(EventRec), hipMemcpyHostToDevice, s));
    d_ev = sl.src[cam];
  }
  uint32_t* d_res = sl.res + (size_t)cam * kSliceResWords;
  uint32_t* h_res = sl.h_res + (size_t)cam * kSliceResWords;
  SliceArgs a{};
  SliceCam& sc = a.cam[0];
  sc.ev = d_ev, sc.n = (uint32_t)n, sc.tiles = tiles;
  sc.bounds = sl.bounds[cam], sc.n_bounds = (uint32_t)n_bounds + 1;
  sc.tmax = sl.tmax[cam], sc.res = (SliceResult*)d_res, sc.cuts = d_res + sizeof(SliceResult) / 4;
  {
    ScopedKernel k(c, K_SLICE_REDUCE, (uint64_t)n * sizeof(EventRec) + (uint64_t)tiles * 4);
    launch_slice_reduce(s, a);
  }
  {
    ScopedKernel k(c, K_SLICE_SCAN, (uint64_t)tiles * 8);
    launch_slice_scan(s, a);
  }
  {
    ScopedKernel k(c, K_SLICE_CUTS, (uint64_t)n * sizeof(EventRec) + (uint64_t)tiles * 4);
    launch_slice_cuts(s, a);
  }
  HIPCHK(c, hipMemcpyAsync(h_res, d_res, sizeof(SliceResult) + kSliceInlineCuts * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  const SliceResult r = *(const SliceResult*)h_res;
  if (r.overflow || r.closed > n_bounds)
    return fail(c, ESVIO_FE_EINTERNAL, "slice_events_at: a count reached the table's closing entry");
  if (r.closed > cuts_cap) {
    if (info) info->closed = r.closed;
    return fail(c, ESVIO_FE_EINVAL, "slice_events_at: the call closes %u windows, cuts has room for %zu; the camera's state is as it was", r.closed, cuts_cap);
  }
  if (r.closed > kSliceInlineCuts) {
    HIPCHK(c, hipMemcpyAsync(h_res + sizeof(SliceResult) / 4 + kSliceInlineCuts, d_res + sizeof(SliceResult) / 4 + kSliceInlineCuts,
                             (size_t)(r.closed - kSliceInlineCuts) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  for (uint32_t j = 0; j < r.closed; j++) cuts[j] = h_res[sizeof(SliceResult) / 4 + j];
  st.open = r.closed ? n - r.first_of_last : cur.open + n;
  st.m += r.closed;
  if (info) {
    info->closed = r.closed, info->first_window = cur.m, info->count = st.m, info->open_events = st.open;
    if (r.closed) {
      info->first_sec = bounds[0].sec, info->first_nsec = bounds[0].nsec;
      info->last_sec = bounds[r.closed - 1].sec, info->last_nsec = bounds[r.closed - 1].nsec;
    }
  }
  sl.st[cam] = st;
  return 0;
}

int slice_events_impl(esvio_fe_ctx* c, int cam, const esvio_fe_event* ev, size_t n, int space, const esvio_fe_slice_params* prm,
                      uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info) {
  if (int rc = slice_cam_check(c, "slice_events", cam)) return rc;
  esvio_fe_ctx::Slice& sl = c->slice;
  const SliceState& cur = sl.st[cam];
  slice_info_state(info, cur);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "slice_events: bad memory space");
  if (!prm) return fail(c, ESVIO_FE_EINVAL, "slice_events: prm is null");
  if (prm->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "slice_events: reserved must be 0");
  if (!(prm->frequency >= 1e-3 && prm->frequency <= 1e6))
    return fail(c, ESVIO_FE_EINVAL, "slice_events: frequency must be in [1e-3, 1e6] (got %g)", prm->frequency);
  if (n && !ev) return fail(c, ESVIO_FE_EINVAL, "slice_events: ev is null");
  if (n > kSliceMaxEvents) return fail(c, ESVIO_FE_EINVAL, "slice_events: a call takes at most 2^30 events");
  if (space == ESVIO_FE_DEVICE && ((uintptr_t)ev & 15) != 0)
    return fail(c, ESVIO_FE_EINVAL, "slice_events: device events must be 16-byte aligned");
  if (cuts_cap && !cuts) return fail(c, ESVIO_FE_EINVAL, "slice_events: cuts is null");
  if (!n) return 0;
  if (cur.seen && cur.at)
    return fail(c, ESVIO_FE_EINVAL, "slice_events: the camera's first call fixed windows at given stamps (esvio_fe_slice_reset first)");
  HIPCHK(c, hipSetDevice(c->dev));
  hipStream_t s = cur_stream(c);
  // the state this call works from: the camera's, or — for its first events — the one they and prm define
  SliceState st = cur;
  if (cur.seen) {
    const bool same = prm->frequency == cur.frequency && (prm->has_origin != 0) == (cur.has_origin != 0) &&
                      (!prm->has_origin || (prm->origin.sec == cur.o_sec && prm->origin.nsec == cur.o_nsec));
    if (!same)
      return fail(c, ESVIO_FE_EINVAL, "slice_events: frequency and origin are fixed by the camera's first call (esvio_fe_slice_reset first)");
  } else {
    esvio_fe_event first = prm->origin;
    if (!prm->has_origin) {
      if (space == ESVIO_FE_HOST) {
        first = ev[0];
      } else {
        HIPCHK(c, hipMemcpyAsync(&first, ev, sizeof(first), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
      }
    }
    st.seen = true, st.has_origin = prm->has_origin != 0, st.frequency = prm->frequency;
    st.o_sec = first.sec, st.o_nsec = first.nsec;
  }
  uint32_t n_bounds = 0;
  if (int rc = slice_table(c, cam, st, &n_bounds, s)) return rc;
  const uint32_t tiles = (uint32_t)((n + kSliceTile - 1) / kSliceTile);
  if (!sl.res)
    if (int rc = sl.res.alloc(c, 2 * kSliceResWords)) return rc;
  if (!sl.h_res)
    if (int rc = sl.h_res.alloc(c, 2 * kSliceResWords)) return rc;
  if (int rc = sl.tmax[cam].grow(c, tiles)) return rc;
  const EventRec* d_ev = (const EventRec*)ev;
  if (space == ESVIO_FE_HOST) {
    if (int rc = sl.src[cam].grow(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(sl.src[cam], ev, n * sizeof(EventRec), hipMemcpyHostToDevice, s));
    d_ev = sl.src[cam];
  }
  uint32_t* d_res = sl.res + (size_t)cam * kSliceResWords;
  uint32_t* h_res = sl.h_res + (size_t)cam * kSliceResWords;
  SliceArgs a{};
  SliceCam& sc = a.cam[0];
  sc.ev = d_ev, sc.n = (uint32_t)n, sc.tiles = tiles;
  sc.bounds = sl.bounds[cam] + (size_t)(st.m - sl.tb[cam]), sc.n_bounds = n_bounds;
  sc.tmax = sl.tmax[cam], sc.res = (SliceResult*)d_res, sc.cuts = d_res + sizeof(SliceResult) / 4;
  {
    ScopedKernel k(c, K_SLICE_REDUCE, (uint64_t)n * sizeof(EventRec) + (uint64_t)tiles * 4);
    launch_slice_reduce(s, a);
  }
  {
    ScopedKernel k(c, K_SLICE_SCAN, (uint64_t)tiles * 8);
    launch_slice_scan(s, a);
  }
  {
    ScopedKernel k(c, K_SLICE_CUTS, (uint64_t)n * sizeof(EventRec) + (uint64_t)tiles * 4);
    launch_slice_cuts(s, a);
  }
  HIPCHK(c, hipMemcpyAsync(h_res, d_res, sizeof(SliceResult) + kSliceInlineCuts * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (c->prof_on) resolve_profile(c);
  const SliceResult r = *(const SliceResult*)h_res;
  if (r.overflow) {
    const SliceBound last = slice_bound(c, cam, st.m + n_bounds - 1);
    if (last.sec >> 32)
      return fail(c, ESVIO_FE_EINVAL, "slice_events: an event lies at or beyond a boundary whose seconds leave 32 bits; the camera's state is as it was");
    return fail(c, ESVIO_FE_EINVAL, "slice_events: an event lies at or beyond E_%llu: a call closes at most %u windows; the camera's state is as it was",
                (unsigned long long)(st.m + n_bounds - 1), kSliceMaxWindows);
  }
  if (r.closed > cuts_cap) {
    if (info) info->closed = r.closed;
    return fail(c, ESVIO_FE_EINVAL, "slice_events: the call closes %u windows, cuts has room for %zu; the camera's state is as it was", r.closed, cuts_cap);
  }
  if (r.closed > kSliceInlineCuts) {
    HIPCHK(c, hipMemcpyAsync(h_res + sizeof(SliceResult) / 4 + kSliceInlineCuts, d_res + sizeof(SliceResult) / 4 + kSliceInlineCuts,
                             (size_t)(r.closed - kSliceInlineCuts) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  for (uint32_t j = 0; j < r.closed; j++) cuts[j] = h_res[sizeof(SliceResult) / 4 + j];
  // the call succeeded: the camera's state is what it computed
  st.open = r.closed ? n - r.first_of_last : cur.open + n;
  st.m += r.closed;
  if (info) {
    info->closed = r.closed, info->first_window = cur.m, info->count = st.m, info->open_events = st.open;
    if (r.closed) {
      const SliceBound f = slice_bound(c, cam, cur.m), l = slice_bound(c, cam, st.m - 1);
      info->first_sec = (uint32_t)f.sec, info->first_nsec = f.nsec, info->last_sec = (uint32_t)l.sec, info->last_nsec = l.nsec;
    }
  }
  sl.st[cam] = st;
  return 0;
}
}  // namespace

int esvio_fe_slice_flush(esvio_fe_handle c, int cam, esvio_fe_slice_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = slice_cam_check(c, "slice_flush", cam)) return rc;
  if (int rc = slice_feed_check(c, "slice_flush")) return rc;
  SliceState& st = c->slice.st[cam];
  slice_info_state(info, st);
  if (!st.seen) return 0;
  if (st.at) {  // windows at given stamps: the open window has no boundary, the stamp fields stay as they are
    st.m += 1, st.open = 0;
    if (info) info->closed = 1, info->count = st.m, info->open_events = 0;
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->dev));
  uint32_t n_bounds = 0;
  if (int rc = slice_table(c, cam, st, &n_bounds, cur_stream(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));  // (a refilled table leaves its pinned copy before the next call can rewrite it)
  const SliceBound e = slice_bound(c, cam, st.m);
  if (e.sec >> 32) return fail(c, ESVIO_FE_EINVAL, "slice_flush: the open window's boundary leaves 32 bits of seconds");
  st.m += 1, st.open = 0;
  if (info) {
    info->closed = 1, info->count = st.m, info->open_events = 0;
    info->first_sec = info->last_sec = (uint32_t)e.sec, info->first_nsec = info->last_nsec = e.nsec;
  }
  return 0;
}

int esvio_fe_slice_reset(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = slice_feed_check(c, "slice_reset")) return rc;
  c->slice.st[0] = c->slice.st[1] = SliceState();
  return 0;
}

// ---- the feed: chunks in, time-aligned windows tracked where they lie (include/esvio_fe.h)
namespace {
using FeedCam = esvio_fe_ctx::Feed::Cam;
constexpr size_t kFeedMinRecords = 4096;  // a camera's first buffer

// No records, no windows; the buffers stay.  The append position falls back to the front of the current buffer, where a
// returned track call may still be reading a window (include/esvio_fe.h: buffer lifetime): unless every stream is known
// to be idle, the next append waits for what that call left on the side streams first (feed_room).
void feed_empty(esvio_fe_ctx* c, bool streams_idle) {
  esvio_fe_ctx::Feed& f = c->feed;
  for (esvio_fe_ctx::Feed::Cam& fc : f.cam) {
    fc.pos0 = fc.len = fc.open_begin = 0;
    fc.win.clear();
    if (streams_idle) fc.read_rec[0] = fc.read_rec[1] = false;
    fc.rewound = fc.read_rec[fc.cur];
  }
  f.origin_known = f.prm.has_origin != 0;
}
int feed_gate(esvio_fe_ctx* c, const char* who) {
  if (!c->feed.open) return fail(c, ESVIO_FE_EINVAL, "%s: no feed is open on this handle (esvio_fe_feed_open)", who);
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "%s: batches are announced on this handle", who);
  return 0;
}
// Room for `need` more records behind the camera's records, *dst = the append position.  When they do not fit, the
// untracked tail moves to the front of the other buffer (grown first if it is too small: that frees it, which waits
// for the device) on the main stream, behind whatever the last track call that read that buffer left on the side streams.
// the main stream behind whatever the last track call that read camera buffer b left on the side streams
int feed_wait_readers(esvio_fe_ctx* c, FeedCam& fc, int b) {
  if (fc.read_rec[b]) {
    hipStream_t side[4] = {c->stream2, c->stream3, c->stream4, c->stream6};
    for (int k = 0; k < 4; k++)
      if (side[k]) HIPCHK(c, hipStreamWaitEvent(cur_stream(c), fc.read_ev[b][k], 0));
  }
  fc.read_rec[b] = false;
  return 0;
}
int feed_room(esvio_fe_ctx* c, int cam, size_t need, EventRec** dst) {
  FeedCam& fc = c->feed.cam[cam];
  if (!fc.buf[fc.cur])
    if (int rc = fc.buf[fc.cur].alloc(c, std::max(need + need / 4, kFeedMinRecords))) return rc;
  if (fc.len + need > fc.buf[fc.cur].cap) {
    const uint64_t keep_from = fc.win.empty() ? fc.open_begin : fc.win.front().begin;
    const size_t tail = (size_t)(fc.pos0 + fc.len - keep_from), want = tail + need;
    const int to = fc.cur ^ 1;
    hipStream_t s = cur_stream(c);
    if (want > fc.buf[to].cap) {
      if (int rc = fc.buf[to].alloc(c, std::max(want + want / 4, kFeedMinRecords))) return rc;
      fc.read_rec[to] = false;
    } else if (int rc = feed_wait_readers(c, fc, to)) {
      return rc;
    }
    fc.rewound = false;  // (the buffer left behind keeps its read_rec: coming back to it waits)
    if (tail)
      HIPCHK(c, hipMemcpyAsync(fc.buf[to], fc.buf[fc.cur] + (size_t)(keep_from - fc.pos0), tail * sizeof(EventRec), hipMemcpyDeviceToDevice, s));
    fc.cur = to, fc.pos0 = keep_from, fc.len = tail;
  }
  if (fc.rewound) {  // the first append behind a close / open: the front of this buffer may still be read
    if (int rc = feed_wait_readers(c, fc, fc.cur)) return rc;
    fc.rewound = false;
  }
  *dst = fc.buf[fc.cur] + (size_t)fc.len;
  return 0;
}
void feed_info_fill(esvio_fe_feed_info* info, const FeedCam& fc, uint64_t appended, uint64_t rejected, uint64_t bad, uint64_t closed) {
  if (!info) return;
  info->appended = appended, info->rejected = rejected, info->bad = bad, info->closed = closed, info->queued = fc.win.size();
}

enum FeedKind { FEED_EVENTS, FEED_FIELDS, FEED_RAW, FEED_AEDAT, FEED_TEXT };
struct FeedSrc {
  FeedKind kind;
  const esvio_fe_event* ev = nullptr;
  const esvio_fe_event_fields* fields = nullptr;
  size_t n = 0;  // events or fields
  int format = 0;
  const void* words = nullptr;
  size_t n_bytes = 0;
  int64_t t_offset_us = 0;  // FEED_AEDAT, FEED_TEXT: nanoseconds
  uint32_t flags = 0;       // FEED_AEDAT
  const esvio_fe_text_format* text = nullptr;  // FEED_TEXT
  int space = 0;
};

int feed_push(esvio_fe_ctx* c, const char* who, int cam, const FeedSrc& src, esvio_fe_feed_info* info) {
  if (info) *info = esvio_fe_feed_info{};
  if (int rc = slice_cam_check(c, who, cam)) return rc;
  if (int rc = feed_gate(c, who)) return rc;
  esvio_fe_ctx::Feed& f = c->feed;
  FeedCam& fc = f.cam[cam];
  feed_info_fill(info, fc, 0, 0, 0, 0);
  if (src.space != ESVIO_FE_HOST && src.space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (src.kind == FEED_EVENTS) {
    if (src.n && !src.ev) return fail(c, ESVIO_FE_EINVAL, "%s: ev is null", who);
    if (src.space == ESVIO_FE_DEVICE && ((uintptr_t)src.ev & 15) != 0) return fail(c, ESVIO_FE_EINVAL, "%s: device events must be 16-byte aligned", who);
  } else if (src.kind == FEED_FIELDS) {
    if (int rc = fields_check(c, src.fields, src.n, who)) return rc;
  } else if (src.kind == FEED_AEDAT) {
    if (int rc = aedat_args_check(c, who, src.words, src.n_bytes, src.t_offset_us, src.flags)) return rc;
  } else if (src.kind == FEED_TEXT) {
    if (int rc = text_args_check(c, who, src.text, src.words, src.n_bytes, src.space, src.t_offset_us)) return rc;
  } else if (int rc = raw_args_check(c, who, src.format, src.words, src.n_bytes, src.space, src.t_offset_us)) {
    return rc;
  }
  const bool byte_src = src.kind == FEED_RAW || src.kind == FEED_AEDAT || src.kind == FEED_TEXT;
  if (!byte_src && src.n >= (1ull << 30)) return fail(c, ESVIO_FE_EINVAL, "%s: chunk too large", who);
  if (src.kind == FEED_TEXT ? !text_active(c, cam, *src.text, src.n_bytes) : byte_src ? !src.n_bytes : !src.n) return 0;
  AedatJob ajob[2];
  if (src.kind == FEED_AEDAT) {  // (every header checked before any device work)
    ajob[0].bytes = src.words, ajob[0].n_bytes = src.n_bytes;
    if (int rc = aedat_count_walk(c, who, cam, &ajob[0])) return rc;
  }
  if (cam == 1 && !f.origin_known)
    return fail(c, ESVIO_FE_EINVAL, "%s: the origin is the first left record, and no left record has been appended yet", who);
  HIPCHK(c, hipSetDevice(c->dev));
  hipStream_t s = cur_stream(c);
  const esvio_fe_filter_params* flt = f.has_filter ? &f.filter : nullptr;
  EventRec* dst = nullptr;
  uint64_t n_new = 0, rejected = 0, bad = 0;
  // what the filter reads, when the records have to be made first (a byte source)
  const esvio_fe_event* flt_ev = src.ev;
  const esvio_fe_event_fields* flt_fields = src.fields;
  size_t flt_n = src.n;
  int flt_space = src.space;
  // a byte source: decoded into the feed's room, or, in front of the filter, into the decode scratch
  RawResult raw_res[2] = {};
  DecodedCam dc[2];
  auto put = [&](size_t want, DecodedCam* to) -> int {
    if (flt) return dec_scratch(c, cam, std::max<size_t>(want, 1), to);
    if (int rc = feed_room(c, cam, want, &dst)) return rc;
    to->d = dst, to->cap = fc.buf[fc.cur].cap - (size_t)fc.len;
    return 0;
  };
  const int cam_of[2] = {cam, cam};
  if (src.kind == FEED_RAW) {
    RawJob job[2];
    job[0].words = src.words, job[0].n_bytes = src.n_bytes;
    auto place = [&](const size_t want[2], bool, DecodedCam to[2]) { return put(want[0], &to[0]); };
    if (int rc = raw_run(c, src.format, src.space, src.t_offset_us, job, cam_of, false, SIZE_MAX, place, raw_res, dc)) return rc;
  }
  if (src.kind == FEED_AEDAT) {
    auto place = [&](const size_t want[2], DecodedCam to[2]) { return put(want[0], &to[0]); };
    AedatResult ar[2] = {};
    if (int rc = aedat_run(c, src.t_offset_us, src.flags, ajob, cam_of, place, ar, dc)) return rc;
  }
  TextJob tjob[2];
  if (src.kind == FEED_TEXT) {
    tjob[0].bytes = src.words, tjob[0].n_bytes = src.n_bytes, tjob[0].active = true;
    auto place = [&](const size_t want[2], DecodedCam to[2]) { return put(want[0], &to[0]); };
    TextResult tr[2] = {};
    if (int rc = text_run(c, *src.text, src.space, src.t_offset_us, tjob, cam_of, place, tr, dc)) return rc;
    if (int rc = text_malformed_check(c, who, *src.text, tr, 1, "nothing was appended, the camera's state is")) return rc;
  }
  if (byte_src) {
    if (dc[0].bad) {
      feed_info_fill(info, fc, 0, 0, dc[0].bad, 0);
      return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events have a stamp outside [0, 2^32 s); nothing was appended, the camera's %s is as it was",
                  who, dc[0].bad, dc[0].events, src.kind == FEED_RAW ? "decoder state" : "state");
    }
    n_new = dc[0].events;
    flt_ev = (const esvio_fe_event*)dc[0].d, flt_fields = nullptr, flt_n = dc[0].events, flt_space = ESVIO_FE_DEVICE;
  }
  if (flt) {
    n_new = 0;
    if (flt_n) {
      if (int rc = feed_room(c, cam, flt_n, &dst)) return rc;
      if (int rc = baf_ensure(c, flt_n, flt_ev && flt_space == ESVIO_FE_HOST, false, flt_fields != nullptr)) return rc;
      BafResult r{};
      if (int rc = baf_enqueue(c, cam, flt_ev, flt_fields, flt_n, flt_space, *flt, dst, who)) return rc;
      if (int rc = baf_fetch(c, cam, &r, nullptr, 0)) return rc;
      HIPCHK(c, hipStreamSynchronize(s));
      if (c->prof_on) resolve_profile(c);
      if (int rc = baf_result_check(c, r, who)) return rc;
      if (r.n_bad) {
        feed_info_fill(info, fc, 0, 0, r.n_bad, 0);
        return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events %s; nothing was appended, the camera's plane is as it was", who, r.n_bad, flt_n, kBadStampText);
      }
      n_new = r.n_kept, rejected = r.n_rejected;
    }
  } else if (src.kind == FEED_EVENTS) {
    if (int rc = feed_room(c, cam, src.n, &dst)) return rc;
    HIPCHK(c, hipMemcpyAsync(dst, src.ev, src.n * sizeof(EventRec), src.space == ESVIO_FE_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    n_new = src.n;
  } else if (src.kind == FEED_FIELDS) {
    if (int rc = feed_room(c, cam, src.n, &dst)) return rc;
    if (int rc = convert_begin(c)) return rc;
    if (int rc = convert_enqueue(c, *src.fields, src.n, src.space, dst, 0)) return rc;
    unsigned long long nb = 0;
    if (int rc = convert_end(c, &nb)) return rc;
    if (c->prof_on) resolve_profile(c);
    if (nb) {
      feed_info_fill(info, fc, 0, 0, nb, 0);
      return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events %s; nothing was appended", who, nb, src.n, kBadStampText);
    }
    n_new = src.n;
  }
  // the slicer over the appended records; the windows it closes are queued
  esvio_fe_slice_info si{};
  uint64_t first_window = c->slice.st[cam].m;
  if (n_new) {
    esvio_fe_slice_params prm = f.prm;
    if (cam == 1 && !prm.has_origin) {  // the first left record's stamp, as the left camera's slicer took it
      prm.has_origin = 1;
      prm.origin = esvio_fe_event{};
      prm.origin.sec = c->slice.st[0].o_sec, prm.origin.nsec = c->slice.st[0].o_nsec;
    }
    f.cuts.resize(kSliceMaxWindows);
    if (int rc = slice_events_impl(c, cam, (const esvio_fe_event*)dst, (size_t)n_new, ESVIO_FE_DEVICE, &prm, f.cuts.data(), f.cuts.size(), &si))
      return rc;  // (nothing was appended: len has not moved; the decoder's state is not taken over)
    first_window = si.first_window;
  }
  if (src.kind == FEED_RAW) raw_commit(c, cam, raw_res[0]);
  if (src.kind == FEED_AEDAT) c->aedat.ev_st[cam] = ajob[0].st;
  if (src.kind == FEED_TEXT) c->text.st[cam] = tjob[0].st;
  const uint64_t at = fc.pos0 + fc.len;
  for (uint64_t j = 0; j < si.closed; j++) {
    const SliceBound e = slice_bound(c, cam, first_window + j);
    fc.win.push_back(esvio_fe_ctx::Feed::Window{first_window + j, fc.open_begin, at + f.cuts[(size_t)j], (uint32_t)e.sec, e.nsec});
    fc.open_begin = at + f.cuts[(size_t)j];
  }
  fc.len += n_new;
  if (cam == 0 && n_new) f.origin_known = true;
  feed_info_fill(info, fc, n_new, rejected, bad, si.closed);
  return 0;
}
}  // namespace

int esvio_fe_feed_open(esvio_fe_handle c, const esvio_fe_slice_params* prm, const esvio_fe_filter_params* filter) {
  if (!c) return ESVIO_FE_EINVAL;
  if (c->feed.open) return fail(c, ESVIO_FE_EINVAL, "feed_open: a feed is open on this handle (esvio_fe_feed_close first)");
  if (!prm) return fail(c, ESVIO_FE_EINVAL, "feed_open: prm is null");
  if (prm->reserved != 0) return fail(c, ESVIO_FE_EINVAL, "feed_open: reserved must be 0");
  if (!(prm->frequency >= 1e-3 && prm->frequency <= 1e6))
    return fail(c, ESVIO_FE_EINVAL, "feed_open: frequency must be in [1e-3, 1e6] (got %g)", prm->frequency);
  if (filter)
    if (int rc = baf_prm_check(c, filter, "feed_open")) return rc;
  if (!c->announced.empty() || !c->inflight.empty()) return fail(c, ESVIO_FE_EINVAL, "feed_open: batches are announced on this handle");
  esvio_fe_ctx::Feed& f = c->feed;
  f.prm = *prm;
  f.prm.has_origin = prm->has_origin != 0;
  f.has_filter = filter != nullptr;
  if (filter) f.filter = *filter;
  c->slice.st[0] = c->slice.st[1] = SliceState();
  feed_empty(c, false);
  f.open = true;
  return 0;
}

int esvio_fe_feed_close(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  if (!c->feed.open) return fail(c, ESVIO_FE_EINVAL, "feed_close: no feed is open on this handle");
  c->feed.open = false;
  feed_empty(c, false);
  return 0;
}

int esvio_fe_feed_push_events(esvio_fe_handle c, int cam, const esvio_fe_event* ev, size_t n, int space, esvio_fe_feed_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  FeedSrc src{FEED_EVENTS};
  src.ev = ev, src.n = n, src.space = space;
  return feed_push(c, "feed_push_events", cam, src, info);
}
int esvio_fe_feed_push_fields(esvio_fe_handle c, int cam, const esvio_fe_event_fields* fields, size_t n, int space,
                              esvio_fe_feed_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  FeedSrc src{FEED_FIELDS};
  src.fields = fields, src.n = n, src.space = space;
  return feed_push(c, "feed_push_fields", cam, src, info);
}
int esvio_fe_feed_push_raw(esvio_fe_handle c, int cam, int format, const void* words, size_t n_bytes, int space,
                           int64_t t_offset_us, esvio_fe_feed_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  FeedSrc src{FEED_RAW};
  src.format = format, src.words = words, src.n_bytes = n_bytes, src.t_offset_us = t_offset_us, src.space = space;
  return feed_push(c, "feed_push_raw", cam, src, info);
}

int esvio_fe_feed_push_text(esvio_fe_handle c, int cam, const esvio_fe_text_format* fmt, const void* bytes, size_t n_bytes, int space,
                            int64_t t_offset_ns, esvio_fe_feed_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  FeedSrc src{FEED_TEXT};
  src.text = fmt, src.words = bytes, src.n_bytes = n_bytes, src.t_offset_us = t_offset_ns, src.space = space;
  return feed_push(c, "feed_push_text", cam, src, info);
}

int esvio_fe_feed_push_aedat(esvio_fe_handle c, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                             esvio_fe_feed_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  FeedSrc src{FEED_AEDAT};
  src.words = bytes, src.n_bytes = n_bytes, src.t_offset_us = t_offset_ns, src.flags = flags, src.space = ESVIO_FE_HOST;
  return feed_push(c, "feed_push_aedat", cam, src, info);
}

// Both cameras' events of a bag chunk into the feed: decoded into the decode stage's buffers, then appended left before
// right as device records.  The left camera's append is undone when the right camera's fails: nothing is appended to
// either, and the walker moves only when both are.
int esvio_fe_feed_push_bag(esvio_fe_handle c, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_feed_info info[2]) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "feed_push_bag";
  if (info) info[0] = info[1] = esvio_fe_feed_info{};
  if (int rc = feed_gate(c, who)) return rc;
  esvio_fe_ctx::Feed& f = c->feed;
  for (int cam = 0; cam < 2 && info; cam++) feed_info_fill(&info[cam], f.cam[cam], 0, 0, 0, 0);
  if (int rc = bag_args_check(c, who, bytes, n_bytes, flags)) return rc;
  if (!n_bytes) return 0;
  BagCall b;
  if (int rc = bag_count_walk(c, who, bytes, n_bytes, &b)) return rc;
  const size_t n[2] = {(size_t)b.cnt.n_events[0], (size_t)b.cnt.n_events[1]};
  if (n[1] && !n[0] && !f.origin_known)
    return fail(c, ESVIO_FE_EINVAL, "%s: the origin is the first left record; this chunk brings right events and no left one, and none has been appended yet "
                "(push a longer chunk, or open the feed with an origin); the walker's state is as it was", who);
  HIPCHK(c, hipSetDevice(c->dev));
  auto place = [&](const size_t want[2], DecodedCam dc[2]) -> int {  // the decode scratch: exactly the chunk's records
    for (int cam = 0; cam < 2; cam++) {
      if (!want[cam]) continue;
      if (int rc = dec_scratch(c, cam, want[cam], &dc[cam])) return rc;
      dc[cam].cap = want[cam];
    }
    return 0;
  };
  DecodedCam dc[2];
  if (int rc = bag_run(c, bytes, n_bytes, &b, nullptr, 0, place, dc)) return rc;
  if (dc[0].bad || dc[1].bad) {
    for (int cam = 0; cam < 2 && info; cam++) feed_info_fill(&info[cam], f.cam[cam], 0, 0, dc[cam].bad, 0);
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu of %zu events have nsec >= 10^9; nothing was appended, the walker's state is as it was", who,
                dc[0].bad + dc[1].bad, n[0] + n[1]);
  }
  // what the left camera's append moves, for the case that the right camera's fails
  FeedCam& fl = f.cam[0];
  const uint64_t end0 = fl.pos0 + fl.len, open0 = fl.open_begin;
  const size_t win0 = fl.win.size();
  const SliceState slice0 = c->slice.st[0];
  const bool origin0 = f.origin_known;
  for (int cam = 0; cam < 2; cam++) {
    FeedSrc src{FEED_EVENTS};
    src.ev = (const esvio_fe_event*)dc[cam].d, src.n = n[cam], src.space = ESVIO_FE_DEVICE;
    const int rc = feed_push(c, who, cam, src, info ? &info[cam] : nullptr);
    if (rc == 0) continue;
    if (cam == 1) {
      fl.len = end0 - fl.pos0, fl.open_begin = open0;
      while (fl.win.size() > win0) fl.win.pop_back();
      c->slice.st[0] = slice0, f.origin_known = origin0;
      if (info) feed_info_fill(&info[0], fl, 0, 0, 0, 0);
    }
    return rc;
  }
  c->bag.ev_st = b.st;
  return 0;
}

int esvio_fe_feed_peek(esvio_fe_handle c, esvio_fe_feed_window* out) {
  if (!c || !out) return ESVIO_FE_EINVAL;
  *out = esvio_fe_feed_window{};
  if (int rc = feed_gate(c, "feed_peek")) return rc;
  const FeedCam &l = c->feed.cam[0], &r = c->feed.cam[1];
  if (l.win.empty() || r.win.empty()) return 0;
  const esvio_fe_ctx::Feed::Window &wl = l.win.front(), &wr = r.win.front();
  out->ready = 1, out->index = wl.index, out->end_sec = wl.sec, out->end_nsec = wl.nsec;
  out->count[0] = wl.end - wl.begin, out->count[1] = wr.end - wr.begin;
  return 0;
}

int esvio_fe_feed_track(esvio_fe_handle c, int pub_this_frame, const esvio_fe_motion* motion, esvio_fe_tracks* out,
                        esvio_fe_batch_info* info_out) {
  if (!c) return ESVIO_FE_EINVAL;
  esvio_fe_batch_info info{};
  if (info_out) *info_out = info;
  if (int rc = feed_gate(c, "feed_track")) return rc;
  FeedCam* fc[2] = {&c->feed.cam[0], &c->feed.cam[1]};
  if (fc[0]->win.empty() || fc[1]->win.empty()) return fail(c, ESVIO_FE_EINVAL, "feed_track: no window is closed in both cameras (esvio_fe_feed_peek)");
  const esvio_fe_ctx::Feed::Window w[2] = {fc[0]->win.front(), fc[1]->win.front()};
  if (w[0].index != w[1].index) return fail(c, ESVIO_FE_EINTERNAL, "feed_track: the cameras' windows do not pair");
  const size_t n[2] = {(size_t)(w[0].end - w[0].begin), (size_t)(w[1].end - w[1].begin)};
  if (n[0] + n[1] >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "feed_track: window too large");
  fc[0]->win.pop_front(), fc[1]->win.pop_front();
  info.kept[0] = n[0], info.kept[1] = n[1];
  if (info_out) *info_out = info;
  if (!n[0]) return 0;  // node:150: an empty left message is not tracked
  HIPCHK(c, hipSetDevice(c->dev));
  const EventRec* d[2];
  for (int cam = 0; cam < 2; cam++) d[cam] = fc[cam]->buf[fc[cam]->cur] + (size_t)(w[cam].begin - fc[cam]->pos0);
  EventRec last{};
  HIPCHK(c, hipMemcpyAsync(&last, d[0] + (n[0] - 1), sizeof(EventRec), hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  info.cur_time = (double)last.sec + 1e-9 * (double)last.nsec;
  const int rc = track_event_impl(c, info.cur_time, (const esvio_fe_event*)d[0], n[0], (const esvio_fe_event*)(n[1] ? d[1] : nullptr), n[1],
                                  ESVIO_FE_DEVICE, pub_this_frame != 0, motion);
  // what this call left on the side streams reads the buffers the windows lie in
  hipStream_t side[4] = {c->stream2, c->stream3, c->stream4, c->stream6};
  for (int cam = 0; cam < 2; cam++)
    for (int k = 0; k < 4; k++)
      if (side[k]) {
        Event& e = fc[cam]->read_ev[fc[cam]->cur][k];
        if (!e) HIPCHK(c, e.create());
        HIPCHK(c, hipEventRecord(e, side[k]));
      }
  fc[0]->read_rec[fc[0]->cur] = fc[1]->read_rec[fc[1]->cur] = true;
  info.tracked = rc == 0;
  if (info_out) *info_out = info;
  if (rc) return rc;
  return fill_tracks(c, out);
}

// ---- image front-end
int esvio_fe_good_features_to_track(esvio_fe_handle c, const uint8_t* img, int max_corners,
                                    double quality, double min_distance, const uint8_t* mask,
                                    float* out_xy, int32_t* n_out, float* eig_out) {
  if (!c || !img || !n_out) return ESVIO_FE_EINVAL;
  *n_out = 0;
  if (max_corners <= 0 || max_corners > c->cfg.max_cnt)
    return fail(c, ESVIO_FE_EINVAL, "max_corners must be in 1..max_cnt");
  if (!(quality > 0) || min_distance < 1 || min_distance > kMaxDiscR)
    return fail(c, ESVIO_FE_EINVAL, "quality must be > 0, min_distance in [1, %d]", kMaxDiscR);
  if (!out_xy) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->inflight.empty()) return fail(c, ESVIO_FE_EINVAL, "a prefetched batch is pending");
  if (int rc = prep_tmp_pyr(c, 0, img, c->W, c->H, 0)) return rc;
  PyrDesc d = c->tmp_pyr[0].d;
  pyr_build(c, &d, 1);  // materialises the reflect-101 border the Sobel taps read
  const ResView& pin = c->pin[0];
  if (mask) {  // nonzero = allowed; the device bitmap holds the BLOCKED pixels
    host::BitMask bm;
    bm.reset(c->W, c->H);
    for (int y = 0; y < c->H; y++)
      for (int x = 0; x < c->W; x++)
        if (!mask[(size_t)y * c->W + x]) bm.bits[(size_t)y * bm.wpr + (x >> 5)] |= 1u << (x & 31);
    std::memcpy(pin.mask, bm.bits.data(), bm.bits.size() * 4);
    HIPCHK(c, hipMemcpyAsync(c->d_mask_bits, pin.mask, bm.bits.size() * 4, hipMemcpyHostToDevice,
                             cur_stream(c)));
  }
  if (int rc = gftt_run(c, d, max_corners, quality, min_distance, mask != nullptr, (float2*)c->zpin[0].news, 0,
                        c->zpin[0].counts))
    return rc;
  if (eig_out)
    HIPCHK(c, hipMemcpyAsync(eig_out, c->d_gftt_eig, (size_t)c->W * c->H * 4, hipMemcpyDeviceToHost,
                             cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (int rc = lookback_expired(c)) return rc;
  const int k = pin.counts[0];
  std::memcpy(out_xy, pin.news, (size_t)k * 8);
  *n_out = k;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// FAST on the time surface (or a caller's image): fast.h:22-47 of the reference's vendored library
int esvio_fe_fast_corners(esvio_fe_handle c, int cam, const uint8_t* img, int space, int arc, int barrier,
                          int nonmax, int16_t* out_xy, int32_t* out_score, int32_t capacity, int32_t* n_out,
                          int32_t* n_detected) {
  if (!c || !n_out) return ESVIO_FE_EINVAL;
  *n_out = 0;
  if (n_detected) *n_detected = 0;
  if (arc != 9 && arc != 10) return fail(c, ESVIO_FE_EINVAL, "fast_corners: arc must be 9 or 10 (got %d)", arc);
  if (barrier < 0 || barrier > 255) return fail(c, ESVIO_FE_EINVAL, "fast_corners: barrier must be in 0..255 (got %d)", barrier);
  if (nonmax != 0 && nonmax != 1) return fail(c, ESVIO_FE_EINVAL, "fast_corners: nonmax must be 0 or 1");
  if (arc == 9 && (nonmax || out_score))
    return fail(c, ESVIO_FE_EINVAL, "fast_corners: the reference scores FAST-10 only: arc 9 has neither non-max nor scores");
  if (capacity < 0 || (capacity > 0 && !out_xy)) return fail(c, ESVIO_FE_EINVAL, "fast_corners: capacity %d without out_xy", capacity);
  if (!img && cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "fast_corners: cam must be 0 or 1");
  if (img && space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "fast_corners: bad memory space");
  HIPCHK(c, hipSetDevice(c->dev));
  const uint8_t* src = img;
  int stride = c->W;
  if (!img) {  // the plane esvio_fe_get_time_surface copies out, read where it lies; the main stream is behind
               // whatever rendered it (a prefetched batch's images are waited for when its track call takes it up)
    const PyrDesc& d = raw_ts_desc(c, cam);
    src = px00(d);
    stride = d.stride[0];
  } else if (space == ESVIO_FE_HOST) {
    const size_t bytes = (size_t)c->W * c->H;
    if (!c->d_fast_img)
      if (int rc = c->d_fast_img.alloc(c, bytes)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_fast_img, img, bytes, hipMemcpyHostToDevice, cur_stream(c)));
    src = c->d_fast_img;
  }
  return fast_run(c, src, stride, arc, barrier, nonmax != 0, out_xy, out_score, capacity, n_out, n_detected);
}

// FAST as trackEvent's detector (include/esvio_fe.h)
int esvio_fe_set_detector(esvio_fe_handle c, int detector, int fast_barrier) {
  if (!c) return ESVIO_FE_EINVAL;
  if (detector != ESVIO_FE_DETECT_ARC && detector != ESVIO_FE_DETECT_FAST)
    return fail(c, ESVIO_FE_EINVAL, "set_detector: detector must be ESVIO_FE_DETECT_ARC or ESVIO_FE_DETECT_FAST (got %d)", detector);
  if (detector == ESVIO_FE_DETECT_FAST && (fast_barrier < 0 || fast_barrier > 255))
    return fail(c, ESVIO_FE_EINVAL, "set_detector: fast_barrier must be in 0..255 (got %d)", fast_barrier);
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "esvio_fe_set_detector while batches are announced");
  HIPCHK(c, hipSetDevice(c->dev));
  // (the launch thread reads the setting, and growing a candidate set frees it: nothing may be in flight)
  if (int rc = launcher_drain(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream3));
  HIPCHK(c, hipStreamSynchronize(c->stream4));
  if (c->stream6) HIPCHK(c, hipStreamSynchronize(c->stream6));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (detector == ESVIO_FE_DETECT_FAST) {
    if (int rc = ensure_fast_detector(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fast_barrier = fast_barrier;
  }
  c->detector = detector;
  return 0;
}

// ---- event images (the rule: include/esvio_fe.h "event images"; the kernels: fe_kernels.h; the update: evimg_update)
int esvio_fe_set_event_images(esvio_fe_handle c, int on) {
  if (!c) return ESVIO_FE_EINVAL;
  if (on != 0 && on != 1 && on != ESVIO_FE_EVENT_IMAGES_AHEAD)
    return fail(c, ESVIO_FE_EINVAL, "esvio_fe_set_event_images: the value must be 0, 1 or ESVIO_FE_EVENT_IMAGES_AHEAD (got %d)", on);
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "esvio_fe_set_event_images while batches are announced");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = launcher_drain(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream3));
  HIPCHK(c, hipStreamSynchronize(c->stream4));
  if (c->stream6) HIPCHK(c, hipStreamSynchronize(c->stream6));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  esvio_fe_ctx::Evimg& E = c->evimg;
  E.on = false;
  E.mode = 0;
  E.nsets = 0;
  E.cur = 0;
  E.fresh_cams = 0;
  for (esvio_fe_ctx::Evimg::Set& S : E.set) {
    S.wstream[0] = S.wstream[1] = nullptr;
    for (int cam = 0; cam < 2; cam++) {
      S.marks[cam].release();
      S.img[cam].release();
      S.written[cam] = Event();
    }
  }
  E.canvas.release();
  if (!on) return 0;
  // everything the feature needs, pixel-proportional: per set 2 x (4 + 3) bytes per pixel — one set, or one for the
  // frame being tracked and one per prefetch lane — and the getter's canvas, 6 more
  E.groups = (c->P + 3u) / 4u;
  const int nsets = on == ESVIO_FE_EVENT_IMAGES_AHEAD ? esvio_fe_ctx::Evimg::kSets : 1;
  for (int k = 0; k < nsets; k++)
    for (int cam = 0; cam < 2; cam++) {
      esvio_fe_ctx::Evimg::Set& S = E.set[k];
      if (int rc = S.marks[cam].alloc(c, (size_t)E.groups * 4)) return rc;
      if (int rc = S.img[cam].alloc(c, (size_t)E.groups * 3)) return rc;
      HIPCHK(c, S.written[cam].create());
      HIPCHK(c, hipMemsetAsync(S.marks[cam], 0, (size_t)E.groups * 16, c->stream));
      HIPCHK(c, hipMemsetAsync(S.img[cam], 0, (size_t)E.groups * 12, c->stream));
    }
  if (int rc = E.canvas.alloc(c, (size_t)c->P * 6)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  E.nsets = nsets;
  E.mode = on;
  E.on = true;
  return 0;
}

int esvio_fe_clear_event_images(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  if (!c->evimg.on) return fail(c, ESVIO_FE_EINVAL, "clear_event_images: esvio_fe_set_event_images is off");
  HIPCHK(c, hipSetDevice(c->dev));
  return evimg_zero(c);
}

// a getter's argument checks, then the wait for the last write to the cameras' images on whichever stream made it
static int evimg_get_ready(esvio_fe_ctx* c, const char* who, int cam0, int cam1, const uint8_t* dst, int space) {
  if (!c->evimg.on) return fail(c, ESVIO_FE_EINVAL, "%s: esvio_fe_set_event_images is off", who);
  if (cam0 < 0 || cam1 > 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1", who);
  if (!dst) return fail(c, ESVIO_FE_EINVAL, "%s: dst is null", who);
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d", who, space);
  HIPCHK(c, hipSetDevice(c->dev));
  // (the current set's writes alone: a batch prefetched since writes a set of its own)
  const esvio_fe_ctx::Evimg::Set& S = c->evimg.set[c->evimg.cur];
  for (int cam = cam0; cam <= cam1; cam++)
    if (S.wstream[cam]) HIPCHK(c, hipEventSynchronize(S.written[cam]));
  return 0;
}

int esvio_fe_get_event_image(esvio_fe_handle c, int cam, uint8_t* dst, int space) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = evimg_get_ready(c, "get_event_image", cam, cam, dst, space)) return rc;
  // one dense copy on the null stream (none of the handle's: they are non-blocking streams), waited for
  HIPCHK(c, hipMemcpyAsync(dst, c->evimg.set[c->evimg.cur].img[cam], (size_t)c->P * 3, space == ESVIO_FE_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, nullptr));
  HIPCHK(c, hipStreamSynchronize(nullptr));
  return 0;
}

int esvio_fe_get_event_canvas(esvio_fe_handle c, uint8_t* dst, int space) {
  if (!c) return ESVIO_FE_EINVAL;
  if (int rc = evimg_get_ready(c, "get_event_canvas", 0, 1, dst, space)) return rc;
  esvio_fe_ctx::Evimg& E = c->evimg;
  // composed at getter time: device memory takes it directly, host memory one dense copy of the scratch
  uint8_t* canvas = space == ESVIO_FE_DEVICE ? dst : E.canvas.p;
  const esvio_fe_ctx::Evimg::Set& S = E.set[E.cur];
  launch_evimg_canvas(nullptr, (const uint8_t*)S.img[0].p, (const uint8_t*)S.img[1].p, c->W, c->H, canvas);
  if (space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(dst, canvas, (size_t)c->P * 6, hipMemcpyDeviceToHost, nullptr));
  HIPCHK(c, hipStreamSynchronize(nullptr));
  HIPCHK(c, hipGetLastError());
  return 0;
}

int esvio_fe_event_image_kernel_stats(esvio_fe_handle c, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c || which < 0 || which > 1) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(c->stream4));
  if (c->stream6) HIPCHK(c, hipStreamSynchronize(c->stream6));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  const KStat& s = c->stats[K_EVIMG_MARK + which];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}

int esvio_fe_features_to_track_fast(esvio_fe_handle c, const uint8_t* img, int space, int barrier, int max_corners,
                                    const uint8_t* mask, float* out_xy, int32_t* out_score, int32_t* n_out,
                                    int32_t* n_candidates) {
  if (!c || !n_out) return ESVIO_FE_EINVAL;
  *n_out = 0;
  if (n_candidates) *n_candidates = 0;
  if (barrier < 0 || barrier > 255)
    return fail(c, ESVIO_FE_EINVAL, "features_to_track_fast: barrier must be in 0..255 (got %d)", barrier);
  if (img && space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE)
    return fail(c, ESVIO_FE_EINVAL, "features_to_track_fast: bad memory space");
  if (max_corners > c->cfg.max_cnt) return fail(c, ESVIO_FE_EINVAL, "max_corners > max_cnt");
  if (max_corners > 0 && !out_xy) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = ensure_fast_tap(c)) return rc;
  const uint8_t* src = img;
  int stride = c->W;
  if (!img) {  // (as esvio_fe_fast_corners: the main stream is behind whatever rendered the plane)
    const PyrDesc& d = raw_ts_desc(c, 0);
    src = px00(d);
    stride = d.stride[0];
  } else if (space == ESVIO_FE_HOST) {
    HIPCHK(c, hipMemcpyAsync(c->d_fast_tap_img, img, (size_t)c->W * c->H, hipMemcpyHostToDevice, cur_stream(c)));
    src = c->d_fast_tap_img;
  }
  const esvio_fe_ctx::FastCand& fc = c->fastc[kRightSlots];
  if (int rc = fast_cand_pass(c, src, stride, barrier, c->fast_tap, fc, n_candidates != nullptr)) return rc;
  const ResView& pin = c->pin[0];
  if (max_corners > 0) {
    host::BitMask bm;
    bm.reset(c->W, c->H);
    if (mask) bm.from_bytes(mask);
    std::memcpy(pin.mask, bm.bits.data(), bm.bits.size() * 4);
    HIPCHK(c, hipMemcpyAsync(c->d_mask_bits, pin.mask, bm.bits.size() * 4, hipMemcpyHostToDevice, cur_stream(c)));
    // the selection of esvio_fe_features_to_track over the tap's own set; out_idx: the sort keys, score in bits 8..15
    SelectArgs sa = make_select_args(c, 0, max_corners, c->d_ptsD, 0, c->d_sel_idx);
    sa.comp_xy = c->fast_tap.comp_xy;
    sa.comp_idx = c->fast_tap.comp_idx;
    sa.total = c->fast_tap.total;
    sa.init_bits = c->d_mask_bits;
    launch_select_args(c, sa);
    HIPCHK(c, hipMemcpyAsync(pin.counts, c->dres.counts, 8, hipMemcpyDeviceToHost, cur_stream(c)));
  }
  uint32_t n_cand = 0;
  if (n_candidates) HIPCHK(c, hipMemcpyAsync(&n_cand, fc.tot, 4, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (int rc = lookback_expired(c)) return rc;
  const int k = max_corners > 0 ? pin.counts[0] : 0;
  if (k > 0) {
    HIPCHK(c, hipMemcpy(out_xy, c->d_ptsD, (size_t)k * 8, hipMemcpyDeviceToHost));
    if (out_score) {
      HIPCHK(c, hipMemcpy(out_score, c->d_sel_idx, (size_t)k * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < k; i++) out_score[i] = (out_score[i] >> 8) & 255;
    }
  }
  *n_out = k;
  if (n_candidates) *n_candidates = (int32_t)n_cand;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// Test tap (include/esvio_fe_test.h): the handle's selection launch over a caller's candidate list.  Nothing of the
// kernels is doubled here: the list goes into the current candidate set, the arguments through make_select_args /
// launch_select_args like every other selection's.
int esvio_fe_select_candidates(esvio_fe_handle c, const uint32_t* xy, const int32_t* payload, int n, double disc,
                               int flags, const uint8_t* mask, const float* stamp_xy, int n_stamp, int max_corners,
                               int out_base, int variant, float* out_xy, int32_t* out_idx, int32_t counts[3],
                               int32_t* kernel_id) {
  if (!c || !out_xy || !out_idx || !counts || n < 0 || n_stamp < 0 || (n && (!xy || !payload)) || (n_stamp && !stamp_xy))
    return ESVIO_FE_EINVAL;
  const int M = c->cfg.max_cnt;
  if (flags & ~(ESVIO_FE_SELECT_EUCLID | ESVIO_FE_SELECT_TABLE))
    return fail(c, ESVIO_FE_EINVAL, "select_candidates: unknown flag bits %d", flags);
  if (variant < 0 || variant > 2) return fail(c, ESVIO_FE_EINVAL, "select_candidates: variant must be 0, 1 or 2 (got %d)", variant);
  if (max_corners < 0 || out_base < 0 || max_corners > M || out_base > M - max_corners)
    return fail(c, ESVIO_FE_EINVAL, "select_candidates: max_corners and out_base + max_corners must be in 0..max_cnt");
  if (n_stamp > M) return fail(c, ESVIO_FE_EINVAL, "select_candidates: n_stamp > max_cnt");
  const bool euclid = (flags & ESVIO_FE_SELECT_EUCLID) != 0;
  if (!(disc >= 1) || disc > kMaxDiscR || (!euclid && disc != (double)(int)disc))
    return fail(c, ESVIO_FE_EINVAL, "select_candidates: the disc must be an integer radius or a min_distance in [1, %d]", kMaxDiscR);
  // (the kernels index the bitmap with a candidate's position, and the short stamp with a point's, unchecked)
  for (int i = 0; i < n; i++)
    if ((int)(xy[i] & 0xffffu) >= c->W || (int)(xy[i] >> 16) >= c->H)
      return fail(c, ESVIO_FE_EINVAL, "select_candidates: candidate %d lies outside the sensor", i);
  for (int i = 0; i < n_stamp; i++) {
    const float px = stamp_xy[2 * i], py = stamp_xy[2 * i + 1];
    if (!(px >= -0.5f && px < (float)c->W && py >= -0.5f && py < (float)c->H) || std::lrintf(px) >= c->W || std::lrintf(py) >= c->H)
      return fail(c, ESVIO_FE_EINVAL, "select_candidates: stamp point %d does not round to a pixel of the sensor", i);
  }
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "select_candidates while batches are announced");
  if (c->pend_right.active)
    if (int rc = finalize_lazy(c)) return rc;
  if (variant == 2 && c->select_ok && !c->d_sel_bitmap)
    if (int rc = c->d_sel_bitmap.alloc(c, (size_t)c->H * ((c->W + 31) / 32) + 4)) return rc;
  const int set = c->cand_cur;
  if (int rc = ensure_cand_capacity(c, set, (size_t)std::max(n, 1))) return rc;
  const esvio_fe_ctx::CandSet& cs = c->cand[set];
  hipStream_t s = cur_stream(c);
  const uint32_t total = (uint32_t)n;
  if (n) {
    HIPCHK(c, hipMemcpyAsync(cs.comp_xy, xy, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(cs.comp_idx, payload, (size_t)n * 4, hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipMemcpyAsync(cs.total, &total, 4, hipMemcpyHostToDevice, s));
  // (the whole output goes up first and comes back whole: what the kernel leaves alone is the caller's own bytes)
  HIPCHK(c, hipMemcpyAsync(c->d_ptsD, out_xy, (size_t)M * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->d_sel_idx, out_idx, (size_t)M * 4, hipMemcpyHostToDevice, s));
  const ResView &pin = c->pin[0], &zpin = c->zpin[0];
  SelectArgs sa = make_select_args(c, set, max_corners, c->d_ptsD, out_base, c->d_sel_idx);
  if (euclid) {
    euclid_halfwidths(disc, sa.hw, &sa.radius);
  } else {
    const std::vector<int> hw = host::disc_halfwidths((int)disc);
    sa.radius = (int)disc;
    for (int i = 0; i <= kMaxDiscR; i++) sa.hw[i] = i < (int)hw.size() ? (int8_t)hw[i] : -1;
  }
  sa.disc_c = (flags & ESVIO_FE_SELECT_TABLE) ? -1 : disc_threshold(sa.hw, sa.radius);
  if (mask) {
    host::BitMask bm;
    bm.reset(c->W, c->H);
    bm.from_bytes(mask);
    std::memcpy(pin.mask, bm.bits.data(), bm.bits.size() * 4);
    HIPCHK(c, hipMemcpyAsync(c->d_mask_bits, pin.mask, bm.bits.size() * 4, hipMemcpyHostToDevice, s));
    sa.init_bits = c->d_mask_bits;
  }
  if (n_stamp) {
    std::memcpy(pin.news, stamp_xy, (size_t)n_stamp * 8);
    sa.stamp_pts = (const float2*)zpin.news;
    sa.n_stamp = n_stamp;
  }
  pin.counts[0] = pin.counts[1] = pin.counts[2] = -1;
  sa.host_counts = zpin.counts;
  if (variant == 1) sa.one_wave = 1;
  if (variant == 2) sa.gbitmap = c->d_sel_bitmap;
  const KernelId id = launch_select_args(c, sa);
  HIPCHK(c, hipMemcpyAsync(out_xy, c->d_ptsD, (size_t)M * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(out_idx, c->d_sel_idx, (size_t)M * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (int i = 0; i < 3; i++) counts[i] = pin.counts[i];
  if (kernel_id) *kernel_id = (int32_t)id;
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_track_image_space(esvio_fe_handle c, double cur_time, const uint8_t* img_left, const uint8_t* img_right, int space,
                               int pub_this_frame, esvio_fe_tracks* out) {
  if (!c || !img_left) return ESVIO_FE_EINVAL;
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "track_image_space: bad memory space");
  HIPCHK(c, hipSetDevice(c->dev));
  if (!c->announced.empty() || !c->inflight.empty())
    return fail(c, ESVIO_FE_EINVAL, "event batches are announced on this handle");
  if (int rc = track_image_impl(c, cur_time, img_left, img_right, pub_this_frame != 0, space)) return rc;
  return fill_tracks(c, out);
}

int esvio_fe_track_image(esvio_fe_handle c, double cur_time, const uint8_t* img_left,
                         const uint8_t* img_right, int pub_this_frame, esvio_fe_tracks* out) {
  return esvio_fe_track_image_space(c, cur_time, img_left, img_right, ESVIO_FE_HOST, pub_this_frame, out);
}

// The node's sensor_msgs/PointCloud packing (stereo_event_tracker_node.cpp:273-329) of the current
// result members, as a fixed-size block: left entries with track_cnt > 1, then right entries whose
// id is among them; rows (x_un, y_un, 1, id*2+cam as float32, u, v, vx, vy); padding rows id -1.
int esvio_fe_pack_track_records(esvio_fe_handle c, float* out, int32_t* n_rows) {
  if (!c || !out) return ESVIO_FE_EINVAL;
  if (c->pend_right.active) {  // (lazy mode, packing a frame that was not to be published)
    HIPCHK(c, hipSetDevice(c->dev));
    // (in this order: the previous published frame's new corners — which that frame's call may have left to "the next
    // call" while their stereo LK was running — extend the map this frame's right-camera velocities read)
    if (int rc = finalize_lazy(c)) return rc;
  }
  const int rows = 2 * std::max(c->cfg.max_cnt, 1);
  int k = 0;
  std::vector<int> left_ids;
  left_ids.reserve(c->ids.size());
  for (size_t j = 0; j < c->ids.size() && k < rows; j++)
    if (c->track_cnt[j] > 1) {
      float* r = out + (size_t)k++ * 8;
      r[0] = c->cur_un_pts[j].x;
      r[1] = c->cur_un_pts[j].y;
      r[2] = 1.f;
      r[3] = (float)(c->ids[j] * 2 + 0);
      r[4] = c->cur_pts[j].x;
      r[5] = c->cur_pts[j].y;
      r[6] = c->pts_velocity[j].x;
      r[7] = c->pts_velocity[j].y;
      left_ids.push_back(c->ids[j]);
    }
  std::sort(left_ids.begin(), left_ids.end());
  for (size_t j = 0; j < c->ids_right.size() && k < rows; j++)
    if (std::binary_search(left_ids.begin(), left_ids.end(), c->ids_right[j])) {
      float* r = out + (size_t)k++ * 8;
      r[0] = c->cur_un_right_pts[j].x;
      r[1] = c->cur_un_right_pts[j].y;
      r[2] = 1.f;
      r[3] = (float)(c->ids_right[j] * 2 + 1);
      r[4] = c->cur_right_pts[j].x;
      r[5] = c->cur_right_pts[j].y;
      r[6] = c->right_pts_velocity[j].x;
      r[7] = c->right_pts_velocity[j].y;
    }
  if (n_rows) *n_rows = k;
  for (; k < rows; k++) {
    float* r = out + (size_t)k * 8;
    for (int i = 0; i < 8; i++) r[i] = 0.f;
    r[3] = -1.f;
  }
  return 0;
}

// ---- RCCL hand-off (north-star: "a single RCCL all-gather over xGMI to merge tracked corners") ----
int esvio_fe_exchange_tracks(esvio_fe_handle c, void* nccl_comm, int world, float* gathered) {
  if (!c || !nccl_comm || world < 1 || !gathered) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  nccl_allgather_fn all_gather = rccl_all_gather();
  if (!all_gather) return fail(c, ESVIO_FE_ENOTIMPL, "librccl.so not found (dlopen): %s", dlerror());
  const size_t cnt = (size_t)2 * std::max(c->cfg.max_cnt, 1) * 8;
  // the send / receive areas are shared with the asynchronous exchange of the handle's own
  // communicator: whatever that one still has packed or in flight goes first and is waited for
  if (int rc = exchange_flush(c)) return rc;
  if (c->x_pending) HIPCHK(c, hipEventSynchronize(c->x_done));
  if (c->x_pending && (size_t)world * cnt > c->x_pin_recv.cap)
    c->x_pending = false;  // (its gathered block is dropped with the buffer that is about to grow)
  if (int rc = exchange_buffers(c, world)) return rc;
  if (int rc = esvio_fe_pack_track_records(c, c->x_pin, nullptr)) return rc;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->x_send, c->x_pin, cnt * 4, hipMemcpyHostToDevice, st));
  const int nrc = all_gather(c->x_send, c->x_recv, cnt, 7 /* ncclFloat32 */, nccl_comm, st);
  if (nrc != 0) return fail(c, ESVIO_FE_EHIP, "ncclAllGather failed: %d", nrc);
  HIPCHK(c, hipMemcpyAsync(gathered, c->x_recv, (size_t)world * cnt * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

int esvio_fe_comm_unique_id(uint8_t id[128]) {
  if (!id) return ESVIO_FE_EINVAL;
  nccl_get_id_fn get_id = rccl_sym<nccl_get_id_fn>("ncclGetUniqueId");
  if (!get_id) return ESVIO_FE_ENOTIMPL;
  NcclId u;
  if (get_id(&u) != 0) return ESVIO_FE_EHIP;
  std::memcpy(id, u.internal, 128);
  return 0;
}

int esvio_fe_comm_init(esvio_fe_handle c, const uint8_t id[128], int rank, int world) {
  if (!c || !id || world < 1 || rank < 0 || rank >= world) return ESVIO_FE_EINVAL;
  if (c->x_comm) return fail(c, ESVIO_FE_EINVAL, "the handle has a communicator already");
  HIPCHK(c, hipSetDevice(c->dev));
  nccl_init_rank_fn init_rank = rccl_sym<nccl_init_rank_fn>("ncclCommInitRank");
  if (!init_rank || !rccl_all_gather()) return fail(c, ESVIO_FE_ENOTIMPL, "librccl.so not found (dlopen)");
  NcclId u;
  std::memcpy(u.internal, id, 128);
  void* comm = nullptr;
  const int nrc = init_rank(&comm, world, u, rank);
  if (nrc != 0 || !comm) return fail(c, ESVIO_FE_EHIP, "ncclCommInitRank failed: %d", nrc);
  c->x_comm = comm;
  c->x_world = world;
  if (!c->x_done) {  // (the second of the two)
    if (!c->x_stream) HIPCHK(c, c->x_stream.create());
    HIPCHK(c, c->x_done.create());
  }
  return exchange_buffers(c, world);
}

}  // extern "C"
namespace esvio {
namespace fe {
int exchange_pack(esvio_fe_ctx* c) {
  // (the previous exchange has to be through with the pinned areas)
  if (c->x_pending) HIPCHK(c, hipEventSynchronize(c->x_done));
  c->x_pending = false;
  if (int rc = esvio_fe_pack_track_records(c, c->x_pin, nullptr)) return rc;
  c->x_deferred = true;
  return 0;
}
int exchange_flush(esvio_fe_ctx* c) {
  if (!c->x_deferred) return 0;
  c->x_deferred = false;
  const size_t cnt = (size_t)2 * std::max(c->cfg.max_cnt, 1) * 8;
  HIPCHK(c, hipMemcpyAsync(c->x_send, c->x_pin, cnt * 4, hipMemcpyHostToDevice, c->x_stream));
  const int nrc = rccl_all_gather()(c->x_send, c->x_recv, cnt, 7 /* ncclFloat32 */, c->x_comm, c->x_stream);
  if (nrc != 0) return fail(c, ESVIO_FE_EHIP, "ncclAllGather failed: %d", nrc);
  HIPCHK(c, hipMemcpyAsync(c->x_pin_recv, c->x_recv, (size_t)c->x_world * cnt * 4, hipMemcpyDeviceToHost,
                           c->x_stream));
  HIPCHK(c, hipEventRecord(c->x_done, c->x_stream));
  c->x_pending = true;
  return 0;
}
}  // namespace fe
}  // namespace esvio
extern "C" {

int esvio_fe_exchange_begin(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  if (!c->x_comm) return fail(c, ESVIO_FE_EINVAL, "esvio_fe_comm_init has not been called");
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = exchange_flush(c)) return rc;  // (an automatic one that is still waiting goes first)
  if (int rc = exchange_pack(c)) return rc;
  return exchange_flush(c);
}

int esvio_fe_set_auto_exchange(esvio_fe_handle c, int on) {
  if (!c) return ESVIO_FE_EINVAL;
  if (on && !c->x_comm) return fail(c, ESVIO_FE_EINVAL, "esvio_fe_comm_init has not been called");
  c->x_auto = on != 0;
  return 0;
}

int esvio_fe_exchange_end(esvio_fe_handle c, float* gathered) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = exchange_flush(c)) return rc;
  if (!c->x_pending) return fail(c, ESVIO_FE_EINVAL, "no exchange in flight");
  HIPCHK(c, hipEventSynchronize(c->x_done));
  c->x_pending = false;
  if (gathered)
    std::memcpy(gathered, c->x_pin_recv, (size_t)c->x_world * 2 * std::max(c->cfg.max_cnt, 1) * 8 * sizeof(float));
  return 0;
}

int esvio_fe_set_lazy_new_stereo(esvio_fe_handle c, int on) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = finalize_lazy(c)) return rc;
  c->lazy_new = on != 0;
  return 0;
}

int esvio_fe_set_host_threads(esvio_fe_handle c, int threads) {
  if (!c || threads < 1 || threads > 16) return ESVIO_FE_EINVAL;
  host::ransac_pool_destroy(c->pool);
  c->pool = host::ransac_pool_create(threads - 1);
  stager_share_pool(c);
  return 0;
}

int esvio_fe_finish(esvio_fe_handle c, esvio_fe_tracks* out) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = finalize_lazy(c)) return rc;
  return fill_tracks(c, out);
}

static int set_next_batch_impl(esvio_fe_handle c, double next_cur_time, const esvio_fe_event* left,
                               size_t nL, const esvio_fe_event* right, size_t nR, int space,
                               int pub_hint, const esvio_fe_motion* motion) {
  if (!c) return ESVIO_FE_EINVAL;
  if (nL == 0 || !left || (nR && !right)) return fail(c, ESVIO_FE_EINVAL, "bad next batch");
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return ESVIO_FE_EINVAL;
  if (c->ext_right_pending) return fail(c, ESVIO_FE_EINVAL, "not with an imported right image");
  if (c->evimg.mode == 1)
    return fail(c, ESVIO_FE_EINVAL, "not while esvio_fe_set_event_images is 1: the event images do not follow announced batches (ESVIO_FE_EVENT_IMAGES_AHEAD does)");
  if ((int)(c->announced.size() + c->inflight.size()) >= 2 * kPrefetchDepth)
    return fail(c, ESVIO_FE_EINVAL, "at most %d batches can be announced and not yet tracked", 2 * kPrefetchDepth);
  Batch b;
  b.time = next_cur_time;
  b.left = left;
  b.nL = nL;
  b.right = right;
  b.nR = nR;
  b.space = space;
  b.pub = pub_hint != 0;
  if (motion) {
    b.has_motion = true;
    b.motion = *motion;
  }
  if (space == ESVIO_FE_HOST && stager_enabled(c)) {
    // the batch starts on its way to the device now: pinned chunks + DMA by the helper threads, under
    // the frames tracked before it
    HIPCHK(c, hipSetDevice(c->dev));
    // (one DMA for the whole batch.  Round 4 measured two to four, and the odd ones on a second copy stream:
    // no gain in the bench's configuration — 0.136-0.146 ms/step either way — and a loss without the RANSAC
    // helpers' share of the copying, 0.140 -> 0.165-0.18; two DMA engines at once: 0.197)
    if (int rc = stager_begin(c, left, nL, right, nR, 1, &b.stage)) return rc;
  } else if (space == ESVIO_FE_DEVICE && !c->stream6) {
    // (the first announcement of a batch that is already on the device: the second stereo stream, if this handle
    // is going to use it — here and not in esvio_fe_set_launch_thread, because a handle that is fed host batches
    // never splits and a stream it does not use still takes a hardware queue from the process's pool)
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = stereo_split_prepare(c)) return rc;
  }
  c->announced.push_back(b);
  return 0;
}

int esvio_fe_set_next_batch(esvio_fe_handle c, double next_cur_time, const esvio_fe_event* left,
                            size_t nL, const esvio_fe_event* right, size_t nR, int space,
                            int pub_hint) {
  return set_next_batch_impl(c, next_cur_time, left, nL, right, nR, space, pub_hint, nullptr);
}

int esvio_fe_set_next_batch_mc(esvio_fe_handle c, double next_cur_time, const esvio_fe_event* left,
                               size_t nL, const esvio_fe_event* right, size_t nR, int space,
                               int pub_hint, const esvio_fe_motion* motion) {
  if (!motion) return ESVIO_FE_EINVAL;
  return set_next_batch_impl(c, next_cur_time, left, nL, right, nR, space, pub_hint, motion);
}

int esvio_fe_mem_alloc(int space, size_t bytes, void** out) {
  if (!out || (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE)) return ESVIO_FE_EINVAL;
  *out = nullptr;
  const size_t b = std::max<size_t>(bytes, 16);
  const hipError_t e = space == ESVIO_FE_HOST ? hipHostMalloc(out, b, hipHostMallocDefault) : hipMalloc(out, b);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return ESVIO_FE_EHIP;
  }
  return 0;
}

int esvio_fe_mem_free(int space, void* p) {
  if (space != ESVIO_FE_HOST && space != ESVIO_FE_DEVICE) return ESVIO_FE_EINVAL;
  if (!p) return 0;
  return (space == ESVIO_FE_HOST ? hipHostFree(p) : hipFree(p)) == hipSuccess ? 0 : ESVIO_FE_EHIP;
}

int esvio_fe_mem_upload(void* dst_device, const void* src_host, size_t bytes) {
  if (bytes && (!dst_device || !src_host)) return ESVIO_FE_EINVAL;
  if (!bytes) return 0;
  return hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : ESVIO_FE_EHIP;
}

int esvio_fe_register_host_buffer(void* p, size_t bytes) {
  if (!p || !bytes) return ESVIO_FE_EINVAL;
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return ESVIO_FE_EHIP;
  }
  return 0;
}

int esvio_fe_unregister_host_buffer(void* p) {
  if (!p) return ESVIO_FE_EINVAL;
  if (hipHostUnregister(p) != hipSuccess) {
    (void)hipGetLastError();
    return ESVIO_FE_EHIP;
  }
  return 0;
}

int esvio_fe_debug_inject(esvio_fe_handle c, int mask) {
  if (!c || mask < 0 || mask > 31) return ESVIO_FE_EINVAL;
  c->lim = esvio_fe_ctx::WaitLimits();
  c->lazy_late = (mask & ESVIO_FE_FAULT_LAZY_LATE) != 0;
  if (mask & ESVIO_FE_FAULT_TICKET) c->lim.ticket = 0;
  if (mask & ESVIO_FE_FAULT_LOOKBACK) c->lim.lookback = 0;
  if (mask & ESVIO_FE_FAULT_SPECULATIVE) c->lim.poll = 0;
  if (mask & ESVIO_FE_FAULT_CHAINED) c->lim.chain = 0;
  return 0;
}

int esvio_fe_debug_counters(esvio_fe_handle c, uint64_t out4[4]) {
  if (!c || !out4) return ESVIO_FE_EINVAL;
  out4[0] = c->n_spec_expired;
  out4[1] = c->n_chain_expired;
  out4[2] = c->tr_chain_launch;
  out4[3] = c->tr_chain_used;
  return 0;
}

int esvio_fe_plain_call_counters(esvio_fe_handle c, uint64_t out4[4]) {
  if (!c || !out4) return ESVIO_FE_EINVAL;
  out4[0] = c->n_plain_calls;
  out4[1] = c->n_cam_split;
  out4[2] = c->n_stereo_chained;
  out4[3] = c->n_chain_expired;
  return 0;
}

int esvio_fe_reserve(esvio_fe_handle c, size_t max_left, size_t max_right, int host_batches) {
  if (!c) return ESVIO_FE_EINVAL;
  const size_t n = max_left + max_right;
  if (n >= (1ull << 31)) return fail(c, ESVIO_FE_EINVAL, "batch too large");
  if (!c->inflight.empty() || !c->announced.empty())
    return fail(c, ESVIO_FE_EINVAL, "esvio_fe_reserve while batches are announced");
  HIPCHK(c, hipSetDevice(c->dev));
  // (growing frees the old buffers: nothing may still be using them)
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(c->stream3));
  HIPCHK(c, hipStreamSynchronize(c->stream4));
  if (c->stream6) HIPCHK(c, hipStreamSynchronize(c->stream6));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->tiled) {
    if (int rc = ensure_part_capacity(c, n, false)) return rc;
  } else if (int rc = ensure_sort_capacity(c, n)) {
    return rc;
  }
  for (int k = 0; k < kRightSlots; k++)
    if (int rc = ensure_arc_capacity(c, max_left, k)) return rc;
  // a handle that filters (esvio_fe_filter_events): the stage's scratch for one camera's batch and, for host batches,
  // the copy of a host source — not the records behind a host dst, which grow on the first call that has one
  if (c->baf.B)
    if (int rc = baf_ensure(c, std::max(max_left, max_right), host_batches != 0, false, false)) return rc;
  // a handle that has used an ingest stage: the stage's scratch for chunks of max_left and max_right events
  const size_t events[2] = {max_left, max_right};
  if (int rc = raw_reserve(c, events, host_batches != 0)) return rc;
  if (int rc = text_reserve(c, events, host_batches != 0)) return rc;
  if (int rc = aedat_reserve(c, events)) return rc;
  if (int rc = bag_reserve(c, events)) return rc;
  if (int rc = bag_image_reserve(c)) return rc;
  if (int rc = aedat_frame_reserve(c)) return rc;
  // a handle with an open feed: per camera both buffers for 2 * max_events records (the one that holds records is left alone)
  if (c->feed.open) {
    const size_t ev[2] = {max_left, max_right};
    for (int cam = 0; cam < 2; cam++) {
      esvio_fe_ctx::Feed::Cam& fc = c->feed.cam[cam];
      for (int b = 0; b < 2; b++)
        if ((b != fc.cur || fc.len == 0) && fc.buf[b].cap < 2 * ev[cam]) {
          if (int rc = fc.buf[b].alloc(c, 2 * ev[cam])) return rc;
          fc.read_rec[b] = false;
        }
    }
  }
  if (host_batches) {
    if (int rc = ensure_event_capacity(c, n)) return rc;
    if (stager_enabled(c)) {
      if (int rc = stager_reserve(c, n)) return rc;
    } else {
      for (int lane = 0; lane < kPrefetchDepth; lane++)
        if (n > c->d_evp[lane].cap)
          if (int rc = c->d_evp[lane].alloc(c, n + n / 4)) return rc;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

const char* esvio_fe_latency_phase_name(int i) {
  return (i >= 0 && i < PH_COUNT) ? kPhaseNames[i] : "";
}

int esvio_fe_latency_recent(esvio_fe_handle c, int back, esvio_fe_latency_call* out) {
  if (!c || !out || back < 0) return ESVIO_FE_EINVAL;
  const esvio_fe_ctx::Latency& L = c->lat;
  if ((uint64_t)back >= L.total_calls || back >= esvio_fe_ctx::Latency::kRecent) return ESVIO_FE_EINVAL;
  *out = L.recent[(L.total_calls - 1 - (uint64_t)back) % esvio_fe_ctx::Latency::kRecent];
  return 0;
}

int esvio_fe_latency_stats(esvio_fe_handle c, esvio_fe_latency* out, int reset) {
  if (!c || !out) return ESVIO_FE_EINVAL;
  const esvio_fe_ctx::Latency& L = c->lat;
  std::memset(out, 0, sizeof(*out));
  out->calls = L.calls;
  const size_t n = (size_t)std::min<uint64_t>(L.calls, esvio_fe_ctx::Latency::kRing);
  if (n) {
    std::vector<float> v(L.ring, L.ring + n);
    std::sort(v.begin(), v.end());
    out->mean_ms = L.sum_ms / (double)L.calls;
    out->p50_ms = v[n / 2];
    out->p99_ms = v[std::min(n - 1, (size_t)((double)n * 0.99))];
    out->max_ms = L.max_ms;
    out->max_call = L.max_call;
    out->max_published = L.max_pub;
    out->max_cpu_begin = L.max_cpu0;
    out->max_cpu_end = L.max_cpu1;
    out->max_invol_switches = L.max_nivcsw;
    out->max_allocs = L.max_allocs;
    std::memcpy(out->max_phase_ms, L.max_phase, sizeof(out->max_phase_ms));
  }
  out->allocs = L.allocs;
  out->invol_switches = L.nivcsw;
  if (reset) c->lat = esvio_fe_ctx::Latency();
  return 0;
}

int esvio_fe_ransac_tail(uint64_t out6[6], int reset) {
  if (!out6) return ESVIO_FE_EINVAL;
  host::ransac_tail(out6, reset != 0);
  return 0;
}

int esvio_fe_set_launch_thread(esvio_fe_handle c, int on) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  return launcher_set(c, on != 0);
}

int esvio_fe_set_profiling(esvio_fe_handle c, int on) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = launcher_drain(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  c->prof_on = on != 0;
  return 0;
}
int esvio_fe_device_memory(esvio_fe_handle c, size_t* free_bytes, size_t* total_bytes) {
  if (!c || !free_bytes || !total_bytes) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipMemGetInfo(free_bytes, total_bytes));
  return 0;
}

int esvio_fe_kernel_count(void) { return kTrackKernels; }
int esvio_fe_stage_kernel_count(void) { return K_COUNT; }
int esvio_fe_ingest_kernel_count(void) { return K_INGEST_COUNT; }
const char* esvio_fe_kernel_name(int id) {
  return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : (id >= K_COUNT && id < K_INGEST_COUNT) ? kIngestKernelNames[id - K_COUNT] : "";
}
int esvio_fe_get_kernel_stats(esvio_fe_handle c, int id, double* total_ms, uint64_t* launches,
                              uint64_t* alg_bytes) {
  if (!c || id < 0 || id >= K_INGEST_COUNT) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  if (int rc = launcher_drain(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  if (total_ms) *total_ms = c->stats[id].ms;
  if (launches) *launches = c->stats[id].launches;
  if (alg_bytes) *alg_bytes = c->stats[id].bytes;
  return 0;
}
int esvio_fe_reset_kernel_stats(esvio_fe_handle c) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  for (auto& s : c->stats) s = KStat();
  return 0;
}
void* esvio_fe_stream(esvio_fe_handle c) { return c ? (void*)cur_stream(c) : nullptr; }

// ---- rosbag images (the rule: include/esvio_fe.h "rosbag images"; the host walk: fe_bag.h; the kernel: fe_kernels.h)
namespace {
size_t bag_image_slot(size_t payload_bytes) { return (payload_bytes + 15) & ~(size_t)15; }
// the scratch of pix_bytes gathered payload bytes (padding included) and n_images descriptors, and gray_bytes behind a host dst
int bag_image_ensure(esvio_fe_ctx* c, size_t pix_bytes, size_t n_images, size_t gray_bytes) {
  esvio_fe_ctx::Bag& B = c->bag;
  B.img_used = true;
  const size_t bytes = bag_image_slot(pix_bytes) + 16 + n_images * sizeof(ImageDesc);  // (16: convert_image keeps its source's offset from a 16-byte boundary)
  if (int rc = B.h_img.grow(c, bytes)) return rc;
  if (int rc = B.d_img.grow(c, bytes)) return rc;
  return gray_bytes ? B.d_gray.grow(c, gray_bytes) : 0;
}
// esvio_fe_reserve for a handle that decodes bag images: the scratch of one stereo pair of rgb8 frames of its size
int bag_image_reserve(esvio_fe_ctx* c) {
  return c->bag.img_used ? bag_image_ensure(c, 2 * bag_image_slot((size_t)c->W * c->H * 3), 2, 2 * (size_t)c->W * c->H) : 0;
}
void bag_image_state_reset(esvio_fe_ctx* c) { c->bag.img_st = bg::Walk{}; }
// the copy of the gathered bytes and the table, and the launch, on the current stream; nothing is waited for
int bag_image_enqueue(esvio_fe_ctx* c, size_t table_at, uint32_t n_images, uint32_t width, uint32_t height, uint64_t alg_bytes) {
  esvio_fe_ctx::Bag& B = c->bag;
  hipStream_t s = cur_stream(c);
  HIPCHK(c, hipMemcpyAsync(B.d_img, B.h_img, table_at + n_images * sizeof(ImageDesc), hipMemcpyHostToDevice, s));
  ImageArgs a{};
  a.desc = (const ImageDesc*)(B.d_img.p + table_at), a.n_images = n_images, a.width = width, a.height = height;
  ScopedKernel k(c, K_IMAGE_EMIT, alg_bytes);
  launch_image_emit(s, a);
  return 0;
}
}  // namespace

int esvio_fe_image_tile_pixels(void) { return (int)kImageTile; }

int esvio_fe_bag_set_image_topics(esvio_fe_handle c, const char* left, const char* right) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* why = nullptr;
  if (!bg::set_image_topics(left, right, &c->bag.topics, &why)) return fail(c, ESVIO_FE_EINVAL, "bag_set_image_topics: %s", why);
  bag_image_state_reset(c);
  return 0;
}

int esvio_fe_decode_bag_images(esvio_fe_handle c, const void* bytes, size_t n_bytes, uint32_t flags, uint8_t* const dst[2],
                               const size_t dst_cap[2], int dst_space, esvio_fe_bag_image* msgs, size_t msgs_cap,
                               esvio_fe_bag_image_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info) *info = esvio_fe_bag_image_info{};
  const char* who = "decode_bag_images";
  if (int rc = bag_args_check(c, who, bytes, n_bytes, flags)) return rc;
  if (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  const size_t room[2] = {dst && dst_cap ? dst_cap[0] : 0, dst && dst_cap ? dst_cap[1] : 0};
  for (int cam = 0; cam < 2; cam++)
    if (room[cam] && !dst[cam]) return fail(c, ESVIO_FE_EINVAL, "%s: dst[%d] is null", who, cam);
  if (msgs_cap && !msgs) return fail(c, ESVIO_FE_EINVAL, "%s: msgs is null", who);
  if (!n_bytes) return 0;
  esvio_fe_ctx::Bag& B = c->bag;
  const uint32_t W = (uint32_t)c->W, H = (uint32_t)c->H;
  const size_t wh = (size_t)W * H;
  // the counting walk: everything in the chunk checked, the messages and their bytes counted, nothing stored or moved
  bg::Out cnt;
  cnt.want_w = W, cnt.want_h = H;
  {
    bg::Walk probe = B.img_st;
    if (!bg::walk(&probe, B.topics, bg::kImages, (const uint8_t*)bytes, n_bytes, &cnt))
      return fail(c, ESVIO_FE_EINVAL, "%s: malformed bag or refused message (%s); the walker's state is as it was", who, cnt.why);
  }
  const size_t n[2] = {(size_t)cnt.n_cam_imgs[0], (size_t)cnt.n_cam_imgs[1]};
  if (info) {
    for (int cam = 0; cam < 2; cam++) {
      esvio_fe_bag_image_cam_info& ci = info->cam[cam];
      ci.images = n[cam];
      ci.first_sec = cnt.first_stamp[cam][0], ci.first_nsec = cnt.first_stamp[cam][1], ci.last_sec = cnt.last_stamp[cam][0], ci.last_nsec = cnt.last_stamp[cam][1];
    }
    info->other_messages = cnt.other_messages, info->other_records = cnt.other_records, info->chunks = cnt.chunks, info->connections = cnt.connections;
  }
  if (n[0] > room[0] || n[1] > room[1])
    return fail(c, ESVIO_FE_EINVAL, "%s: the chunk completes %zu left and %zu right images, dst has room for %zu and %zu; the walker's state is as it was", who,
                n[0], n[1], room[0], room[1]);
  if (cnt.n_imgs > msgs_cap)
    return fail(c, ESVIO_FE_EINVAL, "%s: the chunk completes %llu image messages, msgs has room for %zu; the walker's state is as it was", who,
                (unsigned long long)cnt.n_imgs, msgs_cap);
  const size_t n_all = (size_t)cnt.n_imgs, table_at = (size_t)cnt.n_pix_bytes;
  if (n_all) {
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = bag_image_ensure(c, table_at, n_all, dst_space == ESVIO_FE_HOST ? n_all * wh : 0)) return rc;
  }
  // the gathering walk (checked by the counting walk): the completed payloads into the pinned scratch, what the call's end
  // cuts into the carry; the state it leaves is taken over at the end
  bg::Out o;
  o.want_w = W, o.want_h = H, o.carry = &B.carry;
  o.pix = n_all ? B.h_img.p : nullptr, o.pix_cap = table_at, o.imgs = msgs, o.imgs_cap = msgs_cap;
  bg::Walk st = B.img_st;
  bg::walk(&st, B.topics, bg::kImages, (const uint8_t*)bytes, n_bytes, &o);
  if (n_all) {
    ImageDesc* desc = (ImageDesc*)(B.h_img.p + table_at);
    size_t at = 0;
    uint64_t alg = 0;
    for (size_t k = 0; k < n_all; k++) {
      const esvio_fe_bag_image& m = msgs[k];
      uint8_t* base = dst_space == ESVIO_FE_HOST ? B.d_gray.p + (m.cam ? n[0] * wh : 0) : dst[m.cam];
      desc[k] = ImageDesc{B.d_img.p + at, base + (size_t)m.index * wh, m.step, (uint32_t)m.encoding};
      at += bag_image_slot((size_t)m.step * m.height);
      alg += (uint64_t)wh * (bg::encoding_bpp(m.encoding) + 1);
    }
    if (int rc = bag_image_enqueue(c, table_at, (uint32_t)n_all, W, H, alg)) return rc;
    if (dst_space == ESVIO_FE_HOST)
      for (int cam = 0; cam < 2; cam++)
        if (n[cam]) HIPCHK(c, hipMemcpyAsync(dst[cam], B.d_gray.p + (cam ? n[0] * wh : 0), n[cam] * wh, hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
    if (c->prof_on) resolve_profile(c);
  }
  B.img_st = st;
  return 0;
}

int esvio_fe_convert_image(esvio_fe_handle c, const void* src, int src_space, uint32_t height, uint32_t width, uint32_t step,
                           int32_t encoding, uint8_t* dst, int dst_space) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "convert_image";
  if (!src || !dst) return fail(c, ESVIO_FE_EINVAL, "%s: src or dst is null", who);
  if ((src_space != ESVIO_FE_HOST && src_space != ESVIO_FE_DEVICE) || (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE))
    return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (height < 1 || height > kImageMaxSide || width < 1 || width > kImageMaxSide)
    return fail(c, ESVIO_FE_EINVAL, "%s: height and width must be 1 .. %u", who, kImageMaxSide);
  if (encoding < bg::kEncMono || encoding > bg::kEncRgb) return fail(c, ESVIO_FE_EINVAL, "%s: encoding must be 1 (mono8, 8UC1), 2 (bgr8, 8UC3) or 3 (rgb8)", who);
  const size_t row = (size_t)width * bg::encoding_bpp(encoding), wh = (size_t)width * height;
  if (step < row) return fail(c, ESVIO_FE_EINVAL, "%s: step is below width * bytes per pixel", who);
  const size_t need = (size_t)step * (height - 1) + row;  // the bytes up to the last row's last pixel
  if (need > kRawMaxBytes) return fail(c, ESVIO_FE_EINVAL, "%s: a source holds at most 2^28 bytes", who);
  esvio_fe_ctx::Bag& B = c->bag;
  HIPCHK(c, hipSetDevice(c->dev));
  const size_t lead = src_space == ESVIO_FE_HOST ? (size_t)((uintptr_t)src & 15) : 0;  // the copy lies as the source does
  const size_t table_at = bag_image_slot(src_space == ESVIO_FE_HOST ? lead + need : 0);
  if (int rc = bag_image_ensure(c, table_at, 1, dst_space == ESVIO_FE_HOST ? wh : 0)) return rc;
  if (src_space == ESVIO_FE_HOST) memcpy(B.h_img.p + lead, src, need);
  ImageDesc* desc = (ImageDesc*)(B.h_img.p + table_at);
  desc[0] = ImageDesc{src_space == ESVIO_FE_HOST ? B.d_img.p + lead : (const uint8_t*)src, dst_space == ESVIO_FE_HOST ? B.d_gray.p : dst, step, (uint32_t)encoding};
  if (int rc = bag_image_enqueue(c, table_at, 1, width, height, (uint64_t)wh * (bg::encoding_bpp(encoding) + 1))) return rc;
  if (dst_space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(dst, B.d_gray.p, wh, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// the image walk tap (include/esvio_fe_test.h): the host walk alone, no handle, no device
int esvio_fe_bag_image_walk_tap(void* state, size_t state_bytes, const char* left, const char* right, uint32_t width, uint32_t height,
                                const void* bytes, size_t n_bytes, uint8_t* carry, size_t carry_cap, uint8_t* pix, size_t pix_cap,
                                esvio_fe_bag_image* imgs, size_t imgs_cap, uint64_t counts[12], char* why, size_t why_cap) {
  if (why && why_cap) why[0] = 0;
  if (!state || state_bytes != sizeof(bg::Walk) || (n_bytes && !bytes) || !counts) return ESVIO_FE_EINVAL;
  bg::Topics t;
  const char* bad_topics = nullptr;
  if (!bg::set_image_topics(left, right, &t, &bad_topics)) return ESVIO_FE_EINVAL;
  bg::Walk st;
  memcpy(&st, state, sizeof st);
  if (st.carry_len > carry_cap || (st.carry_len && !carry)) return ESVIO_FE_EINVAL;
  bg::Carry cy;
  if (st.carry_len) cy.buf[st.carry_buf & 1u].assign(carry, carry + st.carry_len);
  bg::Out cnt, o;
  cnt.want_w = o.want_w = width, cnt.want_h = o.want_h = height;
  bg::Walk probe = st;
  bool ok = bg::walk(&probe, t, bg::kImages, (const uint8_t*)bytes, n_bytes, &cnt);  // the counting walk, as the library's call does
  if (ok) {
    o.carry = &cy;
    if (pix && cnt.n_pix_bytes <= pix_cap) o.pix = pix, o.pix_cap = pix_cap;
    o.imgs = imgs, o.imgs_cap = imgs ? imgs_cap : 0;
    bg::walk(&st, t, bg::kImages, (const uint8_t*)bytes, n_bytes, &o);
    ok = st.carry_len <= carry_cap && (!st.carry_len || carry);
  }
  const uint64_t v[12] = {cnt.n_imgs, cnt.n_cam_imgs[0], cnt.n_cam_imgs[1], cnt.n_pix_bytes, cnt.other_messages, cnt.other_records,
                          cnt.chunks, cnt.connections, ok ? st.carry_len : 0, 0, 0, 0};
  memcpy(counts, v, sizeof v);
  if (!ok) {  // (the caller's state and carry are as they were)
    if (why && why_cap) snprintf(why, why_cap, "%s", cnt.why ? cnt.why : "carry_cap is too small for the bytes that wait");
    return ESVIO_FE_EINVAL;
  }
  if (st.carry_len) memcpy(carry, cy.buf[st.carry_buf & 1u].data(), (size_t)st.carry_len);
  memcpy(state, &st, sizeof st);
  return 0;
}

// ---- AEDAT 3.1 frames (the rule: include/esvio_fe.h "AEDAT 3.1 frames"; the host walk: fe_aedat.h; the kernel: fe_kernels.h)
namespace {
size_t frame_slot(size_t pixel_bytes) { return (pixel_bytes + 15) & ~(size_t)15; }
// the scratch of pix_bytes gathered pixel bytes (padding included) and n_frames descriptors, and gray_bytes behind a host dst
int aedat_frame_ensure(esvio_fe_ctx* c, size_t pix_bytes, size_t n_frames, size_t gray_bytes) {
  esvio_fe_ctx::Aedat& A = c->aedat;
  A.frm_used = true;
  const size_t bytes = frame_slot(pix_bytes) + n_frames * sizeof(Frame16Desc);
  if (int rc = A.h_frm.grow(c, bytes)) return rc;
  if (int rc = A.d_frm.grow(c, bytes)) return rc;
  return gray_bytes ? A.d_gray.grow(c, gray_bytes) : 0;
}
// esvio_fe_reserve for a handle that decodes frames: the scratch of one rgb frame of its size
int aedat_frame_reserve(esvio_fe_ctx* c) {
  return c->aedat.frm_used ? aedat_frame_ensure(c, frame_slot((size_t)c->W * c->H * 6), 1, (size_t)c->W * c->H) : 0;
}
// the copy of the gathered bytes and the table, and the launch, on the current stream; nothing is waited for
int aedat_frame_enqueue(esvio_fe_ctx* c, size_t table_at, uint32_t n_frames, uint32_t width, uint32_t height, uint64_t alg_bytes) {
  esvio_fe_ctx::Aedat& A = c->aedat;
  hipStream_t s = cur_stream(c);
  HIPCHK(c, hipMemcpyAsync(A.d_frm, A.h_frm, table_at + n_frames * sizeof(Frame16Desc), hipMemcpyHostToDevice, s));
  Frame16Args a{};
  a.desc = (const Frame16Desc*)(A.d_frm.p + table_at), a.n_frames = n_frames, a.width = width, a.height = height;
  ScopedKernel k(c, K_FRAME16_EMIT, alg_bytes);
  launch_frame16_emit(s, a);
  return 0;
}
}  // namespace

int esvio_fe_frame16_tile_pixels(void) { return (int)kFrame16Tile; }

int esvio_fe_aedat_frame_kernel_stats(esvio_fe_handle c, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  const KStat& s = c->stats[K_FRAME16_EMIT];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}

int esvio_fe_decode_aedat_frames(esvio_fe_handle c, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                                 uint8_t* dst, size_t dst_cap, int dst_space, esvio_fe_aedat_frame* frames, size_t frames_cap,
                                 esvio_fe_aedat_frame_info* info) {
  if (!c) return ESVIO_FE_EINVAL;
  if (info) *info = esvio_fe_aedat_frame_info{};
  const char* who = "decode_aedat_frames";
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (int rc = aedat_args_check(c, who, bytes, n_bytes, t_offset_ns, flags)) return rc;
  if (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (dst_cap && !dst) return fail(c, ESVIO_FE_EINVAL, "%s: dst is null", who);
  if (frames_cap && !frames) return fail(c, ESVIO_FE_EINVAL, "%s: frames is null", who);
  if (!n_bytes) return 0;
  esvio_fe_ctx::Aedat& A = c->aedat;
  const uint32_t W = (uint32_t)c->W, H = (uint32_t)c->H;
  const size_t wh = (size_t)W * H;
  // the counting walk: everything in the chunk checked, the frames and their bytes counted, nothing stored or moved
  ae::Out cnt;
  cnt.want_w = W, cnt.want_h = H;
  {
    ae::Walk probe = A.frame_st[cam];
    if (!ae::walk(&probe, ae::kFrames, (const uint8_t*)bytes, n_bytes, t_offset_ns, flags, &cnt))
      return fail(c, ESVIO_FE_EINVAL, "%s: malformed packet or refused frame (%s); the camera's state is as it was", who, cnt.why);
  }
  if (info) {
    info->frames = cnt.n_frames, info->invalid = cnt.invalid, info->bad = cnt.bad;
    info->frame_packets = cnt.frame_packets, info->other_packets = cnt.other_packets;
    info->first_sec = cnt.first_stamp[0], info->first_nsec = cnt.first_stamp[1], info->last_sec = cnt.last_stamp[0], info->last_nsec = cnt.last_stamp[1];
  }
  if (cnt.bad)
    return fail(c, ESVIO_FE_EINVAL, "%s: %llu frames have a stamp outside [0, 2^32 s); the camera's state is as it was", who, (unsigned long long)cnt.bad);
  if (cnt.n_frames > dst_cap || cnt.n_frames > frames_cap)
    return fail(c, ESVIO_FE_EINVAL, "%s: the chunk completes %llu frames, dst has room for %zu and frames for %zu; the camera's state is as it was", who,
                (unsigned long long)cnt.n_frames, dst_cap, frames_cap);
  const size_t n_all = (size_t)cnt.n_frames, table_at = (size_t)cnt.n_pix_bytes;
  if (n_all) {
    HIPCHK(c, hipSetDevice(c->dev));
    if (int rc = aedat_frame_ensure(c, table_at, n_all, dst_space == ESVIO_FE_HOST ? n_all * wh : 0)) return rc;
  }
  // the gathering walk (checked by the counting walk): the emitted frames' pixel bytes into the pinned scratch, what the
  // call's end cuts into the carry; the state it leaves is taken over at the end
  ae::Out o;
  o.want_w = W, o.want_h = H, o.carry = &A.carry[cam];
  o.pix = n_all ? A.h_frm.p : nullptr, o.pix_cap = table_at, o.frames = frames, o.frames_cap = frames_cap;
  ae::Walk st = A.frame_st[cam];
  ae::walk(&st, ae::kFrames, (const uint8_t*)bytes, n_bytes, t_offset_ns, flags, &o);
  if (n_all) {
    Frame16Desc* desc = (Frame16Desc*)(A.h_frm.p + table_at);
    uint8_t* base = dst_space == ESVIO_FE_HOST ? A.d_gray.p : dst;
    size_t at = 0;
    uint64_t alg = 0;
    for (size_t k = 0; k < n_all; k++) {
      const uint32_t ch = (uint32_t)frames[k].channels;
      desc[k] = Frame16Desc{A.d_frm.p + at, base + k * wh, ch, 0u};
      at += frame_slot(wh * ch * 2);
      alg += (uint64_t)wh * (ch * 2 + 1);
    }
    if (int rc = aedat_frame_enqueue(c, table_at, (uint32_t)n_all, W, H, alg)) return rc;
    if (dst_space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(dst, A.d_gray.p, n_all * wh, hipMemcpyDeviceToHost, cur_stream(c)));
    HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
    if (c->prof_on) resolve_profile(c);
  }
  A.frame_st[cam] = st;
  return 0;
}

int esvio_fe_convert_frame16(esvio_fe_handle c, const uint16_t* src, int src_space, uint32_t height, uint32_t width, int32_t channels,
                             uint8_t* dst, int dst_space) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "convert_frame16";
  if (!src || !dst) return fail(c, ESVIO_FE_EINVAL, "%s: src or dst is null", who);
  if ((src_space != ESVIO_FE_HOST && src_space != ESVIO_FE_DEVICE) || (dst_space != ESVIO_FE_HOST && dst_space != ESVIO_FE_DEVICE))
    return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (height < 1 || height > kImageMaxSide || width < 1 || width > kImageMaxSide)
    return fail(c, ESVIO_FE_EINVAL, "%s: height and width must be 1 .. %u", who, kImageMaxSide);
  if (channels != 1 && channels != 3) return fail(c, ESVIO_FE_EINVAL, "%s: channels must be 1 (mono8) or 3 (rgb8), got %d", who, channels);
  if ((uintptr_t)src & 1u) return fail(c, ESVIO_FE_EINVAL, "%s: src must be 2-byte aligned", who);
  const size_t wh = (size_t)width * height, need = wh * (size_t)channels * 2;
  esvio_fe_ctx::Aedat& A = c->aedat;
  HIPCHK(c, hipSetDevice(c->dev));
  const size_t table_at = frame_slot(src_space == ESVIO_FE_HOST ? need : 0);
  if (int rc = aedat_frame_ensure(c, table_at, 1, dst_space == ESVIO_FE_HOST ? wh : 0)) return rc;
  if (src_space == ESVIO_FE_HOST) memcpy(A.h_frm.p, src, need);
  Frame16Desc* desc = (Frame16Desc*)(A.h_frm.p + table_at);
  desc[0] = Frame16Desc{src_space == ESVIO_FE_HOST ? A.d_frm.p : (const uint8_t*)src, dst_space == ESVIO_FE_HOST ? A.d_gray.p : dst, (uint32_t)channels, 0u};
  if (int rc = aedat_frame_enqueue(c, table_at, 1, width, height, (uint64_t)wh * (channels * 2 + 1))) return rc;
  if (dst_space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(dst, A.d_gray.p, wh, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  if (c->prof_on) resolve_profile(c);
  return 0;
}

// the frame walk tap (include/esvio_fe_test.h): the host walk alone, no handle, no device
int esvio_fe_aedat_frame_walk_tap(void* state, size_t state_bytes, uint32_t width, uint32_t height, const void* bytes, size_t n_bytes,
                                  int64_t t_offset_ns, uint32_t flags, uint8_t* carry, size_t carry_cap, uint8_t* pix, size_t pix_cap,
                                  esvio_fe_aedat_frame* frames, size_t frames_cap, uint64_t counts[8], char* why, size_t why_cap) {
  if (why && why_cap) why[0] = 0;
  if (!state || state_bytes != sizeof(ae::Walk) || (n_bytes && !bytes) || !counts) return ESVIO_FE_EINVAL;
  ae::Walk st;
  memcpy(&st, state, sizeof st);
  if (st.carry_len > carry_cap || (st.carry_len && !carry)) return ESVIO_FE_EINVAL;
  ae::Carry cy;
  if (st.carry_len) cy.buf[st.carry_buf & 1u].assign(carry, carry + st.carry_len);
  ae::Out cnt, o;
  cnt.want_w = o.want_w = width, cnt.want_h = o.want_h = height;
  ae::Walk probe = st;
  bool ok = ae::walk(&probe, ae::kFrames, (const uint8_t*)bytes, n_bytes, t_offset_ns, flags, &cnt);  // the counting walk, as the library's call does
  char bad_text[64];
  if (ok && cnt.bad) {
    snprintf(bad_text, sizeof bad_text, "%llu frames have a BAD stamp", (unsigned long long)cnt.bad);
    cnt.why = bad_text, ok = false;
  }
  if (ok) {
    o.carry = &cy;
    if (pix && cnt.n_pix_bytes <= pix_cap) o.pix = pix, o.pix_cap = pix_cap;
    o.frames = frames, o.frames_cap = frames ? frames_cap : 0;
    ae::walk(&st, ae::kFrames, (const uint8_t*)bytes, n_bytes, t_offset_ns, flags, &o);
    ok = st.carry_len <= carry_cap && (!st.carry_len || carry);
  }
  const uint64_t v[8] = {cnt.n_frames, cnt.n_pix_bytes, cnt.invalid, cnt.bad, cnt.frame_packets, cnt.other_packets, ok ? st.carry_len : 0, 0};
  memcpy(counts, v, sizeof v);
  if (!ok) {  // (the caller's state and carry are as they were)
    if (why && why_cap) snprintf(why, why_cap, "%s", cnt.why ? cnt.why : "carry_cap is too small for the bytes that wait");
    return ESVIO_FE_EINVAL;
  }
  if (st.carry_len) memcpy(carry, cy.buf[st.carry_buf & 1u].data(), (size_t)st.carry_len);
  memcpy(state, &st, sizeof st);
  return 0;
}

}  // extern "C"

// ---- loop-closure keyframes (the rules: include/esvio_fe.h "keyframes"; the kernels: fe_kernels.h)
#include "fe_kf.h"

// ---- loop detection: DBoW2 words, database, L1 query (the rules: include/esvio_fe.h "loop detection")
#include "fe_bow.h"

// ---- creating a vocabulary: k-means++, the tree, the word weights (the rule: include/esvio_fe.h "C")
#include "fe_voc.h"
