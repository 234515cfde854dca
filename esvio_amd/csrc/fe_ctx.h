// fe_ctx.h — the handle (esvio_fe_ctx) and the small helpers every part of the library uses.
// Internal: the public boundary is include/esvio_fe.h.
//
//   fe_stages.cpp  device memory, the per-stage launches (SAE update, rendering, pyramids, LK, Arc*,
//                  selection) and the <= max_cnt-point host bookkeeping of the reference
//   fe_track.cpp   FeatureTracker::trackEvent: the per-frame sequence and its replay-mode scheduler
//                  (prefetch stream, speculative / chained temporal LK, lazy right-camera tails)
//   fe_image.cpp   FeatureTracker::trackImage and goodFeaturesToTrack
//   fe_api.cpp     the C ABI entry points
//   fe_layout.h    the layout of the blocks the LK kernels work in (d_res / h_pin, h_spec) and the views of them
//                  the handle keeps; no HIP, every offset into those blocks is computed there
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <string>
#include <utility>
#include <deque>
#include <vector>

#include "../../include/esvio_fe.h"
#include "../../include/esvio_fe_test.h"
#include "fe_aedat.h"
#include "fe_bag.h"
#include "fe_host.h"
#include "fe_kernels.h"
#include "fe_layout.h"
#include "fe_mc.h"
#include "fe_res.h"
#include "fe_text.h"

using namespace esvio;

namespace esvio {
namespace fe {

// std::map<int, cv::Point2f> as ptsVelocity uses it (insert-if-absent, find, empty, clear), kept as a
// sorted flat vector: same semantics, no node allocations per frame
struct IdMap {
  std::vector<std::pair<int, P2f>> v;
  bool empty() const { return v.empty(); }
  void clear() { v.clear(); }
  void swap(IdMap& o) { v.swap(o.v); }
  void build(const std::vector<int>& ids, const std::vector<P2f>& pts) {
    v.clear();
    v.reserve(ids.size());
    for (size_t i = 0; i < ids.size(); i++) v.emplace_back(ids[i], pts[i]);
    std::stable_sort(v.begin(), v.end(),
                     [](const std::pair<int, P2f>& a, const std::pair<int, P2f>& b) { return a.first < b.first; });
    // map::insert keeps the first element of equal keys
    v.erase(std::unique(v.begin(), v.end(),
                        [](const std::pair<int, P2f>& a, const std::pair<int, P2f>& b) { return a.first == b.first; }),
            v.end());
  }
  const P2f* find(int id) const {
    auto it = std::lower_bound(v.begin(), v.end(), id,
                               [](const std::pair<int, P2f>& a, int k) { return a.first < k; });
    return (it != v.end() && it->first == id) ? &it->second : nullptr;
  }
};

const char* const kKernelNames[K_COUNT] = {
    "k_tile_hist", "k_tile_scan", "k_tile_scatter", "k_tile_apply", "k_sae_keys", "k_radix_pass", "k_sae_apply",
    "k_time_surface4", "k_time_surface", "k_median", "k_clahe", "k_norm_pyr", "k_pyr3", "k_pyr_down", "k_pyr_pad",
    "k_scharr", "k_pad_scharr", "k_lk_f32", "k_lk", "k_arc_map", "k_arc_ev", "k_dedup", "k_compact", "k_select_mw",
    "k_select", "k_select_gbm", "k_fast_score", "k_fast_collect", "k_events_from_fields", "k_baf_heads", "k_baf_filter",
    "k_baf_count", "k_baf_scan", "k_baf_emit", "k_baf_keys_fields", "k_baf_emit_fields", "k_raw_reduce", "k_raw_scan",
    "k_raw_emit", "k_slice_reduce", "k_slice_scan", "k_slice_cuts", "k_baf_keys_addr", "k_hot_count", "k_hot_keys",
    "k_hot_pick", "k_trig_reduce", "k_trig_emit"};
// the ingest range behind the stage table (IngestKernelId, fe_kernels.h): esvio_fe_ingest_kernel_count()
const char* const kIngestKernelNames[K_INGEST_COUNT - K_COUNT] = {"k_aedat_count", "k_aedat_scan", "k_aedat_emit", "k_bag_emit", "k_image_emit"};

// The host phases of one trackEvent call, in the order of esvio_fe_latency_call::phase_ms; kPhaseNames is what
// esvio_fe_latency_phase_name returns and what the ESVIO_FE_TRACE summary prints.  The PH_PUB_* phases are parts of
// PH_MASK_DETECT on published frames, PH_STAGE_HOST is part of PH_ENQ_BATCH.
enum Phase {
  PH_ENQ_BATCH, PH_ENQ_TEMPORAL, PH_WAIT_TEMPORAL, PH_FILTER, PH_RANSAC, PH_MASK_DETECT, PH_WAIT_STEREO, PH_TAIL,
  PH_PUB_SETMASK, PH_PUB_SELECT, PH_PUB_SPEC, PH_PUB_PREV_RIGHT, PH_PUB_STEREO_NEW, PH_PUB_PREFETCH,
  PH_CHECK, PH_STAGE_HOST, PH_COUNT
};
static_assert(PH_COUNT == ESVIO_FE_LATENCY_PHASES, "one enumerator per public latency phase");
const char* const kPhaseNames[PH_COUNT] = {
    "enqueue sae+ts+pyr", "enqueue temporal LK", "wait temporal LK", "host filter", "host ransac",
    "host mask + enqueue detect/stereo", "wait stereo LK", "host tail",
    "pub: Event_setMask", "pub: points + k_select launch", "pub: speculative + chained LK launches",
    "pub: previous frame's right tail", "pub: stereo LK of new corners launch", "pub: next batch's prefetch launches",
    "check + take-up of a late batch", "sae: staging the host batch (part of enqueue sae+ts+pyr)"};

// the stopwatch behind every phase: lap() = the milliseconds since the last lap (or the construction)
struct PhaseClock {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double lap() {
    const auto now = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    return ms;
  }
};

// the event images' two timer slots behind the ingest range: esvio_fe_event_image_kernel_stats reads them, the stage
// and ingest tables (whose ends tests pin) stay as they are
// ... and behind them the keyframe stage's three (esvio_fe_kf_kernel_count / _name / _stats, include/esvio_fe_test.h)
// ... and behind those loop detection's four (esvio_fe_bow_kernel_count / _name / _stats)
// ... and behind those the AEDAT frames' one, k_frame16_emit (esvio_fe_aedat_frame_kernel_stats)
// ... and behind that vocabulary creation's (esvio_fe_bow_create_kernel_count / _name / _stats)
// ... and behind those the text stage's three (esvio_fe_text_kernel_count / _name / _stats)
enum { K_EVIMG_MARK = K_INGEST_COUNT, K_EVIMG_EMIT, K_KF_BLUR, K_KF_BRIEF, K_KF_MATCH, K_BOW_WALK, K_BOW_VECTOR, K_BOW_SCORE,
       K_BOW_SELECT, K_FRAME16_EMIT, K_VOC_FIRST, K_VOC_MINDIST, K_VOC_SCAN_REDUCE, K_VOC_SCAN_TOP, K_VOC_SCAN_DOWN, K_VOC_DRAW,
       K_VOC_PICK, K_VOC_ASSIGN, K_VOC_COUNT_BIG, K_VOC_MEAN_BIG, K_VOC_MEAN_SMALL, K_VOC_CHILD_COUNT, K_VOC_REGROUP_KEYS,
       K_VOC_DOC_COUNT, K_TEXT_COUNT, K_TEXT_PLACE, K_TEXT_EMIT, K_ALL_COUNT };
constexpr int kKfKernels = K_BOW_WALK - K_KF_BLUR;
const char* const kKfKernelNames[kKfKernels] = {"k_kf_blur", "k_kf_brief", "k_kf_match"};
constexpr int kBowKernels = K_FRAME16_EMIT - K_BOW_WALK;
const char* const kBowKernelNames[kBowKernels] = {"k_bow_walk", "k_bow_vector", "k_bow_score", "k_bow_select"};
constexpr int kVocKernels = K_TEXT_COUNT - K_VOC_FIRST;
const char* const kVocKernelNames[kVocKernels] = {
    "k_voc_first", "k_voc_mindist", "k_voc_scan_reduce", "k_voc_scan_top", "k_voc_scan_down", "k_voc_draw", "k_voc_pick",
    "k_voc_assign", "k_voc_count_big", "k_voc_mean_big", "k_voc_mean_small", "k_voc_child_count", "k_voc_regroup_keys",
    "k_voc_doc_count"};
constexpr int kTextKernels = K_ALL_COUNT - K_TEXT_COUNT;
const char* const kTextKernelNames[kTextKernels] = {"k_text_count", "k_text_place", "k_text_emit"};

struct KStat {
  double ms = 0;
  uint64_t launches = 0;
  uint64_t bytes = 0;
};

struct ProfRec {
  int id;
  Event a, b;
  uint64_t bytes;
};

// buildOpticalFlowPyramid's level count [OpenCV video/lkpyramid.cpp]
inline int pyr_levels(int w, int h, int win, int max_level) {
  int sw = w, sh = h;
  for (int level = 0; level <= max_level; ++level) {
    sw = (sw + 1) / 2;
    sh = (sh + 1) / 2;
    if (sw <= win || sh <= win) return level;
  }
  return max_level;
}

// esvio_fe_set_next_batch: a batch announced ahead of its trackEvent call ...
struct Batch {
  const esvio_fe_event *left = nullptr, *right = nullptr;
  size_t nL = 0, nR = 0;
  int space = 0;
  double time = 0;
  int pub = 0;  // caller's PUB_THIS_FRAME hint
  int stage = -1;  // host events: the staging slot they travel through (fe_evstage.cpp), -1: none
  bool has_motion = false;  // esvio_fe_set_next_batch_mc: the motion-compensated overload
  esvio_fe_motion motion{};
};
// ... and, once its SAE update / images / pyramids (/ Arc*) are enqueued on the prefetch stream,
// the resources they were given
struct Inflight : Batch {
  int lane = 0;  // staging buffer + event pair
  int slotL = 0, slotR = 0, raw = 0, cand = 0;
  const EventRec *dL = nullptr, *dR = nullptr;
  bool arc_done = false;
  uint32_t gate = 0;  // != 0: the value the batch's prefetch sequence leaves in d_lane_gate[lane] (issued by the launch thread)
  // event images that follow announced batches: the set the batch's prefetch sequence rewrites (-1: none), and the
  // cameras of that set whose last write was made on another stream than the prefetch stream (their `written` events
  // are waited for first)
  int evset = -1, ev_wait = 0;
};
constexpr int kPrefetchDepth = 3;
// host-event staging slots: one per batch the handle can know about at a time (2 * kPrefetchDepth
// announced or prefetched and not yet tracked, the one being tracked, one spare)
constexpr int kStageSlots = 2 * kPrefetchDepth + 2;
struct EventStager;  // fe_evstage.cpp
struct Launcher;     // fe_track.cpp: the thread that issues announced batches' prefetch sequences
constexpr int kLeftSlots = 2 + kPrefetchDepth;   // prev, cur, prefetched...
constexpr int kRightSlots = 1 + kPrefetchDepth;  // cur, prefetched...

struct PyrStore {
  PyrDesc d{};
  DevBuf<uint8_t> mem;
  int w = 0, h = 0, max_level = -1;
};

}  // namespace fe
}  // namespace esvio
using namespace esvio::fe;

// Every device buffer, pinned block, event and stream below is a member that releases itself (fe_res.h).  The
// members' destruction order — the reverse of their declaration — carries no dependency: esvio_fe_destroy deletes the
// handle only after its threads have stopped and every stream is idle, and the one step that has an order (the
// RCCL communicator before the stream it runs on) is written out there.  Pointers INTO a block (the views of
// d_res, h_pin and h_spec, fe_layout.h) stay raw: only the block is owned.
struct esvio_fe_ctx {
  esvio_fe_config cfg{};
  int dev = 0;
  Stream stream;   // main stream
  Stream stream2;  // prefetch stream (next batch's SAE update / images)
  Stream stream3;  // speculative temporal LK of the next frame
  // stereo LK of the temporal survivors: nothing on the frame's chain reads its results before the
  // right-camera tail, and on the main stream it would hold up the corner selection behind it
  Stream stream4;
  // ... of an UNPUBLISHED frame (stereo_stream() below).  The chained temporal LK of the frame after next sits on
  // stream4 from the published call that launched it until its last point is done; the unpublished frame's stereo
  // LK queued behind it, the next published frame's behind that, and the published call waited 35-45 us for its
  // stereo results at its end (and 10-55 for the previous frame's): with the unpublished frame's launch on a stream
  // of its own both waits are gone — cycle 272 -> 246 us in the trace, 0.131 -> 0.119 ms/step.  (WHICH launches
  // share a stream matters more than how many streams there are: the published frame's stereo LK and the chained
  // launch on the new stream instead — `k_select_mw` 17 -> 40 us, cycle 300 us; KERNELS.md.)
  Stream stream6;
  std::vector<double> pre_lx, pre_ly;  // prev_pts lifted through the left camera model under the temporal LK's wait
  bool pre_lift_valid = false;
  bool stereo_unpub = false;  // the frame being tracked publishes nothing (and stereo_split is on)
  // -1: lk_accum == 2 && launch thread on (decided per call); 0 / 1: ESVIO_FE_STEREO_SPLIT
  int stereo_split_env = -1;
  bool stereo_split = false;
  int n_queue_conflicts = 0;  // pairs of the handle's streams found on one hardware queue (ESVIO_FE_QUEUE_PROBE)
  Event ev_planes_free;
  // a plain (not announced) call: the frame's images are built (main stream) -> its Arc* pass on the
  // prefetch stream and its stereo LK on stream4 start beside the temporal LK; the Arc* pass is done
  Event ev_imgs_ready, ev_arc_side;
  // ... split by camera: the left camera's update + image on the main stream (ev_imgs_ready: the LEFT image
  // then), the right camera's behind it on the stereo stream — behind ev_sae_left (the one partition
  // scratch) and, for a batch in pageable memory, behind the right array's own DMA; ev_right_ready: done
  Event ev_sae_left, ev_right_ready;
  Event ev_pts_ready, ev_spec_done, ev_sel_host;
  std::string err;
  int W = 0, H = 0;
  uint32_t P = 0;
  int key_bits = 0;
  uint32_t invalid_key = 0;
  std::vector<int> hw;  // disc half-widths for min_dist

  // ---- device state
  DevBuf<double2> L2;  // [2P] {L[0],L[1]} per (cam,pixel)
  DevBuf<double2> S2;  // [2P] {S[0],S[1]}
  DevBuf<EventRec> d_ev;
  DevBuf<uint32_t> keys[2], vals[2], hist;
  size_t sort_cap = 0;  // of keys, vals and sae_marks (ensure_sort_capacity)
  size_t sae_ev_min = (size_t)1 << 20;  // batches of at least this many events: k_sae_apply_ev
  // tiled SAE update (default; ESVIO_FE_SAE_SORT=1 or a sensor too large for one digit: the radix
  // sort form above)
  bool tiled = false;
  TileGeom tgeom{};
  DevBuf<EventRec> d_part;  // the batch's events partitioned by bucket
  DevBuf<uint32_t> d_warp;  // [d_part.cap] motion compensation: the pixel each event is warped to
  DevBuf<uint32_t> d_tile;  // TileScratch
  DevBuf<uint8_t> sae_marks;         // [sort_cap] its per-event "stores L / stores S" marks
  DevBuf<unsigned long long> d_rejected;
  // left: slots 0..kLeftSlots-1 rotate (prev, cur, up to kPrefetchDepth being prefetched);
  // right: the kRightSlots after them (cur + prefetched)
  PyrStore pyr[kLeftSlots + kRightSlots];
  int slot_prevL = 0, slot_curL = 0, slot_curR = kLeftSlots;
  bool have_img = false;
  bool ext_right_pending = false;  // esvio_fe_import_image(cam=1) done for the next frame
  // time-sliced stream (esvio_fe_sae_slice_*): scratch planes a slice is applied to, and the one-shot
  // "the planes already hold the next frame's batch" set by esvio_fe_sae_slice_commit
  DevBuf<double2> L2s, S2s;
  DevBuf<double> slice_stage;  // device staging for host-side slice planes
  bool ext_sae_pending = false;
  // esvio_fe_exchange_tracks: send / receive buffers of the all-gather and the pinned pack area
  DevBuf<float> x_send, x_recv;
  PinBuf<float> x_pin, x_pin_recv;
  // esvio_fe_comm_init: the handle's own RCCL communicator, the side stream the asynchronous
  // exchange runs on and the event that marks its end
  void* x_comm = nullptr;
  int x_world = 0;
  Stream x_stream;
  Event x_done;
  bool x_pending = false;
  bool x_auto = false;      // esvio_fe_set_auto_exchange: every published frame's records are exchanged
  bool x_deferred = false;  // packed records waiting to be enqueued (by the next call, under its device wait)
  // ---- next-batch prefetch (esvio_fe_set_next_batch)
  std::deque<Batch> announced;     // announced, nothing enqueued yet (<= kPrefetchDepth)
  std::deque<Inflight> inflight;   // SAE update / images / pyramids enqueued on the prefetch stream
  bool cur_prefetched = false;     // the frame being processed came from the prefetch stream
  EventStager* stager = nullptr;  // host-resident batches: pinned chunks + DMA by helper threads
  // chunks queued in the stager right now; lives here (not in the stager) because the RANSAC helpers poll
  // it while they spin, and the handle outlives both
  std::atomic<int> stage_pending{0};
  int cur_stage = -1;             // staging slot of the batch being tracked
  int stage_threads = 0;          // helper threads of the stager (0: off)
  // esvio_fe_set_launch_thread: the HIP calls of an announced batch's prefetch sequence (~10 launches and
  // event calls, 35-45 us of host time per batch) are issued by a thread of the handle; the calling
  // thread only does the bookkeeping and, before it consumes a lane, checks that its job has been issued
  Launcher* launcher = nullptr;
  uint64_t lane_job[kPrefetchDepth] = {};  // job number that (re)records the lane's events
  int launch_err = 0;  // a launch-thread job failed and the thread has been stopped since: sticky until esvio_fe_reset
  uint64_t lks_wait_job[2] = {};  // latest job whose prefetch sequence waits on ev_lks_done[set] (record_lks_done)
  // bounds of the device-side waits handed to the launches; esvio_fe_debug_inject / ESVIO_FE_FAULT set
  // chosen ones to 0 (the wait expires the first time it would have to wait)
  struct WaitLimits {
    uint32_t lookback = kSpinLookback, ticket = kSpinTicket;
    unsigned long long poll = kTicksPoll, chain = kTicksChain;
  } lim;
  bool lazy_late = false;  // ESVIO_FE_FAULT_LAZY_LATE (test): the lazy completions always at their latest point
  uint64_t n_spec_expired = 0, n_chain_expired = 0;  // speculative / chained temporal LK launches redone
  DevBuf<EventRec> d_evp[kPrefetchDepth];  // host-event staging, one per prefetch lane (stager off)
  Event ev_lane_done[kPrefetchDepth], ev_lane_arc[kPrefetchDepth];
  PyrStore tmp_pyr[2];  // standalone LK / pyramid taps on arbitrary host images
  PyrStore med_tmp[2];  // median_blur_kernel_size > 0: the surfaces before cv::medianBlur
  // equalize: raw time surfaces (single padded level each, left/right) + CLAHE scratch
  PyrStore raw[kRightSlots][2];  // [buffer][cam], rotating like the right pyramids
  int raw_cur = 0;
  DevBuf<uint8_t> d_lut;
  DevBuf<int> d_minmax;
  // device-side point / status buffers of the standalone entry points (LK, featuresToTrack) and the
  // selection counters; one allocation with the layout of ResLayout (dres: its view, no mask area)
  DevBuf<uint8_t> d_res;
  ResView dres{};
  DevBuf<float2> d_ptsD;
  // The per-frame path works on the pinned host block itself (device-visible): the LK kernels read
  // their points from it and write results into it, k_select mirrors its counters into it — no
  // H2D / D2H copy calls on the frame's critical path (each costs more host time than the few
  // hundred bytes take over PCIe).  pin[s] / hspec[b] = the host's views of h_pin (by copy of set 1) and of
  // h_spec (by block), zpin[s] / zspec[b] = the same regions at their device-side addresses; built once, at create.
  ResView pin[2] = {}, zpin[2] = {};
  SpecView hspec[kSpecBlocks] = {}, zspec[kSpecBlocks] = {};
  int res_set = 0;  // which copy of set 1 the current frame works in
  int lks_last = -1;  // copy the latest stereo LK launch (stream4) writes to, -1: none so far
  // ---- speculative temporal LK of the next frame (replay mode): once this frame's kept points
  // and new corners are final, next frame's calcOpticalFlowPyrLK(cur -> next) pair is launched on
  // stream3 against the prefetched pyramids, so it overlaps this frame's stereo LK and host tail
  PinBuf<uint8_t> h_spec;  // pinned, device-visible: [ptsB | ptsC | stA | stB | wait-expired flag] of that launch (SpecLayout)
  bool spec_valid = false;
  int spec_n = 0;             // number of points of that launch (= the next frame's prev_pts.size())
  // ---- chained temporal LK of the frame after next: when the next frame publishes nothing, the
  // frame after it tracks exactly the next frame's forward results, point by point, so its launch
  // (stream4) is made together with the speculative one and each of its waves starts the moment the
  // producer's wave of the same index publishes its forward result (LkArgs::chain_*).  Results:
  // second block of h_spec, indexed like the producer's points; the intermediate frame's temporal
  // filter gives the map from the final frame's prev_pts to those indices.
  DevBuf<unsigned long long> d_chain;  // [2 * max_cnt] published forward results
  // one word per prefetch lane: the serial number of the last prefetch sequence that has RUN there (LkArgs::gate_*)
  DevBuf<uint32_t> d_lane_gate;
  uint32_t gate_seq = 0;
  // LK launches whose waves WAIT on the device for another kernel's results (the speculative temporal launch for
  // k_select's corners, a chained launch for its producer's points) hold their CU while they wait — in the float-order
  // mode one workgroup of four points per CU.  If the waiting workgroups can fill the device, the kernel they wait for
  // may find no CU: with max_cnt 1000 (250 workgroups per launch on 256 CUs) one step in ~20 ran into the wait's 20-40 ms
  // bound and was redone (correct, but 40 ms).  So: a speculative launch only if one launch's workgroups leave two CUs
  // free (k_select_mw's up to 160 KB of LDS need a CU without an LK workgroup), a chained one (two waiting launches at
  // once) only if two do.  (max_cnt <= 1016 / <= 508 on MI355X's 256 CUs.)
  int n_cu = 0;
  bool waits_fit_spec = true, waits_fit_chain = true;
  uint32_t chain_seq = 0;
  bool chain_enabled = true;   // (ESVIO_FE_NO_CHAIN=1 turns it off: A/B measurements)
  bool cam_split_enabled = true;  // a plain call runs the two cameras' updates on two streams (ESVIO_FE_NO_CAMSPLIT=1: one)
  uint64_t n_plain_calls = 0, n_cam_split = 0, n_stereo_chained = 0;  // esvio_fe_plain_call_counters
  bool chain_valid = false;    // a chained launch has been made ...
  uint64_t chain_for = 0;      // ... for the frame with this number
  bool chain_map_ok = false;
  std::vector<int> chain_map;  // final frame's prev_pts[j] = producer point chain_map[j]
  uint64_t frame_no = 0;       // trackEvent calls so far
  Event ev_chain_done;
  // k_select publishes each new corner as it accepts it; the speculative launch, already resident,
  // picks them up one by one instead of starting after the whole selection
  DevBuf<unsigned long long> d_pub_slots, d_pub_done;
  uint32_t pub_seq = 0;
  // ---- lazy stereo of new corners (esvio_fe_set_lazy_new_stereo): a published frame returns
  // without waiting for the stereo LK of the corners it has just detected; their right-camera
  // entries are appended by the next call (before anything reads them) or by esvio_fe_finish
  bool lazy_new = false;
  struct PendingNew {
    bool active = false;
    bool prev_map_was_empty = false;
    std::vector<int> ids;       // the new corners' ids
    std::vector<P2f> left;      // ... and left positions
  } pend;
  // ... and a frame that publishes nothing returns without waiting for its stereo LK at all: the
  // whole right-camera tail (:475-575) is run by the next call, in the shadow of its own kernels,
  // or by esvio_fe_finish.  The next frame works in the other copy of set 1 meanwhile.
  struct PendingRight {
    bool active = false;
    int set = 0;                // copy of set 1 that holds this frame's stereo LK results
    double dt = 0;              // cur_time - prev_time of that frame
    std::vector<int> ids;       // the frame's ids / left points (no new corners: nothing published)
    std::vector<P2f> left;
  } pend_right;
  Event ev_lks_done[2], ev_lknew_done;
  host::RansacPool* pool = nullptr;  // esvio_fe_set_host_threads
  // arc / select
  DevBuf<uint8_t> d_flags;
  // per-block ordered candidate lists written by k_arc; two sets so that the Arc* of a prefetched
  // batch (prefetch stream) never overwrites the set the current frame's selection still reads
  struct CandSet {
    DevBuf<uint32_t> xy, idx, cnt;
    // ... and their ordered compaction into one stream (compact_set, right behind the kernel that filled them)
    DevBuf<uint32_t> comp_xy, comp_idx, total, grp;
    size_t cap = 0;  // of the set (grow_cand_set)
  } cand[kRightSlots];
  // per-pixel earliest candidate of a set's latest Arc* pass (ArcArgs::first_map / launch_dedup)
  DevBuf<uint32_t> d_first[kRightSlots];
  // per-pixel, per-polarity result of the event-independent part of isCorner (k_arc_map), one map
  // per candidate set
  DevBuf<uint32_t> d_cmap[kRightSlots];
  DevBuf<uint8_t> d_touched[kRightSlots];  // (pixel, polarity) pairs a batch's left events hit
  uint32_t first_epoch[kRightSlots] = {};  // Arc* passes into the set so far
  bool dedup_enabled = true;               // (ESVIO_FE_NO_DEDUP=1, test-only: the path batches >= 2^20 events take)
  bool fuse_ts_pyr = true;                 // (ESVIO_FE_NO_FUSE=1, test-only: k_time_surface + 3 x k_pyr_down, the median / equalize path)
  int cand_cur = 0;
  DevBuf<uint32_t> d_mask_bits;
  // goodFeaturesToTrack scratch (image front-end), allocated on first use
  DevBuf<float4> d_gftt_cov, d_gftt_rowsum;
  DevBuf<float> d_gftt_eig;
  DevBuf<uint32_t> d_gftt_max;
  DevBuf<int32_t> d_sel_idx;
  DevBuf<uint8_t> d_fast_img;  // esvio_fe_fast_corners: a caller's host image (linear, width*height); its lists: fast_own below
  // pinned host staging (h_pin's layout: ResLayout)
  PinBuf<uint8_t> h_img;  // copy_level0_in's staging ring: pinned host side ...
  DevBuf<uint8_t> d_img;  // ... and its device side (linear images)
  unsigned img_stage_next = 0;
  PinBuf<uint8_t> h_pin;

  // ---- FeatureTracker state (feature_tracker.h:119-173)
  int n_id = 0;
  double cur_time = 0, prev_time = 0;
  std::vector<P2f> prev_pts, cur_pts, cur_right_pts, n_pts;
  std::vector<P2f> cur_un_pts, cur_un_right_pts, pts_velocity, right_pts_velocity;
  std::vector<int> ids, ids_right, track_cnt, track_cnt_right;
  std::vector<int> src_idx;  // per cur_pts entry: index into the speculative stereo-LK results
  IdMap cur_un_pts_map, prev_un_pts_map, cur_un_right_pts_map, prev_un_right_pts_map;
  host::BitMask mask_event;

  // ---- host phase trace (ESVIO_FE_TRACE=1): the sums of the successful calls' latency records, and what is finer
  DevBuf<uint8_t> d_eq_tmp;  // equalize: the two CLAHE outputs before normalisation (linear W x H each)
  bool select_ok = true;  // the greedy selection's bitmap fits LDS
  bool select_one_wave = false;  // (ESVIO_FE_SELECT_SERIAL=1, test-only: the one-wave selection kernel)
  DevBuf<uint32_t> d_sel_bitmap;  // ... else it lives here (k_select_gbm)
  bool trace = false;
  double trace_phase_ms[2][ESVIO_FE_LATENCY_PHASES] = {};  // [published?][Phase]: lat.cur_phase of every successful call
  double tail_ms[2][4] = {};   // [published?]: left bookkeeping, previous frames' right tails, this frame's right tail, the rest
  uint64_t phase_count[2] = {0, 0};
  uint64_t phase_frames = 0, tr_cand = 0, tr_new = 0, tr_detect = 0, tr_surv = 0;
  uint64_t tr_fm_class[3] = {};  // rejectWithF_event calls with < 8 points (skipped), 8..14 (LMedS), >= 15 (RANSAC)
  double tr_fm_ms = 0;  // time inside find_fundamental_mat alone
  double tr_fm_max_ms = 0, tr_lift_ms = 0;  // ... its slowest call; the two liftProjective batches
  uint64_t tr_chain_launch = 0, tr_chain_used = 0, tr_chain_cancel = 0, tr_spec_used = 0;
  // (trace only) device-side intervals of the published frame's chain, from timing events
  Event ev_dbg_sel_start;
  double tr_gpu_sel = 0, tr_gpu_spec = 0, tr_gpu_chain = 0, tr_host_chain = 0, tr_gpu_pyr = 0;
  int tr_lane = -1;  // prefetch lane of the frame being tracked
  uint64_t tr_gpu_n = 0;
  std::chrono::steady_clock::time_point tr_sel_launch;

  // ---- per-call latency record (esvio_fe_latency_stats; always on)
  struct Latency {
    static constexpr int kRing = 4096;
    float ring[kRing] = {};
    uint64_t calls = 0;
    double sum_ms = 0, max_ms = 0;
    uint64_t max_call = 0;
    int max_pub = 0, max_cpu0 = -1, max_cpu1 = -1;
    long max_nivcsw = 0, max_allocs = 0;
    double max_phase[ESVIO_FE_LATENCY_PHASES] = {};
    uint64_t allocs = 0, nivcsw = 0;
    double cur_phase[ESVIO_FE_LATENCY_PHASES] = {};  // the call in progress
    // the latest calls, whole (esvio_fe_latency_recent)
    static constexpr int kRecent = 256;
    esvio_fe_latency_call recent[kRecent] = {};
    uint64_t total_calls = 0;
    bool have_t0 = false;
    std::chrono::steady_clock::time_point t0;
  } lat;
  uint64_t n_allocs = 0;  // hipMalloc / hipHostMalloc calls of this handle so far
  double slow_call_ms = 0;  // ESVIO_FE_SLOW_CALL_MS: calls slower than this are reported on stderr (0: off)

  // ---- profiling
  bool prof_on = false;
  KStat stats[K_ALL_COUNT];
  std::vector<ProfRec> pending;
  std::vector<Event> ev_pool;

  // ---- event layouts (behind everything else: the members above lie where they lay before these existed)
  // esvio_fe_convert_events, allocated on first use: the field bytes of a host source that is not read in place, the
  // records behind a host destination, the bad-event count
  DevBuf<uint8_t> d_cvt_src;
  DevBuf<EventRec> d_cvt_out;
  DevBuf<unsigned long long> d_cvt_bad;
  int cvt_pinned_copy = -1;  // page-locked sources: -1 = the measured choice; ESVIO_FE_CONVERT_PINNED_COPY=1 / 0: always copied first / always read in place (the A/B in KERNELS.md)
  // esvio_fe_track_event_fields: two pairs of record buffers [pair][camera] that alternate, and per pair the events
  // that mark what its latest call left on stream2 / stream3 / stream4 / stream6 (include/esvio_fe.h: buffer lifetime)
  DevBuf<EventRec> d_cvt_ev[2][2];
  Event ev_cvt_side[2][4];
  bool cvt_side_rec[2] = {false, false};
  int cvt_pair = 0;

  // ---- esvio_fe_set_detector: where trackEvent's new corners come from.  ESVIO_FE_DETECT_FAST: a FAST pass over the
  // frame's raw left time surface fills the frame's candidate set instead of the Arc* pass over its left events
  // (run_fast_cand, fe_image.cpp).  A pass works in scratch of its own — the score map, the counts before the
  // TS_LK_threshold test (+ their sum), the unsorted pairs and the sort's scratch words — one per candidate set, so
  // that passes of batches in flight on different streams share nothing, none of it with esvio_fe_fast_corners; the
  // last one, with a candidate set of its own and a device copy of a caller's host image, is the stage tap's
  // (esvio_fe_features_to_track_fast).  Allocated by esvio_fe_set_detector(FAST) or the tap's first call.
  int detector = ESVIO_FE_DETECT_ARC, fast_barrier = 0;
  struct FastCand {
    DevBuf<uint8_t> m;
    DevBuf<uint32_t> det, tot, keys, vals, hist;
  } fastc[kRightSlots + 1];
  CandSet fast_tap;
  DevBuf<uint8_t> d_fast_tap_img;
  // esvio_fe_fast_corners' own (fast_run, fe_image.cpp), allocated by its first call: a candidate set of one entry per
  // pixel — the per-block lists, the compacted list it returns — and of a FastCand the score map and the counts
  // before non-max alone: it sorts nothing, so tot / keys / vals / hist stay empty.  The set's `total` has two words
  // here, {total, detected before non-max}: adjacent, so that one copy brings both to the host.
  CandSet fast_own;
  FastCand fast_own_fc;

  // ---- esvio_fe_filter_events: the background-activity filter of an event batch (include/esvio_fe.h has the rule,
  // fe_kernels.h the chain).  Everything is allocated by the first filtering call — a handle that never filters
  // holds none of it — and is the stage's own: the main stream is the only one that touches it.  B: the stamp plane
  // of each camera, [2][P] nanoseconds, -1 = none.  head: [P], the chain's per-pixel segment heads (never cleared).
  // Per event, for calls of up to `cap` events: the (key, index) pairs of the sort and its scratch words, the stamps in
  // sorted order (and in stream order: the fields form's, allocated by its first use), the flags, the per-block counts; shared by the two
  // cameras' chains in stream order, while each camera has a result block of its own.  src / out: a host source's records and the records behind a host
  // dst, on first use of either.  (esvio_fe_track_event_filtered filters into esvio_fe_track_event_fields' two pairs.)
  struct Baf {
    DevBuf<long long> B, tsort, tstream;
    DevBuf<uint32_t> head, keys[2], vals[2], sort, blk_cnt;
    DevBuf<uint8_t> flags;
    DevBuf<BafResult> res;  // [2]: one per camera, so that both cameras' chains are waited for once
    DevBuf<EventRec> src, out;
    size_t cap = 0;
  } baf;

  // ---- the address stage of the filter rule and hot-pixel learning (include/esvio_fe.h).  The address filter and the
  // pixel mask are SETTINGS (they survive esvio_fe_reset); the mask's words are allocated by the first call that sets
  // one.  hot: the count planes [2][P] and the per-camera state, allocated by the first learn / select, the host's
  // copy of each camera's state (taken over when a learn call returns), the selection's own scratch (main stream only).
  struct Addr {
    bool on[2] = {false, false};
    esvio_fe_address_filter f[2] = {};
    DevBuf<uint32_t> mask[2];
  } addr;
  struct Hot {
    DevBuf<uint32_t> C, keys[2], vals[2], sort, counts;
    DevBuf<uint16_t> xy;
    DevBuf<HotState> st;   // [2]
    DevBuf<HotResult> res;
    DevBuf<EventRec> src;  // the copy of a host source of records
    HotState h_st[2] = {};
  } hot;

  // ---- esvio_fe_decode_raw / esvio_fe_track_raw: raw sensor streams (include/esvio_fe.h has the rule, fe_kernels.h
  // the chain).  st: each camera's decoder state, kept on the HOST — it travels to the scan launch as an argument and
  // comes back in the camera's result block, which is the pending slot: the host takes it over only once the call is
  // known to succeed.  Everything else is allocated on first use and is the stage's own (main stream only), one per
  // camera so that both cameras' chains are in flight together: src, the copy of a host source that is not read in
  // place; sums, the tiles' transformers; dec, the records behind a host dst (esvio_fe_decode_triggers' 16-byte trigger
  // records too: every call has taken its records out before it returns) and, in esvio_fe_track_raw with a filter,
  // the decoded records the filter reads; res, the two result blocks.
  struct Raw {
    struct State {
      uint32_t seen = 0, th = 0, tl = 0, y = 0, bx = 0, bp = 0;
      uint64_t wraps = 0;
    } st[2];
    State trig_st[2];  // esvio_fe_decode_triggers' own decoder states (seen, th, wraps, tl; the rest stays 0)
    DevBuf<uint8_t> src[2];
    DevBuf<RawXf> sums[2];
    DevBuf<EventRec> dec[2];
    DevBuf<RawResult> res;
    bool used = false;     // esvio_fe_reserve grows the scratch of a handle that has decoded before
    int pinned_copy = -1;  // page-locked sources: -1 = in place up to kRawPinnedInPlaceBytes (fe_api.cpp); ESVIO_FE_RAW_PINNED_COPY=1 / 0: always copied first / always in place
  } rawdec;

  // ---- esvio_fe_decode_aedat / esvio_fe_aedat_side / esvio_fe_track_aedat: libcaer packet streams (include/esvio_fe.h
  // has the rule, fe_aedat.h the host walk, fe_kernels.h the chain).  ev_st / side_st: each camera's two walker states
  // (frame_st: the third, below), on the HOST: a call walks a copy and takes it over only once it is known to succeed.
  // Per camera, allocated on first use and the stage's own (main stream only): h_pack, the pinned scratch the walk
  // gathers into — the packed polarity records, the run table behind them at a 16-byte boundary —, d_pack its device
  // copy (one transfer), sums the tiles' counts; res, the two result blocks.  The records behind a host dst, and in
  // front of a filter, are rawdec.dec's.
  struct Aedat {
    esvio::aedat::Walk ev_st[2] = {}, side_st[2] = {};
    PinBuf<uint8_t> h_pack[2];
    DevBuf<uint8_t> d_pack[2];
    DevBuf<uint32_t> sums[2];
    DevBuf<AedatResult> res;
    bool used = false;  // esvio_fe_reserve grows the scratch of a handle that has decoded AEDAT before
    // esvio_fe_decode_aedat_frames / esvio_fe_convert_frame16 ("AEDAT 3.1 frames").  frame_st: each camera's third walker
    // state, carry the pixel bytes of the frame a call's end cut (fe_aedat.h: Carry), both on the HOST and taken over as
    // the others are.  The stage's own, main stream only, allocated on first use: h_frm, the pinned scratch the walk
    // gathers the frames' pixel bytes into, each frame from a 16-byte boundary, the descriptor table behind them; d_frm
    // its device copy (one transfer); d_gray the images behind a host dst.
    esvio::aedat::Walk frame_st[2] = {};
    esvio::aedat::Carry carry[2];
    PinBuf<uint8_t> h_frm;
    DevBuf<uint8_t> d_frm, d_gray;
    bool frm_used = false;  // esvio_fe_reserve grows the scratch of a handle that has decoded frames before
  } aedat;

  // ---- esvio_fe_decode_bag / esvio_fe_bag_side / esvio_fe_feed_push_bag: rosbag v2.0 recordings (include/esvio_fe.h has
  // the rule, fe_bag.h the host walk, fe_kernels.h the kernel).  topics: esvio_fe_bag_set_topics' copies.  ev_st /
  // side_st: the handle's two walker states, on the HOST: a call walks a copy and takes it over only once it is known
  // to succeed.  Allocated on first use and the stage's own (main stream only): h_pack, the pinned scratch the walk
  // gathers into — the left camera's wire events, the right camera's behind them at a 16-byte boundary —, d_pack its
  // device copy (one transfer); res, the two result blocks.  The records behind a host dst,
  // and on their way into the feed, are rawdec.dec's.
  struct Bag {
    esvio::bag::Topics topics;
    esvio::bag::Walk ev_st = {}, side_st = {};
    PinBuf<uint8_t> h_pack;
    DevBuf<uint8_t> d_pack;
    DevBuf<BagResult> res;
    bool used = false;   // esvio_fe_reserve grows the scratch of a handle that has decoded a bag before
    // esvio_fe_decode_bag_images / esvio_fe_convert_image.  img_st: the third walker state, carry the bytes of the payload
    // a call's end cut (fe_bag.h: Carry), both on the HOST and taken over as the others are.  The stage's own, main
    // stream only, allocated on first use: h_img, the pinned scratch the walk gathers the payloads into, each from a
    // 16-byte boundary, the descriptor table behind them; d_img its device copy (one transfer); d_gray the images behind
    // a host dst.
    esvio::bag::Walk img_st = {};
    esvio::bag::Carry carry;
    PinBuf<uint8_t> h_img;
    DevBuf<uint8_t> d_img, d_gray;
    bool img_used = false;    // esvio_fe_reserve grows the scratch of a handle that has decoded images before
  } bag;

  // ---- esvio_fe_decode_text / esvio_fe_track_text / esvio_fe_feed_push_text: text event files (include/esvio_fe.h has
  // the rule, fe_text.h the classifier and the carry step, fe_kernels.h the chain).  st: each camera's state — the
  // unterminated tail, or "inside an overlong line" — on the HOST: it travels to the launches as an argument; the state
  // behind a call comes from the carry step for a host chunk and from the camera's result block for a device chunk, and
  // is taken over only once the call is known to succeed.  Allocated on first use and the stage's own (main stream
  // only), one per camera: src, the copy of a host source that is not read in place; sums, the tiles' counts; res, the
  // two result blocks.  The records behind a host dst, and in front of a filter, are rawdec.dec's.
  struct Text {
    esvio::text::State st[2];
    DevBuf<uint8_t> src[2];
    DevBuf<TextTile> sums[2];
    DevBuf<TextResult> res;
    bool used = false;  // esvio_fe_reserve grows the scratch of a handle that has decoded text before
  } text;

  // ---- esvio_fe_slice_events: a record stream cut into fixed-rate windows (include/esvio_fe.h has the rule,
  // fe_kernels.h the chain).  st: each camera's state, kept on the HOST like the decoder's: the device works on counts
  // relative to it and the host takes a call's result over only once the call is known to succeed.  E: the boundaries
  // E_{tb} .. of the camera's chain as the host computed them (a cache: tagged with the frequency and origin it was made
  // for), bounds their toSec() on the device.  Everything is allocated on first use and is the stage's own (main stream
  // only): src, the copy of a host source; tmax, the tiles' maxima; res, per camera the result block with the cut
  // entries behind it; h_res, where they arrive.
  struct Slice {
    struct State {
      bool seen = false;
      bool at = false;  // seen: the camera's windows end at stamps the caller gives (esvio_fe_slice_events_at), not at fixed rate
      int32_t has_origin = 0;
      double frequency = 0;
      uint32_t o_sec = 0, o_nsec = 0;  // the origin record's stamp
      uint64_t m = 0, open = 0;        // windows closed so far; events in the open one
    } st[2];
    struct Bound {
      uint64_t sec;  // (may leave 32 bits: such an entry ends the table)
      uint32_t nsec;
    };
    std::vector<Bound> E[2];
    uint64_t tb[2] = {0, 0};
    State tab_for[2];  // frequency / origin the table was computed for (seen == false: none)
    DevBuf<double> bounds[2];
    PinBuf<double> h_bounds[2];
    DevBuf<EventRec> src[2];
    DevBuf<uint32_t> tmax[2];
    DevBuf<uint32_t> res;   // [2][kSliceResWords]
    PinBuf<uint32_t> h_res; // [2][kSliceResWords]
  } slice;

  // ---- esvio_fe_feed_*: chunks in, windows tracked where they lie (include/esvio_fe.h).  Per camera two buffers;
  // `cur` holds records [pos0, pos0 + len) of the camera's stream (positions count the records appended since the feed
  // was opened or emptied), of which everything from the oldest untracked window's start on is still needed.  read_ev:
  // per buffer the events recorded on the side streams when the last track call that read it returned.
  struct Feed {
    bool open = false, has_filter = false, origin_known = false;
    esvio_fe_slice_params prm{};
    esvio_fe_filter_params filter{};
    struct Window {
      uint64_t index, begin, end;  // [begin, end): positions in the camera's stream
      uint32_t sec, nsec;          // E_index
    };
    struct Cam {
      DevBuf<EventRec> buf[2];
      Event read_ev[2][4];
      bool read_rec[2] = {false, false};
      bool rewound = false;  // emptied without idle streams: the next append waits for read_ev[cur] first
      int cur = 0;
      uint64_t pos0 = 0, len = 0, open_begin = 0;
      std::deque<Window> win;
    } cam[2];
    std::vector<uint64_t> cuts;
  } feed;

  // ---- esvio_fe_set_event_images: detector.cur_event_mat_left/right (include/esvio_fe.h has the rule, fe_kernels.h the
  // chain).  A SETTING (it survives esvio_fe_reset).  Everything is pixel-proportional and allocated by set(1), released
  // by set(0): per camera the mark plane (one word per pixel) and the image (3 bytes per pixel), both padded to `groups`
  // groups of four pixels, and the canvas scratch of the getter.  fresh_cams: the cameras whose image the running TRACK
  // call rewrites (set by take_batch, cleared as the camera's emit is enqueued); 0 in a stage call: accumulate.
  // written[cam]: recorded behind every write to the camera's image on wstream[cam], whichever stream made it; the
  // getters wait for it and copy on none of the handle's streams.
  // ESVIO_FE_EVENT_IMAGES_AHEAD (mode 2): kSets image sets instead of one — the frame being tracked's (`cur`) and one per
  // prefetch lane — all allocated by set(2).  A set is what ONE batch writes: an announced batch is given a set that is
  // neither `cur` nor another prefetched batch's with its other resources (prefetch_next; Inflight::evset), its
  // prefetch sequence rewrites both cameras of that set on the prefetch stream, and take_batch makes the set `cur`.
  // The mark planes are kept PER SET, not shared: a set's marks and bytes are then touched by its batch's launches
  // alone, and the one order to keep is between a set's successive owners (written[] / wstream[]) — shared planes
  // would have to be ordered between the prefetch stream and a plain call's main and stereo streams as well.  Mode 2
  // therefore holds kSets x 2 x (4 + 3) + 6 = 62 bytes per pixel, mode 1 its 20.
  // fresh_cams, and the wstream[] of every set, are the CALLING thread's: the launch thread is told what to do by its
  // job (Inflight::evset, ::ev_wait) and touches only the set's device memory and its two events.
  struct Evimg {
    static constexpr int kSets = kPrefetchDepth + 1;
    struct Set {
      DevBuf<uint32_t> marks[2], img[2];
      Event written[2];
      hipStream_t wstream[2] = {nullptr, nullptr};
    };
    bool on = false;
    int mode = 0;   // 0, 1, ESVIO_FE_EVENT_IMAGES_AHEAD
    int nsets = 0;  // 1 in mode 1, kSets in mode 2
    int cur = 0;    // the set the getters read and plain / stage calls write
    uint32_t groups = 0;
    Set set[kSets];
    DevBuf<uint8_t> canvas;
    int fresh_cams = 0;
  } evimg;

  // ---- esvio_fe_kf_*: loop-closure keyframes (include/esvio_fe.h "keyframes" has the rules, fe_kernels.h the kernels,
  // fe_kf.h the host side).  The pattern is a SETTING (it survives esvio_fe_reset): pat, the host's copy, x1 | y1 | x2 |
  // y2; d_pat its device copy, made by esvio_fe_kf_set_pattern.  Everything else is the stage's own scratch (main stream
  // only), allocated on first use: img, the device copy of a host image; blur, the blurred plane (and what stands
  // behind a host dst); pts / desc, the points of a descriptor call and their descriptors; q / t, the device copies of
  // host descriptors of a match call; res, its results (idx | dist | status).  F works in esvio_fe_fast_corners' own
  // candidate set and score map (fast_own, fast_own_fc): both are the main stream's between calls.  h_xy / h_score:
  // where F's list arrives on the host.
  struct Kf {
    bool has_pattern = false;
    int8_t pat[4 * kKfPatternTests] = {};
    DevBuf<int8_t> d_pat;
    DevBuf<uint8_t> img, blur;
    DevBuf<float2> pts;
    DevBuf<uint32_t> desc, q, t;
    DevBuf<int32_t> res;
    std::vector<uint32_t> h_xy, h_score;
    std::vector<float> h_pts;
    std::vector<double> lift_x, lift_y;
  } kf;

  // ---- esvio_fe_bow_*: loop detection (include/esvio_fe.h "loop detection" has the rules, fe_kernels.h the kernels and
  // the tree's device layout, fe_bow.h the host side).  The vocabulary is a SETTING and the database is pose-graph
  // state: esvio_fe_reset touches neither.  Vocabulary: info as esvio_fe_bow_vocabulary_header fills it; the node arrays
  // in the layout's order; word_weight[word id], the weight of the word's leaf; passes, the 8-bit sort passes that cover
  // the keys 0..n_words.  Scratch of a transform (main stream only, grown on first use): desc, a host array's copy; word /
  // weight per descriptor; keys / vals / sort, the radix sort's; heads; q_word / q_val, the vector; cnt, k_bow_vector's
  // two counts and k_bow_select's one; err, the sort's look-back flag.  Database: db_word / db_val, the entries' vectors end
  // to end; off (host) / db_off (device), entries + 1 offsets into them; score / present per entry and res_* per result
  // of a query.
  struct Bow {
    bool has_voc = false;
    esvio_fe_bow_vocabulary_info info = {};
    int passes = 0;
    DevBuf<uint4> node_desc;
    DevBuf<uint2> kids;
    DevBuf<int32_t> node_word;
    DevBuf<double> node_weight, word_weight;
    DevBuf<uint32_t> desc, keys[2], vals[2], sort, heads, q_word, cnt;
    DevBuf<int32_t> word, err;
    DevBuf<double> weight, q_val;
    uint32_t q_n = 0;  // words in q_word / q_val
    DevBuf<uint32_t> db_word;
    DevBuf<double> db_val;
    DevBuf<uint64_t> db_off;
    std::vector<uint64_t> off = std::vector<uint64_t>(1, 0);
    DevBuf<double> score, res_score, res_raw;
    DevBuf<uint8_t> present;
    DevBuf<int32_t> res_id;
  } bow;

  // ---- esvio_fe_bow_create_vocabulary (include/esvio_fe.h "C, creating a vocabulary", fe_voc.h): `image` is the file
  // image of the last successful create, kept by esvio_fe_reset and read by esvio_fe_bow_get_created; everything else is
  // scratch of a create, apart from loop detection's (the vocabulary that is set and the database are not touched):
  // fe_kernels.h VocArgs names the per-level arrays, tree_* is the finished tree in loop detection's layout for the
  // document counts' walk.
  struct Voc {
    std::vector<uint8_t> image;
    DevBuf<uint32_t> desc, keys[2], vals[2], sort, min_dist, assign, seg_off, seg_slot, km_start, km_end, big_km, ncent, draws,
        stopped, changed, centres, pick, counts, slot_size, slot_map, ni;
    DevBuf<int32_t> seg_km, km_big, err, word, tree_word;
    DevBuf<uint64_t> run, tile_sum, km_key;
    DevBuf<double> cut_d, weight, tree_weight;
    DevBuf<int64_t> doc_off;
    DevBuf<uint4> tree_desc;
    DevBuf<uint2> tree_kids;
  } voc;
};

namespace esvio {
namespace fe {

// The stream the helpers enqueue on: the main stream unless the calling thread has switched to
// another one (prefetch -> stream2, speculative LK -> stream3).
inline thread_local hipStream_t t_stream_override = nullptr;
// the stereo stream of the frame being tracked
inline hipStream_t stereo_stream(const esvio_fe_ctx* c) { return c->stereo_unpub ? c->stream6 : c->stream4; }
inline hipStream_t cur_stream(const esvio_fe_ctx* c) {
  return t_stream_override ? t_stream_override : c->stream;
}
struct StreamScope {
  hipStream_t saved;
  explicit StreamScope(hipStream_t s) : saved(t_stream_override) { t_stream_override = s; }
  ~StreamScope() { t_stream_override = saved; }
};

// The announced batch whose prefetch sequence the thread is issuing (prefetch_issue), else null: the sequence's SAE
// update writes the event images of the batch's own set (evimg_update), and nothing handle-global.
inline thread_local const Inflight* t_prefetch_batch = nullptr;
struct PrefetchBatchScope {
  explicit PrefetchBatchScope(const Inflight* b) { t_prefetch_batch = b; }
  ~PrefetchBatchScope() { t_prefetch_batch = nullptr; }
};

// (a thread of the handle that is not the calling thread — the launch thread — gives its error texts a place of its
// own here: c->err belongs to the calling thread)
inline std::string*& fail_sink() {
  static thread_local std::string* sink = nullptr;
  return sink;
}
inline int fail(esvio_fe_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (std::string* sink = fail_sink()) *sink = buf;
    else c->err = buf;
  }
  return code;
}

#define HIPCHK(c, expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail((c), ESVIO_FE_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                  __FILE__, __LINE__);                                                       \
  } while (0)

// every hipMalloc / hipHostMalloc of a handle (Buf::alloc, fe_res.h)
inline int res_alloc(esvio_fe_ctx* c, void** p, size_t bytes, bool pinned) {
  if (pinned)
    HIPCHK(c, hipHostMalloc(p, bytes, hipHostMallocDefault));
  else
    HIPCHK(c, hipMalloc(p, bytes));
  c->n_allocs++;
  return 0;
}

// ---------------------------------------------------------------- profiling
inline Event get_event(esvio_fe_ctx* c) {
  Event e;
  if (!c->ev_pool.empty()) {
    e = std::move(c->ev_pool.back());
    c->ev_pool.pop_back();
  } else {
    (void)e.create(0);
  }
  return e;
}

struct ScopedKernel {  // brackets one launch with HIP events on the handle's stream
  esvio_fe_ctx* c;
  int id;
  uint64_t bytes;
  Event a, b;
  ScopedKernel(esvio_fe_ctx* ctx, int kid, uint64_t alg_bytes) : c(ctx), id(kid), bytes(alg_bytes) {
    if (c->prof_on) {
      a = get_event(c);
      b = get_event(c);
      (void)hipEventRecord(a, cur_stream(c));
    }
  }
  ~ScopedKernel() {
    if (a) {
      (void)hipEventRecord(b, cur_stream(c));
      c->pending.push_back(ProfRec{id, std::move(a), std::move(b), bytes});
    }
  }
};

inline void resolve_profile(esvio_fe_ctx* c) {  // main stream idle; prefetch-stream records may be pending
  std::vector<ProfRec> keep;
  for (auto& r : c->pending) {
    float ms = 0;
    const hipError_t e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e == hipErrorNotReady) {
      keep.push_back(std::move(r));
      continue;
    }
    if (e == hipSuccess) {
      c->stats[r.id].ms += ms;
      c->stats[r.id].launches++;
      c->stats[r.id].bytes += r.bytes;
    }
    c->ev_pool.push_back(std::move(r.a));
    c->ev_pool.push_back(std::move(r.b));
  }
  c->pending.swap(keep);
  (void)hipGetLastError();
}

}  // namespace fe
}  // namespace esvio
