// fe_internal.h — what fe_stages.cpp, fe_track.cpp, fe_image.cpp and fe_api.cpp share.
#pragma once
#include "fe_ctx.h"

namespace esvio {
namespace fe {

// ---------------------------------------------------------------- small templates / layouts
template <class T>
void reduce_vector(std::vector<T>& v, const std::vector<uint8_t>& status) {  // :56-81
  int j = 0;
  for (int i = 0; i < int(v.size()); i++)
    if (status[i]) v[j++] = v[i];
  v.resize(j);
}

inline uint8_t* px00(const PyrDesc& d) { return d.img[0] + (size_t)kPad * d.stride[0] + kPad; }

// the sort passes and the tiled update raise this word of the pinned block when a bounded spin runs out
inline int lookback_expired(esvio_fe_ctx* c) {
  return c->pin[0].counts[3] ? fail(c, ESVIO_FE_EINTERNAL, "radix sort look-back spin expired") : 0;
}

// ---------------------------------------------------------------- fe_stages.cpp
int ensure_event_capacity(esvio_fe_ctx* c, size_t n);
int ensure_sort_capacity(esvio_fe_ctx* c, size_t n);
int ensure_part_capacity(esvio_fe_ctx* c, size_t n, bool mc);
int ensure_cand_capacity(esvio_fe_ctx* c, int set, size_t n);
int ensure_arc_capacity(esvio_fe_ctx* c, size_t n, int set);
int pyr_alloc(esvio_fe_ctx* c, PyrStore& ps, int w, int h, int max_level);
uint64_t pyr_pixels(const PyrDesc& d);  // of all its levels
void pyr_build(esvio_fe_ctx* c, const PyrDesc* p, int nimg);
McParams make_mc_params(const esvio_fe_motion* m);
// arc_set >= 0: this batch's Arc* pass will run into candidate set arc_set; *arc_marked tells
// whether the update has set that set's touched flags on its way (else run_arc does it)
int sae_update(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
               const McParams* mc = nullptr, double2* L2 = nullptr, double2* S2 = nullptr, int arc_set = -1,
               bool* arc_marked = nullptr);
// esvio_fe_set_event_images is on: sae_update of the handle's own planes ends in evimg_update — the batch into the
// event images, the cameras of evimg.fresh_cams rewritten, the others accumulated; with no events it still rewrites
// the fresh ones (a track call whose update is skipped); inside an announced batch's prefetch sequence
// (t_prefetch_batch) it rewrites both cameras of the batch's own set.  evimg_zero: both images of the current set
// zero, on the current stream (every_set: esvio_fe_reset's, behind a call that may have failed half way — every set
// and its mark planes)
int evimg_update(esvio_fe_ctx* c, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR, const McParams* mc);
int evimg_zero(esvio_fe_ctx* c, bool every_set = false);
int radix_sort_pairs(esvio_fe_ctx* c, uint32_t n, int passes, int bits, bool booked = true);
// ... of other buffers than the handle's keys[] / vals[] / hist; n_dev (optional): the count is *n_dev, read on the
// device, and n its upper bound (launch_radix_pass)
struct SortBufs {
  uint32_t *keys[2], *vals[2];
  uint32_t* scratch;  // sort_scratch() layout
  const uint32_t* n_dev;
};
int radix_sort_pairs(esvio_fe_ctx* c, const SortBufs& b, uint32_t n, int passes, int bits, bool booked);
// the seven arrays of a candidate set (total_words: of its `total`; fast_run keeps a second count behind it)
int cand_set_alloc(esvio_fe_ctx* c, esvio_fe_ctx::CandSet& s, size_t cap, size_t total_words = 1);
int stage_events(esvio_fe_ctx* c, const esvio_fe_event* left, size_t nL, const esvio_fe_event* right,
                 size_t nR, int space, const EventRec** dL, const EventRec** dR, int lane = -1);
void render_ts(esvio_fe_ctx* c, double t_sync, uint8_t* dst0, uint8_t* dst1, int ncam, const double2* S2);
void run_clahe(esvio_fe_ctx* c, const uint8_t* src0, const uint8_t* src1, int src_stride, uint8_t* dst0, uint8_t* dst1,
               int dst_stride, int nimg, int stages, uint64_t booked_px);
void render_lk_images(esvio_fe_ctx* c, double t_sync, int cams, int slotL, int slotR, int rawbuf);
bool render_cam_ok(const esvio_fe_ctx* c);  // one camera alone can be built with the fused kernels
void build_lk_images(esvio_fe_ctx* c, double t_sync, int cams /*1 left, 2 right, 3 both*/, int slotL, int slotR,
                     int rawbuf, bool right_imported = false);
inline int other_right_slot(const esvio_fe_ctx* c) { return c->slot_curR == kLeftSlots ? kLeftSlots + 1 : kLeftSlots; }
void rotate_slots(esvio_fe_ctx* c, bool right_advanced);
const PyrDesc& raw_ts_desc(const esvio_fe_ctx* c, int cam);
LkArgs make_lk(const PyrDesc& P, const PyrDesc& N, const float2* prev, const float2* init, float2* next,
               uint8_t* status, const int* n_ptr, int n_max, int max_level, int max_count, double eps,
               int flags);
void run_lk(esvio_fe_ctx* c, const LkArgs& f, const LkArgs* b, float2* back_pts, uint8_t* back_status);
// A forward call P -> N from `src` (null: chained input) and its reverse N -> P, both into `out` (device addresses).
// Temporal (:410, :416-418): the reverse with maxLevel 1 and USE_INITIAL_FLOW, seeded with the source points;
// stereo (:490, :495, and both pairs of trackImage): the reverse like the forward call.  The caller sets the
// poll_* / chain_* / gate_* fields of f; run_lk_pair launches the reverse call with it if cfg.flow_back.
enum LkPairKind { kLkTemporal, kLkStereo };
struct LkPair {
  LkArgs f, b;
  LkOut out;
};
LkPair lk_pair(const PyrDesc& P, const PyrDesc& N, const P2f* src, const int* n_ptr, int n_max, LkPairKind kind,
               const LkOut& out);
void run_lk_pair(esvio_fe_ctx* c, const LkPair& p);
int copy_level0_out(esvio_fe_ctx* c, const PyrDesc& d, uint8_t* out);
int copy_level0_in(esvio_fe_ctx* c, const PyrDesc& d, const uint8_t* in, int space = ESVIO_FE_HOST);  // (where `in` lies)
bool in_border_event(const esvio_fe_ctx* c, const P2f& pt);
double pt_distance(const P2f& a, const P2f& b);
void event_set_mask(esvio_fe_ctx* c);
std::vector<P2f> undistorted_pts(const std::vector<P2f>& pts, const esvio_fe_camera& cam);
std::vector<P2f> pts_velocity_fn(std::vector<int>& ids, std::vector<P2f>& pts, IdMap& cur_id_pts,
                                 IdMap& prev_id_pts, double dt, size_t n_left);
void reject_with_f_event(esvio_fe_ctx* c);
void clear_tracker_state(esvio_fe_ctx* c);
SelectArgs make_select_args(esvio_fe_ctx* c, int set, int max_corners, float2* out_pts, int out_base,
                            int32_t* out_idx);
size_t select_lds_bytes(const esvio_fe_ctx* c);
KernelId launch_select_args(esvio_fe_ctx* c, SelectArgs s);  // (returns the form it launched)
void compact_set(esvio_fe_ctx* c, const esvio_fe_ctx::CandSet& cs, uint32_t nblk, bool booked);
void run_select(esvio_fe_ctx* c, int set, int max_corners, float2* out_pts, int out_base, int32_t* out_idx,
                const uint32_t* mask_bits = nullptr, int* host_counts = nullptr, bool publish = false,
                const float2* stamp_pts = nullptr, int n_stamp = 0);
void run_arc(esvio_fe_ctx* c, const EventRec* ev, uint32_t n, const PyrDesc* ts, bool use_mask,
             bool want_flags, bool want_cand, int set, bool marked = false);
// a frame's candidates into set `set`, by the handle's detector: the Arc* pass over the batch's left events and its
// ordered compaction, or the FAST pass over `ts`, the frame's raw left time surface
int run_detect(esvio_fe_ctx* c, const EventRec* ev, uint32_t n, const PyrDesc& ts, int set, bool marked);
// candidates set `set` must have room for before a frame with n left events is detected in it
inline size_t detect_cand_need(const esvio_fe_ctx* c, size_t n) { return c->detector == ESVIO_FE_DETECT_FAST ? (size_t)c->P : n; }
hipError_t sync_main(esvio_fe_ctx* c);
hipError_t sync_event(hipEvent_t ev);

// ---------------------------------------------------------------- fe_evstage.cpp (host-resident batches)
int stager_threads_from_env();  // ESVIO_FE_STAGE_THREADS (default 2; 0: plain hipMemcpyAsync from the caller's memory)
inline bool stager_enabled(const esvio_fe_ctx* c) { return c->stage_threads > 0; }
int stager_begin(esvio_fe_ctx* c, const esvio_fe_event* left, size_t nL, const esvio_fe_event* right, size_t nR,
                 int dma_groups, int* slot_out, bool by_camera = false);
int stager_attach_left(esvio_fe_ctx* c, int slot, hipStream_t s, const EventRec** dL);
int stager_mark_read_aux(esvio_fe_ctx* c, int slot, hipStream_t s);
bool stager_ready(esvio_fe_ctx* c, int slot);
int stager_attach(esvio_fe_ctx* c, int slot, size_t nL, hipStream_t s, const EventRec** dL, const EventRec** dR);
int stager_mark_read(esvio_fe_ctx* c, int slot, hipStream_t s, bool main_stream);
int stager_release(esvio_fe_ctx* c, int slot);
void stager_abandon(esvio_fe_ctx* c, int slot);
void stager_share_pool(esvio_fe_ctx* c);  // (re)connect the RANSAC helpers to the staging queue
int stager_reserve(esvio_fe_ctx* c, size_t n_events);
void stager_ptrs(esvio_fe_ctx* c, int slot, size_t nL, const EventRec** dL, const EventRec** dR);
void stager_drain(esvio_fe_ctx* c);
void stager_destroy(esvio_fe_ctx* c);
void stager_copy_bytes(uint8_t* dst, const uint8_t* src, size_t len);  // (test tap: a chunk's copy)
bool stager_pack_bytes(uint8_t* dst, const uint8_t* src, size_t len, uint32_t* base_sec);  // (test tap: a chunk packed to 8 B per event)
void stager_counters(esvio_fe_ctx* c, uint64_t out4[4]);  // {batches, bytes, chunks sent packed, chunks of packing batches sent raw}

// ---------------------------------------------------------------- fe_track.cpp
int prefetch_next(esvio_fe_ctx* c, bool wait_planes, bool must_take_first = false);
int launcher_set(esvio_fe_ctx* c, bool on);   // start / stop the launch thread
int stereo_split_prepare(esvio_fe_ctx* c);   // the second stereo stream, if this handle may use it (fe_track.cpp)
int launcher_drain(esvio_fe_ctx* c);          // every job handed over has been issued (returns the first job error)
int launcher_wait_lane(esvio_fe_ctx* c, int lane);  // ... the job that records this lane's events
void launcher_clear_error(esvio_fe_ctx* c);   // esvio_fe_reset: a failed job.s sticky error is dropped with the batches
int cancel_chain(esvio_fe_ctx* c);
int finalize_lazy(esvio_fe_ctx* c);  // what lazy calls left open: the new corners' right entries, then the right-camera tail
int track_event_impl(esvio_fe_ctx* c, double cur_time, const esvio_fe_event* left, size_t nL,
                     const esvio_fe_event* right, size_t nR, int space, bool PUB_THIS_FRAME,
                     const esvio_fe_motion* motion = nullptr);

// ---------------------------------------------------------------- fe_api.cpp (track exchange)
// pack the current frame's PointCloud records into the pinned send area (waits for the previous
// exchange to be through with it) and mark them "to be enqueued"; enqueue what is marked: upload +
// ncclAllGather + download on the exchange stream (no-op when nothing is marked)
int exchange_pack(esvio_fe_ctx* c);
int exchange_flush(esvio_fe_ctx* c);

// ---------------------------------------------------------------- fe_image.cpp
void euclid_halfwidths(double md, int8_t* hw /*[kMaxDiscR+1]*/, int* radius);
int gftt_run(esvio_fe_ctx* c, const PyrDesc& d, int max_corners, double quality, double min_distance,
             bool use_mask, float2* out_pts, int out_base, int* host_counts);
// FAST-9/10 (+ score_10, 3x3 non-max) of the W x H image at `img` (device memory, rows `stride` bytes apart) on
// the current stream; synchronises it.  Up to `capacity` corners in raster order go to out_xy / out_score (host).
int fast_run(esvio_fe_ctx* c, const uint8_t* img, int stride, int arc, int barrier, bool nonmax, int16_t* out_xy,
             int32_t* out_score, int32_t capacity, int32_t* n_out, int32_t* n_detected);
// (in a candidate set and FAST scratch of its own, esvio_fe_ctx::fast_own / fast_own_fc, allocated by the first call)
// rule F of include/esvio_fe.h "keyframes" (cv::FAST, TYPE_9_16, non-max) in the same set and scratch: the whole list
// on the host, raster order, xy[i] = x | y << 16; *n_detected (optional): the corners before non-max
int fast_keyframe_run(esvio_fe_ctx* c, const uint8_t* img, int stride, int threshold, std::vector<uint32_t>& xy,
                      std::vector<uint32_t>& score, int32_t* n_detected);
// ESVIO_FE_DETECT_FAST (esvio_fe_ctx::fastc): everything the candidate passes and the stage tap need, allocated once;
// what the stage tap alone needs
int ensure_fast_detector(esvio_fe_ctx* c);
int ensure_fast_tap(esvio_fe_ctx* c);
// FAST-10 + score_10 + nonmax_3x3 of the image at `img` -> candidate set `cs`, ordered by score (descending, equal
// scores in raster order), corners whose byte is (uint8_t)ts_lk_threshold left out, in the scratch `fc`, on the current
// stream; no host synchronisation.  want_count: fc.tot[0] = the survivors of the non-max, those left out included
int fast_cand_pass(esvio_fe_ctx* c, const uint8_t* img, int stride, int barrier, const esvio_fe_ctx::CandSet& cs,
                   const esvio_fe_ctx::FastCand& fc, bool want_count);
int run_fast_cand(esvio_fe_ctx* c, const PyrDesc& ts, int set);  // ... of a frame's raw left time surface -> cand[set]
int track_image_impl(esvio_fe_ctx* c, double cur_time, const uint8_t* img_left, const uint8_t* img_right,
                     bool PUB_THIS_FRAME, int space = ESVIO_FE_HOST);  // (where both images lie)

}  // namespace fe
}  // namespace esvio
