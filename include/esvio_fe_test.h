/* esvio_fe_test.h — test and measurement taps of libesvio_fe.so.
 *
 * NOT part of the drop-in boundary (include/esvio_fe.h): nothing here replaces a
 * call of the reference.  These entry points exist so that tests/ and bench.py can reach pieces of the host
 * side in isolation (the RANSAC pool under adverse scheduling, the staging copy, the 7-point solver's
 * null-space basis), run the min-distance selection over a list of their own, inject faults into the bounded device-side waits, and read counters.  A caller of the
 * front-end never needs them.
 */
#ifndef ESVIO_FE_TEST_H
#define ESVIO_FE_TEST_H
#include "esvio_fe.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- host RANSAC (esvio_fe_find_fundamental_mat) under test conditions ------------------- */
/* The same with `threads` - 1 helper threads solving / scoring the RANSAC iterations (a temporary
 * pool; test tap for esvio_fe_set_host_threads): status and count are those of the call above. */
int esvio_fe_find_fundamental_mat_mt(const float* p1, const float* p2, int n, double thr,
                                     double conf, int threads, uint8_t* status, int32_t* n_inliers);
/* Test tap: the same with job buffers of the pool marked as still holding a helper (hold_mask bit 0 / 1:
 * buffer 0 / 1), as when a helper thread loses its CPU in the middle of a job: the call must not wait for
 * it — it takes the other buffer, or runs without the helpers when both are held — and must return the
 * same status and count (esvio_fe_ransac_tail counts both cases).  threads >= 2. */
int esvio_fe_find_fundamental_mat_held(const float* p1, const float* p2, int n, double thr, double conf,
                                       int threads, int hold_mask, uint8_t* status, int32_t* n_inliers);
/* Test tap: the same while the pool's helpers have other work between jobs, the way the host-batch staging hands
 * them chunks (fe_evstage.cpp): `repeats` calls, `idle_units` units of ~5 us arriving before each; status and
 * count must equal esvio_fe_find_fundamental_mat's; out3 = {calls of the idle hook (a helper that is idle when the
 * hook is registered calls it once then), units done, units left after a bounded wait (0)}.  threads >= 2. */
int esvio_fe_find_fundamental_mat_idle(const float* p1, const float* p2, int n, double thr, double conf,
                                       int threads, int repeats, int idle_units, uint8_t* status, int32_t* n_inliers,
                                       uint64_t out3[3]);
/* Test tap: the hypot inside that function's 7-point solver: cv::SVD's Jacobi rotations call hypot
 * unqualified inside namespace cv, which resolves to lapack.cpp's own a*sqrt(1+(b/a)^2) template, not
 * to libm's; IEEE operations only, so the result does not depend on the host's libm. */
int esvio_fe_host_hypot(const double* x, const double* y, int n, double* out);
/* Test tap: the copy the staging threads move a chunk of a host-resident event batch with (pageable source ->
 * pinned buffer; streaming stores where dst is 16-byte aligned, memcpy otherwise and for the last < 64 bytes):
 * dst[0, len) = src[0, len), nothing else written.  No device involved. */
int esvio_fe_host_stage_copy(void* dst, const void* src, size_t len);
/* Test tap: the basis of the 7x9 epipolar system's null space that run7Point takes from
 * cv::SVDecomp(A, W, U, Vt, MODIFY_A + FULL_UV) (rows 7 and 8 of Vt; OpenCV calib3d/fundam.cpp, reached
 * from feature_tracker.cpp:935), for n systems of 63 doubles -> f12 = n x (f1[9] | f2[9]).  lanes = 0:
 * one system at a time; lanes != 0: side by side in vector lanes with the sweep's independent row pairs
 * scheduled together, as the RANSAC loop solves its hypotheses — both must give the same bits.
 * *redone (may be NULL) = systems the lane form handed back to the one-at-a-time routine. */
int esvio_fe_host_nullspace(const double* systems, int n, int lanes, double* f12, int32_t* redone);
/* One chunk of a host batch as the staging threads pack it for a plain call's pull over PCIe (fe_evstage.cpp stage_pack):
 * len bytes of 16-byte records at src -> len / 2 bytes at dst (16-byte aligned), 8 bytes per event: x | y << 16, then
 * nsec | (polarity != 0) << 30 | (sec - *base_sec) << 31.  Returns 1 if every event fits that form (nsec < 2^30, second
 * = the first event's or the one after), 0 if not (the chunk then travels raw) — decided before anything is written:
 * returns 0 => no byte of dst is written; returns 1 => dst[0, len / 2) and nothing else —, < 0 on bad arguments. */
int esvio_fe_host_stage_pack(void* dst, const void* src, size_t len, uint32_t* base_sec);
/* {host batches staged, bytes staged, chunks that went to the device packed, chunks of packing batches that went raw} */
int esvio_fe_staging_counters(esvio_fe_handle h, uint64_t out4[4]);

/* ---- fault injection (tests) ----------------------------------------------------------- */
/* Every device-side wait is bounded: a wave that gives up raises a host-visible flag and the call
 * either fails with ESVIO_FE_EINTERNAL (the SAE update's turn ticket and the radix sort's look-back:
 * the planes are then partially updated; esvio_fe_reset makes the handle usable again) or redoes the
 * launch the plain way (the speculative / chained temporal LK of replay mode: results unchanged).
 * esvio_fe_debug_inject makes the chosen waits expire the first time they would have to wait, for the
 * launches that follow (0: normal bounds again); ESVIO_FE_FAULT=<mask> in the environment does the
 * same from esvio_fe_create on.  esvio_fe_debug_counters: {speculative launches redone, chained
 * launches redone, chained launches made, chained launches used}. */
#define ESVIO_FE_FAULT_TICKET 1
#define ESVIO_FE_FAULT_LOOKBACK 2
#define ESVIO_FE_FAULT_SPECULATIVE 4
#define ESVIO_FE_FAULT_CHAINED 8
/* replay mode's lazy completions as late as they may ever happen, whether or not the stereo LK they wait for is over: a
 * lazily returning call always leaves the previous published frame's new corners to the next call, a published call
 * always runs the previous frame's right-camera tail in its own tail — the order of the two, not their timing, is what
 * results depend on */
#define ESVIO_FE_FAULT_LAZY_LATE 16
int esvio_fe_debug_inject(esvio_fe_handle h, int mask);
int esvio_fe_debug_counters(esvio_fe_handle h, uint64_t out4[4]);
/* What the plain calls (nothing announced, not lazy: the reference node's pattern) did since create:
 * {plain calls, of them with the two cameras' SAE update + image on two streams, stereo LK launches
 * chained to the temporal one on the device, chained launches redone}. */
int esvio_fe_plain_call_counters(esvio_fe_handle h, uint64_t out4[4]);

/* Tail of the host RANSAC (process-wide, like esvio_fe_ransac_stats; reset together with it or here):
 * out6 = {slowest RANSAC call [ns], slowest LMedS call [ns], iterations the calling thread redid because
 * the helper that took them did not deliver, jobs the calling thread ran alone because helpers were
 * still inside both job buffers, jobs that took the other buffer because a helper was still inside
 * theirs (a helper that lost its CPU in the middle of a job), involuntary context switches of the helper
 * threads}. */
int esvio_fe_ransac_tail(uint64_t out6[6], int reset);



/* ---- taps on single stages (tests compare them with the oracle; the reference has no such calls) -------- */
/* write a camera's four planes (each width*height doubles, index x + y*width); the read side is
 * esvio_fe_get_sae in esvio_fe.h */
int esvio_fe_set_sae(esvio_fe_handle h, int cam, const double* L0, const double* L1,
                     const double* S0, const double* S1);

/* test tap: the pyramid the LK stage builds for a host image: level `level` u8 image
 * (lw*lh bytes) and its Scharr derivatives (lw*lh*2 int16, interleaved Ix,Iy). Either output
 * may be NULL. Returns the number of levels built (maxLevel+1) in *n_levels. */
int esvio_fe_build_pyramid(esvio_fe_handle h, const uint8_t* img, int w, int hgt, int max_level,
                           int level, uint8_t* out_img, int16_t* out_deriv, int32_t* lw,
                           int32_t* lh, int32_t* n_levels);
/* test tap: one level of the pyramid the last track call (or esvio_fe_sae_to_time_surface: level 0 only) left in the
 * current slot of `cam` (0 left, 1 right: the slots esvio_fe_export_image reads), WITH its border: (h_l + 48) rows of
 * (w_l + 48) image bytes into img, as many interleaved (Ix, Iy) int16 pairs into deriv (either may be NULL); *w, *hgt =
 * w_l, h_l, *levels = the handle's top level.  Copies and a wait for the stream only, no launch.  ESVIO_FE_EINVAL for
 * a bad cam or level and while batches are announced or in flight; what a lazy call left open is completed first. */
int esvio_fe_export_level(esvio_fe_handle h, int cam, int level, uint8_t* img, int16_t* deriv, int32_t* w,
                          int32_t* hgt, int32_t* levels);
/* test tap: the greedy min-distance selection every detector ends in (Event_FeaturesToTrack, the FAST selection,
 * goodFeaturesToTrack's distance pass, trackEvent / trackImage behind Event_setMask), over a caller's candidate list.
 * The rule: seed a map of blocked pixels from `mask` (width*height bytes, 255 = blocked; may be NULL) and from the
 * filled discs round the n_stamp points of stamp_xy (x, y float pairs, rounded like cvRound: to nearest, ties to even;
 * may be NULL when n_stamp = 0); walk the n candidates in order; skip one whose pixel is blocked, else accept it and
 * block the disc round it, clipped to the sensor; stop after max_corners.
 *   xy[i] = x | y << 16, payload[i] comes back in out_idx for an accepted candidate.  n = 0 is valid.  Every candidate
 *   must lie inside the sensor and every stamp point must round to a pixel of it, else ESVIO_FE_EINVAL: the kernels
 *   index the map with them unchecked.
 *   disc: cv::circle's filled disc of the integer radius `disc` in 1..63, or with ESVIO_FE_SELECT_EUCLID the open
 *   Euclidean disc dx*dx + dy*dy < disc*disc of a min_distance in [1, 63] — per call, the handle's min_dist plays no
 *   part.  ESVIO_FE_SELECT_TABLE: the kernels test membership with the half-width table where they would use the
 *   equivalent threshold on dx*dx + dy*dy (which every disc of either kind has: no other caller takes the table path).
 *   n_stamp <= max_cnt, 0 <= max_corners, 0 <= out_base, out_base + max_corners <= max_cnt.
 *   variant 0: the kernel the handle launches for its own selections; 1: the one-wave kernel (as ESVIO_FE_SELECT_SERIAL);
 *   2: the map in device memory even where it fits LDS (allocated on the first such call).
 *   out_xy (max_cnt x, y pairs) and out_idx (max_cnt) are read AND written: they travel to the device whole, the
 *   accepted points land at out_xy[out_base + k], their payloads at out_idx[k], and both travel back whole, so that a
 *   caller sees what the kernel wrote outside these.  counts = {accepted, out_base + accepted, n}.  *kernel_id (may be
 *   NULL): the kernel that ran, for esvio_fe_kernel_name.  Not while batches are announced; what a lazy call left open
 *   is completed first.  Publication to a waiting LK launch (replay mode) is not part of the tap. */
#define ESVIO_FE_SELECT_EUCLID 1
#define ESVIO_FE_SELECT_TABLE 2
int esvio_fe_select_candidates(esvio_fe_handle h, const uint32_t* xy, const int32_t* payload, int n, double disc,
                               int flags, const uint8_t* mask, const float* stamp_xy, int n_stamp, int max_corners,
                               int out_base, int variant, float* out_xy, int32_t* out_idx, int32_t counts[3],
                               int32_t* kernel_id);
/* camodocal PinholeCamera::liftProjective (PinholeCamera.cc:450-510); host-side. */
int esvio_fe_lift_projective(const esvio_fe_camera* cam, double u, double v, double* out3);

/* Measurement tap: process-wide counters of that function since the last reset — out6 = {calls,
 * loop iterations, points, nanoseconds inside the calls} of its RANSAC branch (>= 15 points) and
 * {calls, nanoseconds} of its LMedS branch (8..14 points, what OpenCV runs below 15). */
int esvio_fe_ransac_stats(uint64_t* out6, int reset);

/* ---- measurement --------------------------------------------------------------------- */
/* Wall time of the esvio_fe_track_event(_mc) calls on this handle since the last reset, as the calling
 * thread sees them (always on: a dozen clock reads per call).  The percentiles cover the latest 4096
 * calls.  For the slowest call: its index since the reset, whether it published, where its time went
 * (esvio_fe_latency_phase_name(i) names max_phase_ms[i]; entries 8.. are parts of entry 5 on published
 * frames), the CPUs the calling thread was on when it began / ended, the involuntary context switches
 * the thread suffered inside it (getrusage(RUSAGE_THREAD)) and the device / pinned allocations it
 * made. */
#define ESVIO_FE_LATENCY_PHASES 16
typedef struct esvio_fe_latency {
  uint64_t calls;
  double mean_ms, p50_ms, p99_ms, max_ms;
  uint64_t max_call;
  int32_t max_published;
  int32_t max_cpu_begin, max_cpu_end;
  int64_t max_invol_switches;
  int64_t max_allocs;
  double max_phase_ms[ESVIO_FE_LATENCY_PHASES];
  uint64_t allocs;          /* allocations inside track / announce / keyframe (esvio_fe_kf_*) calls since the reset */
  uint64_t invol_switches;  /* involuntary context switches inside track calls since the reset */
} esvio_fe_latency;
int esvio_fe_latency_stats(esvio_fe_handle h, esvio_fe_latency* out, int reset);
const char* esvio_fe_latency_phase_name(int i);
/* One of the latest 256 track calls as the record above saw it (back = 0: the last call, 1: the one before ...):
 * when it began (ms since the first track call after the last reset), how long it took, whether it published, and its phases —
 * read AFTER a run, so that looking does not change the schedule that is looked at.  ESVIO_FE_EINVAL for a call
 * that is not kept (any more). */
typedef struct esvio_fe_latency_call {
  uint64_t call;      /* index of the call since the last reset of esvio_fe_latency_stats (as max_call there) */
  int32_t published;
  int32_t reserved;
  double begin_ms, ms;
  double phase_ms[ESVIO_FE_LATENCY_PHASES];
} esvio_fe_latency_call;
int esvio_fe_latency_recent(esvio_fe_handle h, int back, esvio_fe_latency_call* out);
/* Per-kernel HIP-event timing on the handle's stream (off by default; when on, every launch is
 * bracketed by hipEventRecord and resolved lazily). */
int esvio_fe_set_profiling(esvio_fe_handle h, int on);
int esvio_fe_kernel_count(void);
/* ids 0 .. esvio_fe_kernel_count()-1: the kernels of the tracker's entry points; ids up to
 * esvio_fe_stage_kernel_count()-1: those and the kernels of stages no track call launches (esvio_fe_filter_events).
 * esvio_fe_kernel_name and esvio_fe_get_kernel_stats take every id below esvio_fe_stage_kernel_count() — and the ingest
 * range behind it, esvio_fe_ingest_kernel_count() below. */
int esvio_fe_stage_kernel_count(void);
const char* esvio_fe_kernel_name(int kernel_id);
/* total_ms / launches / algorithmic bytes accumulated since the last reset_kernel_stats */
int esvio_fe_get_kernel_stats(esvio_fe_handle h, int kernel_id, double* total_ms,
                              uint64_t* launches, uint64_t* alg_bytes);
int esvio_fe_reset_kernel_stats(esvio_fe_handle h);
/* the bytes of raw words one workgroup of the decode chain takes (esvio_fe_decode_raw): where its tile edges lie */
int esvio_fe_raw_tile_bytes(void);
/* the AEDAT chain: events per tile of k_aedat_count / k_aedat_emit; the timer ids of its kernels are a range of their
 * own BEHIND the stage table — esvio_fe_stage_kernel_count() <= id < esvio_fe_ingest_kernel_count() —, which
 * esvio_fe_kernel_name and esvio_fe_get_kernel_stats take as well; the stage table itself stays as it is */
int esvio_fe_aedat_tile_events(void);
int esvio_fe_ingest_kernel_count(void);
/* The AEDAT host walk alone (esvio_amd/csrc/fe_aedat.h), no handle and no device: an event walker's state in and out
 * (state_bytes == esvio_fe_aedat_walk_state_bytes(); all zero is the fresh state), the n_bytes of a chunk in; out come
 * the run table — runs[2k] = index of the run's first record in the packed payload, runs[2k+1] = its eventTSOverflow as
 * a bit pattern; at most runs_cap entries are written —, the packed 8-byte polarity records (at most events_cap of them)
 * and counts = {records, runs, polarity packets, other packets} of the chunk, counted whether stored or not.  runs and
 * payload may be null.  A malformed header: ESVIO_FE_EINVAL, the state as it was. */
int esvio_fe_aedat_walk_tap(void* state, size_t state_bytes, const void* bytes, size_t n_bytes, uint32_t* runs, size_t runs_cap,
                            uint8_t* payload, size_t events_cap, uint64_t counts[4]);
int esvio_fe_aedat_walk_state_bytes(void);
/* The AEDAT host walk in its frame mode alone ("AEDAT 3.1 frames"), no handle and no device: a frame walker's state in
 * and out (as above), the only size taken (width 0: any), the n_bytes of a chunk in.  `carry` holds the pixel bytes of
 * the open frame that earlier calls left waiting (the state says how many) and takes, on success, those that wait behind
 * this call (room for carry_cap; it needs the waiting bytes + n_bytes at the most).  Out come the emitted frames' pixel
 * bytes, each frame from a 16-byte boundary of pix (nothing is stored unless all fit pix_cap bytes), the frame table (at
 * most frames_cap rows) and counts = {frames, pixel bytes with their padding, invalid, BAD, frame packets, other packets,
 * bytes waiting behind the call, 0}.  pix and frames may be null.  A malformed header or event, a refused frame or a BAD
 * stamp: ESVIO_FE_EINVAL, state and carry as they were, the broken rule as text in `why` (room for why_cap; optional). */
int esvio_fe_aedat_frame_walk_tap(void* state, size_t state_bytes, uint32_t width, uint32_t height, const void* bytes,
                                  size_t n_bytes, int64_t t_offset_ns, uint32_t flags, uint8_t* carry, size_t carry_cap,
                                  uint8_t* pix, size_t pix_cap, esvio_fe_aedat_frame* frames, size_t frames_cap,
                                  uint64_t counts[8], char* why, size_t why_cap);
/* k_frame16_emit (esvio_fe_decode_aedat_frames, esvio_fe_convert_frame16), booked in a timer slot of its own behind
 * every other table — the stage and ingest tables, whose ends tests pin, stay as they are; as esvio_fe_get_kernel_stats
 * otherwise.  esvio_fe_frame16_tile_pixels: pixels per workgroup of the kernel. */
int esvio_fe_aedat_frame_kernel_stats(esvio_fe_handle h, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
int esvio_fe_frame16_tile_pixels(void);
/* the bag stage: events per tile of k_bag_emit, whose timer id is appended to the ingest range above */
int esvio_fe_bag_tile_events(void);
/* The bag host walk alone (esvio_amd/csrc/fe_bag.h), no handle and no device: a walker's state in and out (state_bytes ==
 * esvio_fe_bag_walk_state_bytes(); all zero is the fresh state), the topics as esvio_fe_bag_set_topics takes them, side
 * != 0 for the side walk, the n_bytes of a chunk in; out come each camera's gathered 13-byte wire events (at most
 * events_cap[cam]), the message table (at most msgs_cap), the IMU samples (at most imu_cap) and counts = {left events,
 * right events, left messages, right messages, messages, samples, BAD samples, other_messages, other_records, chunks,
 * connections, 0}, counted whether stored or not.  Every output pointer may be null.  A malformed stream:
 * ESVIO_FE_EINVAL, the state as it was, the broken rule as text in `why` (room for why_cap bytes; optional). */
int esvio_fe_bag_walk_tap(void* state, size_t state_bytes, const esvio_fe_bag_topics* topics, int side, const void* bytes,
                          size_t n_bytes, uint8_t* const payload[2], const size_t events_cap[2], esvio_fe_bag_message* msgs,
                          size_t msgs_cap, esvio_fe_imu_sample* imu, size_t imu_cap, uint64_t counts[12], char* why,
                          size_t why_cap);
int esvio_fe_bag_walk_state_bytes(void);
/* The bag host walk in its image mode alone, no handle and no device: the image walker's state in and out (as above), the
 * topics as esvio_fe_bag_set_image_topics takes them, the only size taken (width 0: any), the n_bytes of a chunk in.
 * `carry` holds the bytes of the open payload that earlier calls left waiting (the state says how many) and takes, on
 * success, those that wait behind this call (room for carry_cap; it needs the waiting bytes + n_bytes at the most).  Out
 * come the completed messages' payloads, each from a 16-byte boundary of pix (nothing is stored unless all fit pix_cap
 * bytes), the image table (at most imgs_cap) and counts = {messages, left messages, right messages, payload bytes with
 * their padding, other_messages, other_records, chunks, connections, bytes waiting behind the call, 0, 0, 0}.  pix and
 * imgs may be null.  A malformed stream or a refused message: ESVIO_FE_EINVAL, state and carry as they were, the broken
 * rule as text in `why`. */
int esvio_fe_bag_image_walk_tap(void* state, size_t state_bytes, const char* left, const char* right, uint32_t width,
                                uint32_t height, const void* bytes, size_t n_bytes, uint8_t* carry, size_t carry_cap,
                                uint8_t* pix, size_t pix_cap, esvio_fe_bag_image* imgs, size_t imgs_cap, uint64_t counts[12],
                                char* why, size_t why_cap);
/* pixels per workgroup of k_image_emit, whose timer id is appended to the ingest range above */
int esvio_fe_image_tile_pixels(void);
/* the event images' two kernels (esvio_fe_set_event_images), booked in timer slots of their own outside the stage and
 * ingest tables: which = 0, k_evimg_mark; 1, k_evimg_emit (both forms); as esvio_fe_get_kernel_stats otherwise */
int esvio_fe_event_image_kernel_stats(esvio_fe_handle h, int which, double* total_ms, uint64_t* launches,
                                      uint64_t* alg_bytes);
/* the keyframe stage's kernels (esvio_fe_kf_*), a table of their own in timer slots outside the stage and ingest tables,
 * which stay as they are: esvio_fe_kf_kernel_count() names, k_kf_blur, k_kf_brief, k_kf_match (the corners run on
 * k_fast_score / k_fast_collect / k_compact of the stage table); esvio_fe_kf_kernel_name: "" for any other id;
 * esvio_fe_kf_kernel_stats as esvio_fe_get_kernel_stats.  esvio_fe_kf_blur_tile: the pixels one workgroup of k_kf_blur
 * writes — where its tile seams lie. */
int esvio_fe_kf_kernel_count(void);
const char* esvio_fe_kf_kernel_name(int which);
int esvio_fe_kf_kernel_stats(esvio_fe_handle h, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
int esvio_fe_kf_blur_tile(int32_t* tile_w, int32_t* tile_h);
/* loop detection's kernels (esvio_fe_bow_*), a table of their own in timer slots behind the keyframes'; every other
 * table stays as it is: esvio_fe_bow_kernel_count() names, k_bow_walk, k_bow_vector, k_bow_score, k_bow_select (the sort
 * between the first two is booked as k_radix_pass of the TRACK table, esvio_fe_kernel_count's, as esvio_fe_hot_select's
 * passes are: a host that profiles the track path sees a bow call's sort launches and bytes in that slot); esvio_fe_bow_kernel_name: "" for any other id;
 * esvio_fe_bow_kernel_stats as esvio_fe_get_kernel_stats.
 * esvio_fe_bow_limits: the sizes at which the kernels change path — group_lanes: k_bow_walk's lanes per descriptor (a node
 * with more children takes more rounds); lds_words: the query words k_bow_score keeps in LDS (a longer vector is looked
 * up in memory); vector_block: the values k_bow_vector's norm chain stages at a time.
 * esvio_fe_bow_scores: for the query Q(desc, max_id) the raw sum s_e (score[e], 0.0 where absent) and whether the entry is
 * present (present[e], 0 or 1) for every entry — room for esvio_fe_bow_entries() each, host memory; nothing is added. */
typedef struct esvio_fe_bow_limits_info {
  int32_t group_lanes;
  int32_t lds_words;
  int32_t vector_block;
  int32_t max_results;
} esvio_fe_bow_limits_info;
int esvio_fe_bow_kernel_count(void);
const char* esvio_fe_bow_kernel_name(int which);
int esvio_fe_bow_kernel_stats(esvio_fe_handle h, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
int esvio_fe_bow_limits(esvio_fe_bow_limits_info* out);
int esvio_fe_bow_scores(esvio_fe_handle h, const uint32_t* desc, int n, int space, int max_id, double* score, uint8_t* present);
/* vocabulary creation's kernels (esvio_fe_bow_create_vocabulary), a table of their own in timer slots behind every other;
 * the other tables stay as they are (the stable sorts are booked as k_radix_pass of the TRACK table, the document counts'
 * walk as k_bow_walk of loop detection's).  esvio_fe_bow_create_kernel_name: "" for any other id.
 * esvio_fe_bow_create_pick: C2's pick alone, on the device, with chosen numbers — min_dist [n] (n in 1..2^24), n_seg
 * segments seg_off[0..n_seg] ascending inside 0..n, one cut_d per segment; pick[s] = the first rank inside segment s
 * whose running sum of min_dist, as a double, is >= cut_d[s], the segment's last rank if none, 0xffffffff for an empty
 * segment or a cut_d that is not >= 0.  Host arrays. */
int esvio_fe_bow_create_kernel_count(void);
const char* esvio_fe_bow_create_kernel_name(int which);
int esvio_fe_bow_create_kernel_stats(esvio_fe_handle h, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
int esvio_fe_bow_create_pick(esvio_fe_handle h, const uint32_t* min_dist, int64_t n, const uint32_t* seg_off, int32_t n_seg,
                             const double* cut_d, uint32_t* pick);
/* the text stage (esvio_fe_decode_text): tile_bytes, the bytes of the virtual stream — the carried tail, then the chunk —
 * one workgroup owns the line starts of; max_body, the longest body that is not malformed; max_tail, the longest tail a
 * call leaves.  Its three kernels, k_text_count, k_text_place, k_text_emit, have a table of their own in timer slots
 * behind every other; esvio_fe_text_kernel_name: "" for any other id; _stats as esvio_fe_get_kernel_stats. */
typedef struct esvio_fe_text_limits_info {
  int32_t tile_bytes;
  int32_t max_body;
  int32_t max_tail;
  int32_t reserved;
} esvio_fe_text_limits_info;
int esvio_fe_text_limits(esvio_fe_text_limits_info* out);
int esvio_fe_text_kernel_count(void);
const char* esvio_fe_text_kernel_name(int which);
int esvio_fe_text_kernel_stats(esvio_fe_handle h, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes);
/* the events one workgroup of the slicing chain takes (esvio_fe_slice_events): where its tile edges lie */
int esvio_fe_slice_tile_events(void);
/* The ingest chains' top scans: reduce per tile -> ONE workgroup scans the tiles' summaries -> emit per tile.  A lane of that
 * workgroup owns ceil(tiles / lanes) consecutive tiles, so a call of more tiles than lanes is where a lane folds several
 * summaries, lanes own none, and the last lane's run must still be the whole call.  Per chain, the lanes: raw, k_raw_scan
 * (esvio_fe_decode_raw, _decode_triggers, _track_raw; tile: esvio_fe_raw_tile_bytes); aedat, k_aedat_scan (tile:
 * esvio_fe_aedat_tile_events); text, k_text_place (tile: esvio_fe_text_limits); slice, k_slice_scan (tile:
 * esvio_fe_slice_tile_events); filter, k_baf_scan, over blocks of filter_block_events events; pick, k_voc_scan_top
 * (esvio_fe_bow_create_pick), over tiles of pick_tile_values values. */
typedef struct esvio_fe_scan_lanes_info {
  int32_t raw;
  int32_t aedat;
  int32_t text;
  int32_t slice;
  int32_t filter;
  int32_t pick;
  int32_t filter_block_events;
  int32_t pick_tile_values;
} esvio_fe_scan_lanes_info;
int esvio_fe_scan_lanes(esvio_fe_scan_lanes_info* out);
/* The shared stable sort alone (k_radix_pass through the one driver every stage's passes follow): keys[n] / vals[n] (host)
 * sorted by the low passes * bits bits of the keys in `passes` stable passes of `bits` bits each — bits in 1..8, passes in
 * 1..4, n below 2^30, else ESVIO_FE_EINVAL.  n_dev = -1: n is the count.  n_dev >= 0: the value is placed in device memory
 * and passed as the device-side count, the launch stays sized for n and the first min(n, n_dev) pairs take part.  The
 * pairs and the sort scratch are the call's own device memory, freed before it returns; the digit histograms are counted
 * on the host from the keys that take part, the tickets and look-back words cleared.  The passes go to and fro between
 * two device buffers per array: the first starts as the whole input, the second as the caller's out_keys / out_vals, so
 * a position no pass wrote comes back as it went in — at and beyond a device count the result holds the caller's out_*
 * values behind an odd number of passes, the input pairs where they lay behind an even one.  out_keys / out_vals [n]: the
 * buffer that holds the result; *out_err: the expired-wait flag the passes raise; out_tickets[passes]: the blocks that
 * took a ticket in each pass.  n = 0 launches nothing. */
int esvio_fe_sort_pairs(esvio_fe_handle h, const uint32_t* keys, const uint32_t* vals, int64_t n, int passes, int bits,
                        int64_t n_dev, uint32_t* out_keys, uint32_t* out_vals, int32_t* out_err, uint32_t* out_tickets);
/* the hipStream_t the handle launches on (as void*) */
void* esvio_fe_stream(esvio_fe_handle h);
/* hipMemGetInfo on the handle's device, through the HIP runtime the library itself is linked to */
int esvio_fe_device_memory(esvio_fe_handle h, size_t* free_bytes, size_t* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ESVIO_FE_TEST_H */
