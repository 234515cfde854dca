/*
 * esvio_fe.h — C ABI of the MI355X-native ESVIO event front-end (libesvio_fe.so).
 *
 * Drop-in boundary for the hot path of arclab-hku/ESVIO's `feature_tracker` event node:
 * the calls FeatureTracker::trackEvent makes into esvio::EventDetector and OpenCV, and the
 * result vectors the ROS node reads back.  The reference has no FFI of its
 * own; each entry point below names the reference interface it replaces (file:line relative
 * to the reference tree).  Plain pointers and sizes only — no C++/torch types.
 *
 * Threading: one caller per handle (the reference has exactly one worker thread,
 * feature_tracker/src/stereo_event_tracker_node.cpp:366).  Different handles are independent
 * (one per GPU / per rig).  All functions return 0 on success, <0 on error
 * (see ESVIO_FE_E*), never abort; esvio_fe_last_error() gives a message.
 *
 * Every compute entry point runs hand-written HIP kernels on the handle's device; there is no
 * CPU fallback — creating a handle without a usable GPU fails with ESVIO_FE_ENODEVICE.
 */
#ifndef ESVIO_FE_H
#define ESVIO_FE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESVIO_FE_OK 0
#define ESVIO_FE_EINVAL (-1)      /* bad argument / unsupported config value */
#define ESVIO_FE_ENODEVICE (-2)   /* no usable HIP device */
#define ESVIO_FE_EHIP (-3)        /* HIP runtime error */
#define ESVIO_FE_ENOTIMPL (-4)    /* config asks for a stage that is not built yet */
#define ESVIO_FE_EINTERNAL (-5)   /* device-side invariant violated (bounded spin expired …) */

/* dvs_msgs::Event as laid out in memory (feature_tracker/src/dvs_msgs/Event.h:42-52):
 * uint16 x; uint16 y; ros::Time ts {uint32 sec; uint32 nsec}; uint8 polarity => 16 B AoS.
 * A `std::vector<dvs_msgs::Event>::data()` pointer can be passed as-is. */
typedef struct esvio_fe_event {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity;
  uint8_t _pad[3];
} esvio_fe_event;

/* camodocal pinhole + radtan parameters (camera_model/src/camera_models/PinholeCamera.cc) */
typedef struct esvio_fe_camera {
  double fx, fy, cx, cy, k1, k2, p1, p2;
} esvio_fe_camera;

/* The YAML knobs readParameters_event loads into globals
 * (feature_tracker/src/parameters.cpp:183-282), as one plain struct. */
typedef struct esvio_fe_config {
  int32_t width, height;            /* event_width / event_height -> COL_event, ROW_event */
  double decay_ms;                  /* decay_ms */
  int32_t ignore_polarity;          /* ignore_polarity */
  int32_t median_blur_kernel_size;  /* k: cv::medianBlur(2k+1) of each surface; 0 in every shipped config; k <= 7 */
  double feature_filter_threshold;  /* feature_filter_threshold [s] */
  double ts_lk_threshold;           /* TS_LK_threshold (128.0) */
  int32_t max_cnt;                  /* max_cnt */
  int32_t min_dist;                 /* min_dist */
  int32_t flow_back;                /* flow_back */
  int32_t equalize;                 /* equalize: 1 = CLAHE(40, 8x8) + normalize(0,255) before LK */
  double f_threshold;               /* F_threshold [px] */
  int32_t f_ransac;                 /* 1: run rejectWithF_event's RANSAC on host; 0: skip */
  int32_t lk_accum;                 /* how calcOpticalFlowPyrLK's sums are accumulated: 2 = in float in the
                                     * order of OpenCV 4.2's x86 SIMD128 build, i.e. the reference's own build
                                     * (restated from recall) — the default of every caller in this repository;
                                     * 1 = exactly (int64 sums; 0.65-0.8x the LK time, not that build's
                                     * arithmetic: within 1e-4 px of it on ~97 % of the points) */
  int32_t focal_length;             /* FOCAL_LENGTH, 460 (parameters.cpp:274) */
  int32_t device;                   /* HIP device ordinal, -1 = current device */
  esvio_fe_camera cam[2];           /* event_left_calib / event_right_calib */
} esvio_fe_config;

/* What stereo_event_tracker_node.cpp:289-322 reads from FeatureTracker after trackEvent.
 * Caller-owned buffers, each sized for max_cnt entries (xy arrays: 2*max_cnt floats). */
typedef struct esvio_fe_tracks {
  int32_t n_left;             /* ids.size() */
  int32_t n_right;            /* ids_right.size() */
  int32_t* ids;               /* FeatureTracker::ids */
  int32_t* track_cnt;         /* ::track_cnt */
  float* cur_pts;             /* ::cur_pts (u,v) */
  float* cur_un_pts;          /* ::cur_un_pts */
  float* pts_velocity;        /* ::pts_velocity */
  int32_t* ids_right;         /* ::ids_right */
  float* cur_right_pts;       /* ::cur_right_pts */
  float* cur_un_right_pts;    /* ::cur_un_right_pts */
  float* right_pts_velocity;  /* ::right_pts_velocity */
} esvio_fe_tracks;

typedef struct esvio_fe_ctx* esvio_fe_handle;

/* ---- lifetime ------------------------------------------------------------------------ */
/* replaces: global `esvio::EventDetector detector` (feature_tracker.cpp:7), `trackerData`
 * (stereo_event_tracker_node.cpp:45), EventDetector::init (event_detector.cc:47-70). */
/* Limits (ESVIO_FE_EINVAL beyond them): 42 <= width, height <= 8192; 1 <= max_cnt <= 65536;
 * 3 <= min_dist <= 63; median_blur_kernel_size <= 7.  Up to ~1.3 M pixels (1280x960) the greedy
 * corner selections keep their one-bit-per-pixel map in LDS; above that (the frame cameras of the
 * shipped ESVIO configs go up to 1920x1200) the map lives in device memory: same results, a slower
 * selection. */
int esvio_fe_create(const esvio_fe_config* cfg, esvio_fe_handle* out);
int esvio_fe_destroy(esvio_fe_handle h);
/* Clears SAE planes, images, tracks and ids as a freshly created handle (n_id keeps counting).
 * NOT what the reference does on a stream discontinuity: stereo_event_tracker_node.cpp:163-173 only
 * re-arms the node's own flags and publishes `restart`, the tracker keeps everything — a drop-in
 * caller does not call this there (tools/replay_node.cpp, esvio_amd/node.py). */
int esvio_fe_reset(esvio_fe_handle h);
const char* esvio_fe_last_error(esvio_fe_handle h);
const char* esvio_fe_version(void);

/* ---- EventDetector stages ------------------------------------------------------------ */
/* memory space of an event pointer argument */
#define ESVIO_FE_HOST 0
#define ESVIO_FE_DEVICE 1

/* createSAE_left (cam 0, event_detector.cc:149-166) / createSAE_right (cam 1, :212-228)
 * applied to n events in stream order.  Events with x>=width or y>=height are skipped and
 * counted in *n_rejected (the reference would abort on an Eigen assert). */
int esvio_fe_create_sae(esvio_fe_handle h, int cam, const esvio_fe_event* ev, size_t n,
                        int space, uint64_t* n_rejected);
/* both cameras in one submission (what trackEvent does at feature_tracker.cpp:356-362) */
int esvio_fe_create_sae_stereo(esvio_fe_handle h, const esvio_fe_event* left, size_t nL,
                               const esvio_fe_event* right, size_t nR, int space,
                               uint64_t* n_rejected);
/* SAEtoTimeSurface_left/right (event_detector.cc:230-305).  Renders the camera's time surface
 * (and, with equalize, the CLAHE+normalize image trackEvent derives from it, feature_tracker.cpp:
 * 375-382) into the handle; if out != NULL also copies the raw width*height u8 surface to host. */
int esvio_fe_sae_to_time_surface(esvio_fe_handle h, int cam, double external_sync_time,
                                 uint8_t* out);
/* isCorner (event_detector.cc:308-544) for n events against the LEFT planes; flags[i] in {0,1}
 * (host buffer).  Out-of-sensor events give 0. */
int esvio_fe_is_corner(esvio_fe_handle h, const esvio_fe_event* ev, size_t n, int space,
                       uint8_t* flags);
/* Event_FeaturesToTrack (feature_tracker.cpp:13-38): greedy scan of `ev` in stream order.
 * mask: width*height bytes on host, 255 = blocked (the reference's CV_64F 255.0), may be NULL.
 * Uses the handle's current left time surface for the TS_LK_threshold test.  Writes up to
 * max_corners (x,y) pairs and (optionally) their event indices. */
int esvio_fe_features_to_track(esvio_fe_handle h, const esvio_fe_event* ev, size_t n, int space,
                               int max_corners, const uint8_t* mask, float* out_xy,
                               int32_t* out_idx, int32_t* n_out);
/* read-out of a camera's four planes (each width*height doubles, index x + y*width): what the reference's
 * private sae_[2] / sae_latest_[2] (event_detector.h) hold; the write side (tests) is esvio_fe_set_sae in
 * esvio_fe_test.h */
int esvio_fe_get_sae(esvio_fe_handle h, int cam, double* L0, double* L1, double* S0, double* S1);

/* ---- OpenCV stages used by trackEvent ------------------------------------------------- */
#define ESVIO_FE_LK_USE_INITIAL_FLOW 4 /* cv::OPTFLOW_USE_INITIAL_FLOW */
/* cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(21,21), max_level,
 * TermCriteria(COUNT+EPS, max_count, eps), flags) as called at feature_tracker.cpp:410,417,
 * 490,495.  Host u8 images of w*h (w,h need not equal the config's sensor size). */
int esvio_fe_calc_optical_flow_pyr_lk(esvio_fe_handle h, const uint8_t* prev_img,
                                      const uint8_t* next_img, int w, int hgt,
                                      const float* prev_pts, float* next_pts, uint8_t* status,
                                      int n, int max_level, int max_count, double eps, int flags);
/* cv::findFundamentalMat(p1, p2, FM_RANSAC, thr, conf, status) as used by rejectWithF_event
 * (feature_tracker.cpp:935); host-side. Returns the inlier count in *n_inliers. */
int esvio_fe_find_fundamental_mat(const float* p1, const float* p2, int n, double thr,
                                  double conf, uint8_t* status, int32_t* n_inliers);

/* ---- the fused per-frame call -------------------------------------------------------- */
/* FeatureTracker::trackEvent(cur_time, event_left, event_right) (feature_tracker.cpp:340-603)
 * with PUB_THIS_FRAME passed explicitly (global at parameters.cpp:276, set by
 * stereo_event_tracker_node.cpp:177-188).  nL must be > 0 (node:150 returns early otherwise).
 * `out` may be NULL. */
int esvio_fe_track_event(esvio_fe_handle h, double cur_time, const esvio_fe_event* left,
                         size_t nL, const esvio_fe_event* right, size_t nR, int space,
                         int pub_this_frame, esvio_fe_tracks* out);
/* The fields of Motion_correction_value (event_detector.h:16) that createSAE_left/right with
 * motion compensation read (event_detector.cc:102-147,168-210), as handle_stereo_event fills them
 * (stereo_event_tracker_node.cpp:192-254), plus the K that detector.init(COL,ROW,fx,fy,cx,cy)
 * receives (feature_tracker.cpp:616; the fx,fy,cx,cy globals of parameters.cpp:222-225). */
typedef struct esvio_fe_motion {
  double t1;       /* event_left.header.stamp.toSec() (feature_tracker.cpp:622) */
  double v[3];     /* State_[0..2]: current linear velocity (node:215-217) */
  float v_pre[3];  /* previous velocity (node:220-222) */
  float accel[3];  /* temp_a (node:230-232); the warp is applied when |accel| > 5 m/s^2 */
  float omega[3];  /* IMU angular velocity (node:244-246) */
  double fx, fy, cx, cy;
} esvio_fe_motion;

/* FeatureTracker::trackEvent(cur_time, event_left, event_right, measurements)
 * (feature_tracker.cpp:605-877, configs with Do_motion_correction: 1): events of the first part of
 * the batch are warped to the batch start before the SAE update; everything else as
 * esvio_fe_track_event. */
int esvio_fe_track_event_mc(esvio_fe_handle h, double cur_time, const esvio_fe_event* left,
                            size_t nL, const esvio_fe_event* right, size_t nR, int space,
                            int pub_this_frame, const esvio_fe_motion* motion,
                            esvio_fe_tracks* out);
/* the createSAE_left/right(…, measurements) loops alone (feature_tracker.cpp:627-641) */
int esvio_fe_create_sae_stereo_mc(esvio_fe_handle h, const esvio_fe_event* left, size_t nL,
                                  const esvio_fe_event* right, size_t nR, int space,
                                  const esvio_fe_motion* motion, uint64_t* n_rejected);

/* Throughput (replay) mode: announce the batch the FOLLOWING esvio_fe_track_event call will be
 * given.  The current call then enqueues that batch's SAE update, time surfaces and pyramids on a
 * second HIP stream as soon as the current frame has finished reading the SAE planes, so they overlap
 * the current frame's LK / selection and the host work between calls.  `pub_hint` is the
 * PUB_THIS_FRAME the caller expects to pass with that batch (the node's frequency control depends
 * on timestamps only, stereo_event_tracker_node.cpp:177-188): when non-zero the batch's Arc* pass
 * is prefetched as well; a wrong hint costs time, never correctness.  The following call must
 * pass exactly these pointers, sizes, space and cur_time (else ESVIO_FE_EINVAL) and the event memory
 * must stay valid until then.  Results are identical to the non-pipelined sequence.  After a call
 * that prefetched, the get_sae / time-surface taps already reflect the latest prefetched batch.
 * Up to three batches are taken up ahead of their track calls (the calls that follow must come in
 * the announced order): the later ones' SAE updates then run whole frames early; up to six may be
 * announced and not yet tracked (ESVIO_FE_EINVAL beyond).  Batches in ESVIO_FE_HOST memory start on their way to the
 * device inside this call: helper threads copy them into pinned chunks and enqueue the DMAs on a copy
 * stream of the handle (ESVIO_FE_STAGE_THREADS, default 2; a pinned source is DMA'd as it is), and a
 * track call takes up an announced batch only once that is done — so announce host batches one call
 * further ahead than device batches.  With more than one batch in flight the hint of a published frame must be exact
 * (the SAE has moved on by the time it is tracked): a published frame whose hint was 0 is refused
 * with ESVIO_FE_EINVAL.  With two batches' pyramids in flight and a next frame that publishes
 * nothing (hint 0: no new corners, no RANSAC — the frame after it tracks exactly its forward LK
 * results) the temporal LK of the frame AFTER next is launched together with the next frame's,
 * chained to it point by point on the device; a wrong hint only discards that launch.
 * The reference has no counterpart: it processes one batch at a time (depth-1 queues,
 * node:128-142). */
int esvio_fe_set_next_batch(esvio_fe_handle h, double next_cur_time, const esvio_fe_event* left,
                            size_t nL, const esvio_fe_event* right, size_t nR, int space,
                            int pub_hint);
/* The same for a batch that esvio_fe_track_event_mc will be given (configs with
 * Do_motion_correction: 1): the Motion_correction_value the node has assembled for it travels with the
 * announcement (copied), the following esvio_fe_track_event_mc call must pass the same values. */
int esvio_fe_set_next_batch_mc(esvio_fe_handle h, double next_cur_time, const esvio_fe_event* left,
                               size_t nL, const esvio_fe_event* right, size_t nR, int space,
                               int pub_hint, const esvio_fe_motion* motion);

/* ---- image front-end: FeatureTracker::trackImage ------------------------ */
/* For this path the handle is the image tracker's own instance (stereo_image_tracker_node.cpp:31):
 * width/height = image_width/image_height (parameters.cpp:103-104), max_cnt = max_cnt_img,
 * min_dist = min_dist_img (:100-102); equalize = the node's CLAHE (node:92-96).
 *
 * cv::goodFeaturesToTrack(img, corners, max_corners, quality, min_distance, mask) as trackImage
 * calls it (feature_tracker.cpp:228: blockSize 3, gradientSize 3, Shi-Tomasi) [OpenCV, restated].
 * img: width*height bytes (host); mask: width*height bytes, nonzero = allowed, or NULL;
 * 1 <= max_corners <= max_cnt; out_xy: 2*max_corners floats; eig_out (optional): the
 * cornerMinEigenVal map, width*height floats. */
int esvio_fe_good_features_to_track(esvio_fe_handle h, const uint8_t* img, int max_corners,
                                    double quality, double min_distance, const uint8_t* mask,
                                    float* out_xy, int32_t* n_out, float* eig_out);
/* FeatureTracker::trackImage(cur_time, img_left, img_right) (feature_tracker.cpp:164-338), host
 * images of width*height bytes; img_right may be NULL (the right block is then skipped like the
 * reference's `!img_right.empty()` test).  Results as esvio_fe_track_event. */
int esvio_fe_track_image(esvio_fe_handle h, double cur_time, const uint8_t* img_left,
                         const uint8_t* img_right, int pub_this_frame, esvio_fe_tracks* out);

/* The node's PointCloud packing of the current results (stereo_event_tracker_node.cpp:273-329):
 * out = 2*max_cnt rows of 8 floats (x_un, y_un, 1, id*2+cam as float32, u, v, vx, vy): left entries
 * with track_cnt > 1, then right entries whose id is among them, then padding rows with id -1.
 * This fixed-size block is the unit the multi-GPU all_gather exchanges. */
int esvio_fe_pack_track_records(esvio_fe_handle h, float* out, int32_t* n_rows);

/* The north-star's merge step from C/C++: one ncclAllGather (RCCL over xGMI) of this handle's
 * esvio_fe_pack_track_records block over `nccl_comm` (a ncclComm_t of `world` ranks whose rank uses
 * this handle's device), enqueued on the handle's stream; `gathered` (host) receives
 * world x 2*max_cnt x 8 floats, rank by rank, on every rank.  19.2 KB per rank at max_cnt 300:
 * latency-bound, xGMI bandwidth is irrelevant.  RCCL is dlopen'ed on first use
 * (ESVIO_FE_ENOTIMPL if librccl.so cannot be found).  Replaces: the ROS topic hop of
 * stereo_event_tracker_node.cpp:340 when several GPUs feed one estimator. */
int esvio_fe_exchange_tracks(esvio_fe_handle h, void* nccl_comm, int world, float* gathered);
/* The same exchange without a stop on the caller's thread, over a communicator the handle owns:
 * rank 0 makes an id (esvio_fe_comm_unique_id = ncclGetUniqueId) and passes it to the other ranks by
 * whatever side channel the launcher has; every rank calls esvio_fe_comm_init once
 * (ncclCommInitRank).  esvio_fe_exchange_begin packs the current frame's records and enqueues
 * upload + ncclAllGather + download on a stream of its own — it returns at once, the next frames'
 * kernels run beside it; esvio_fe_exchange_end waits for the latest begun exchange and copies the
 * world x 2*max_cnt x 8 floats out (gathered may be NULL: wait only).  One exchange in flight:
 * begin waits for the previous one. */
int esvio_fe_comm_unique_id(uint8_t id[128]);
int esvio_fe_comm_init(esvio_fe_handle h, const uint8_t id[128], int rank, int world);
int esvio_fe_exchange_begin(esvio_fe_handle h);
int esvio_fe_exchange_end(esvio_fe_handle h, float* gathered);
/* With `on`, every esvio_fe_track_event call with pub_this_frame != 0 exchanges its records by itself:
 * they are packed at the end of that call and the upload / ncclAllGather / download are enqueued by
 * the NEXT call at the point where it waits for its temporal LK anyway (or at its end), so the
 * exchange costs the calling thread no time of its own.  esvio_fe_exchange_end returns the latest
 * one (enqueuing it first if the next call has not come yet).  Every rank must publish the same
 * frames (the node's frequency control reads timestamps only). */
int esvio_fe_set_auto_exchange(esvio_fe_handle h, int on);

/* Throughput option: with `on`, a published esvio_fe_track_event call returns without waiting for
 * the stereo LK of the corners it has just detected.  Everything else in its results is complete
 * (the node's PointCloud never contains corners of track_cnt 1, node:289); the right-camera entries
 * of those new corners (ids_right / cur_right_pts / cur_un_right_pts / right_pts_velocity tails) are
 * appended by a later call's right-camera bookkeeping — the next call's, or, when that call itself
 * returns lazily while their stereo LK is still running, the one after it: always before they can
 * influence anything — or by esvio_fe_finish, after which the state is bit-identical to the eager sequence.
 * A call with pub_this_frame == 0 (the node publishes nothing of it, stereo_event_tracker_node.cpp
 * :262) returns without waiting for its stereo LK at all: its left-camera members are complete, its
 * right-camera members (feature_tracker.cpp:475-575) still show the previous frame until the next
 * call, esvio_fe_finish or esvio_fe_pack_track_records completes them, again bit-identically. */
int esvio_fe_set_lazy_new_stereo(esvio_fe_handle h, int on);
/* Throughput option: rejectWithF_event's RANSAC (feature_tracker.cpp:935, ~100-350 iterations of
 * the 7-point solver per published frame, on the frame's critical path) uses `threads` host threads
 * (1 = the calling thread only, the default; at most 16).  The helpers only solve and score
 * iterations; the cv::RNG draws and the best-model bookkeeping stay sequential on the calling
 * thread, so the result is bit-identical for any thread count.  Helpers spin while frames keep
 * coming and sleep after 2 ms without work. */
int esvio_fe_set_host_threads(esvio_fe_handle h, int threads);
/* Throughput option for replay mode: with `on`, the HIP calls that start an announced batch's SAE update,
 * rendering, pyramids and Arc* pass (~10 launches and event calls, 35-45 us of host time per batch) are
 * issued by a thread of the handle instead of by the calling thread — the calling thread, which bounds
 * the replay rate, keeps only the bookkeeping and checks that a batch's job has been issued before it
 * consumes that batch (three frames later in the steady state).  Results do not depend on it.  The
 * thread spins while batches keep coming and blocks after 2 ms without one: one more busy CPU. */
int esvio_fe_set_launch_thread(esvio_fe_handle h, int on);
/* complete a lazily returned frame (no-op otherwise) and copy the result members into `out` */
int esvio_fe_finish(esvio_fe_handle h, esvio_fe_tracks* out);

/* FeatureTracker::gettimesurface() tap (feature_tracker.cpp:894): current left/right image */
int esvio_fe_get_time_surface(esvio_fe_handle h, int cam, uint8_t* out);

/* ---- FAST corners on the time surface --------------------------------------------------- */
/* fast::fast_corner_detect_9 / fast_corner_detect_10, fast_corner_score_10 and fast_nonmax_3x3 of the FAST
 * detector the reference vendors (dependences/fast_neon-master/include/fast/fast.h:22-47; the plain C++
 * functions, not the SSE2 / NEON ones) — the common alternative to Arc* in event front-ends, on the image
 * where it already lies.  (The reference's own FAST pass over the published time surface,
 * pose_graph/src/keyframe.cpp:138, is cv::FAST: other scores, another non-max; not this.)
 * Integer-only and exact: this stage is tested against outputs of the reference's compiled code.
 *
 * img == NULL: the handle's current time surface of camera `cam` — the plane esvio_fe_get_time_surface
 * returns — read in place on the device.  Otherwise img is width*height bytes of the handle's own size in
 * `space` (ESVIO_FE_HOST: copied to the device first; ESVIO_FE_DEVICE: read in place) and `cam` is ignored.
 * arc: 9 or 10.  barrier: 0..255 (a ring pixel counts when it differs from the centre by MORE than barrier).
 * nonmax 0: every detected corner; out_score (optional) = fast_corner_score_10, arc 10 only.
 * nonmax 1: the survivors of fast_nonmax_3x3 over score_10 (corners[idx[i]] of the library), arc 10 only.
 * The library has no score for arc 9: arc 9 with nonmax or out_score is ESVIO_FE_EINVAL.
 * Corners come in the library's order, raster order (y, then x): out_xy[2*i] = x, out_xy[2*i + 1] = y.
 * *n_out is always the full count; at most `capacity` entries — the first ones — are written, and the call
 * returns ESVIO_FE_OK either way: *n_out > capacity means "call again with room for *n_out".
 * *n_detected (optional): the count before non-max.
 * The call orders itself after the work that renders the plane it reads, waits for its own results and
 * touches nothing of the tracker: made between two esvio_fe_track_event calls (announced batches or not)
 * it changes no later result.  Its scratch (17 bytes per pixel) is allocated by the first call. */
int esvio_fe_fast_corners(esvio_fe_handle h, int cam, const uint8_t* img, int space, int arc, int barrier,
                          int nonmax, int16_t* out_xy, int32_t* out_score, int32_t capacity,
                          int32_t* n_out, int32_t* n_detected);

/* ---- FAST as trackEvent's detector --------------------------------------------------------- */
/* Where esvio_fe_track_event (both overloads, esvio_fe_track_event_fields, announced batches) takes a published
 * frame's NEW corners from.  The reference has one detector, Arc*, and no counterpart to the other: this text is
 * its specification. */
#define ESVIO_FE_DETECT_ARC  0   /* Event_FeaturesToTrack + isCorner: the reference, the default */
#define ESVIO_FE_DETECT_FAST 1   /* FAST-10 + score_10 + nonmax_3x3 on the left time surface, score-ordered */
/* ESVIO_FE_DETECT_FAST, for an image, a mask of blocked pixels and a budget max_corners:
 *  1. C = the corners esvio_fe_fast_corners(arc 10, nonmax 1, barrier) returns for the image, with their
 *     fast_corner_score_10.
 *  2. C is ordered by score, descending; corners of equal score stay in raster order (y, then x, ascending).
 *     (Raster order fed to a greedy scan would fill the budget from the top rows; cv::goodFeaturesToTrack orders by
 *     response for the same reason.)
 *  3. The scan of Event_FeaturesToTrack (feature_tracker.cpp:13-38) over that list, from a working copy of the mask:
 *     a corner whose pixel is blocked in the working mask is skipped; so is one whose image byte equals
 *     (uint8_t)ts_lk_threshold; any other is accepted as ((float)x, (float)y) and the filled cv::circle of radius
 *     min_dist around it is blocked — the disc the Arc* selection stamps, not goodFeaturesToTrack's Euclidean
 *     one; the scan stops at max_corners accepted corners.
 * In trackEvent the image is the batch's raw left time surface (after median_blur_kernel_size, before CLAHE: the
 * plane the TS_LK_threshold test reads and esvio_fe_get_time_surface returns), the mask is Event_setMask's and
 * max_corners = max_cnt - kept points.  Everything else in the call — tracking, filters, ids, the stereo LK, lazy
 * returns, the exchange — is what it is with Arc*, and so is every schedule: with a non-zero pub_hint an announced
 * batch's FAST pass is prefetched as its Arc* pass would be.  esvio_fe_track_image ignores the setting.
 *
 * detector: one of the two above; fast_barrier: 0..255 (ignored for ESVIO_FE_DETECT_ARC).  ESVIO_FE_EINVAL for
 * other values, and while batches are announced and not yet tracked (as esvio_fe_reserve).  The call waits for the
 * handle's streams and, for ESVIO_FE_DETECT_FAST, allocates everything the FAST passes need (about 35 bytes per
 * pixel, and room for one candidate per pixel in every candidate set): no later track call allocates for them.  The setting survives esvio_fe_reset. */
int esvio_fe_set_detector(esvio_fe_handle h, int detector, int fast_barrier);
/* The stage tap beside esvio_fe_features_to_track: steps 1-3 above for one image.
 * img == NULL: the handle's current raw left time surface, read in place; otherwise width*height bytes of the
 * handle's size in `space`, as in esvio_fe_fast_corners.  barrier: 0..255.  mask: width*height bytes on host,
 * 255 = blocked, may be NULL.  max_corners <= max_cnt; <= 0 selects nothing.  Writes the accepted corners' (x,y)
 * pairs to out_xy, (optionally) their scores to out_score, their number to *n_out and (optionally) the size of C —
 * the survivors of the non-max before any mask or threshold test, esvio_fe_fast_corners' *n_out — to
 * *n_candidates.  min_dist and ts_lk_threshold are the handle's.
 * The call runs on the handle's main stream in scratch of its own, waits for its own result and touches nothing of
 * the tracker: made between two track calls (announced batches or not) it changes no later result. */
int esvio_fe_features_to_track_fast(esvio_fe_handle h, const uint8_t* img, int space, int barrier,
                                    int max_corners, const uint8_t* mask, float* out_xy,
                                    int32_t* out_score, int32_t* n_out, int32_t* n_candidates);

/* ---- event layouts: caller-layout arrays -> event records, on the device ------------------ */
/* Recordings (DSEC, MVSEC, VECtor, ECMD) and vendor SDKs deliver events as separate arrays (x[], y[], p[], t[] in
 * microseconds plus a file-wide offset) or as records with a 64-bit stamp, some of them packed; only a ROS host holds
 * dvs_msgs::Event records.  The reference has no counterpart: it only ever sees ROS records — this layout support is
 * the project's own.  esvio_fe_event_fields says where the four fields of event i lie: field + i * stride, at any
 * alignment.  It expresses separate arrays (strides 2, 2, 4 or 8, 1), an aligned AoS record (one base, four offsets,
 * stride 16) and a packed AoS record (stride 13, say, where the 8-byte stamp is unaligned). */
typedef struct esvio_fe_event_fields {
  const void *x, *y, *t, *p;                      /* field of event 0 */
  int32_t x_stride, y_stride, t_stride, p_stride; /* bytes from event i to event i+1 (>= the field's width) */
  int32_t t_bits;     /* 32: unsigned; 64: signed */
  int32_t t_unit_ns;  /* 1 or 1000 (ns or us ticks) */
  int32_t p_bits;     /* 8 or 16, read as SIGNED: polarity = (value > 0), so {0,1} and {-1,+1} both work */
  int64_t t_offset;   /* added to every t, in ticks; |t_offset| <= 2^62 */
} esvio_fe_event_fields;
/* n records into dst (ESVIO_FE_DEVICE: device memory, 16-byte aligned — esvio_fe_mem_alloc's is; ESVIO_FE_HOST: the
 * records are downloaded), exact in integers: x and y (16 bits) are copied as bit patterns (an out-of-sensor value is
 * the SAE update's business: it skips and counts those); ticks = t + t_offset, tps = 10^9 / t_unit_ns,
 * sec = ticks / tps, nsec = (ticks % tps) * t_unit_ns; polarity 0 or 1; the padding bytes 0 — byte for byte what
 * esvio_amd.events.make_events builds on the host.
 * An event is BAD when ticks < 0, when sec >= 2^32, or when a 64-bit t lies outside +-2^62.  Bad events are counted
 * on the device, nothing is clamped: if there is one, the call returns ESVIO_FE_EINVAL with *n_bad (optional) exact
 * and dst unspecified.  n == 0 succeeds and touches nothing.  Descriptor errors (bits or unit outside the lists
 * above, a stride below the field's width, a null field with n > 0, |t_offset| > 2^62) are ESVIO_FE_EINVAL with a
 * message and happen before anything else does.
 * src_space says where the FIELDS lie.  ESVIO_FE_DEVICE: read in place.  ESVIO_FE_HOST: page-locked memory the
 * library's runtime knows (esvio_fe_mem_alloc, esvio_fe_register_host_buffer) is read in place by the kernel, over
 * PCIe (records of 2^20 events and more are copied first: measured faster, KERNELS.md "Event layouts"); pageable
 * memory is copied into scratch of the handle first — the bytes the fields span, not 16 per event
 * (9 or 13 for separate arrays) — and converted there.  That scratch and the buffer behind a host dst grow on first
 * use.
 * The call orders itself on the handle's main stream, waits for its own result and touches nothing of the tracker:
 * made between two track calls (announced batches or not) it changes no later result.  Records in a device dst can be
 * handed to every entry point that takes device events, esvio_fe_set_next_batch included. */
int esvio_fe_convert_events(esvio_fe_handle h, const esvio_fe_event_fields* src, size_t n, int src_space,
                            esvio_fe_event* dst, int dst_space, uint64_t* n_bad);
/* esvio_fe_track_event for a host that has fields, not records: both cameras are converted into device buffers of the
 * handle and the plain esvio_fe_track_event runs on those (ESVIO_FE_DEVICE).  A bad event fails the call
 * (ESVIO_FE_EINVAL) before anything is tracked; nL must be > 0.  Not to be mixed with esvio_fe_set_next_batch (convert
 * into memory of your own for that).
 * Buffer lifetime: a returned track call may still have kernels in flight that read its events — the SAE update of a
 * frame that had nothing to wait for (a first or an unpublished frame without points), the right camera's update on
 * the stereo stream, an Arc* pass beside the temporal LK; what lazy returns leave open (new-corner stereo, an
 * unpublished frame's stereo LK) reads images, not events.  So the handle keeps TWO pairs of buffers that alternate,
 * and a pair is rewritten, two calls later, behind everything that call had enqueued on any of the handle's streams
 * (events recorded when it returned; the wait is on the device and long over by then). */
int esvio_fe_track_event_fields(esvio_fe_handle h, double cur_time, const esvio_fe_event_fields* left, size_t nL,
                                const esvio_fe_event_fields* right, size_t nR, int src_space,
                                int pub_this_frame, esvio_fe_tracks* out);

/* ---- background-activity noise filter of an event batch, on the device -------------------- */
/* The reference's live path never sees raw sensor noise: its DAVIS driver switches the camera's hardware
 * background-activity filter on by default (dependences/rpg_dvs_ros/davis_ros_driver/cfg/DAVIS_ROS_Driver.cfg:28-29:
 * enabled, 80 x 250 us = 20 ms; src/driver.cpp:461-464), so every batch trackEvent gets over ROS has passed it.
 * Recordings, vendor SDKs and simulators hand over unfiltered streams.  That filter is FPGA logic: there is nothing
 * of the reference to be equal to, so — as for ESVIO_FE_DETECT_FAST and the event layouts — THIS TEXT IS THE
 * SPECIFICATION, and the kernels equal its sequential reading (tests/ba_filter_ref.py) exactly.
 *
 * Per handle and camera a plane B[x + y*width] holds, per pixel, either `none` or a stamp in integer nanoseconds.  A
 * fresh handle holds `none` everywhere.  (8 bytes per pixel and camera, allocated by the first filtering call: a
 * handle that never filters allocates nothing for it.)  For the events of one call, in stream order, i = 0 .. n-1:
 *  1. x >= width or y >= height: the event is REJECTED — counted in *n_rejected, flag 0, not emitted; it neither
 *     reads nor writes B.
 *  2. t = sec * 10^9 + nsec, exact in 64-bit integers; nsec is taken as it is, also when it is >= 10^9.
 *  3. support = the number of the 8 neighbour pixels (x+dx, y+dy), dx, dy in {-1,0,1}, not both 0, for which all of
 *     these hold: the pixel lies inside the sensor; B there is not `none`; t - B < window_ns as a SIGNED 64-bit
 *     difference (a neighbour stamped later than t has a negative difference and counts).  The event's own pixel
 *     never counts.  Polarity is ignored.
 *  3b. (esvio_fe_filter_batch, esvio_fe_track_batch: esvio_fe_filter_params.refractory_ns) own = B[x + y*width] as it
 *     is just before this event.  The event is REFRACTORY when all three hold: refractory_ns > 0; own is not `none`;
 *     t - own < refractory_ns as a SIGNED 64-bit difference (a pixel stamped later than t has a negative difference and
 *     counts, exactly as for neighbours).  A stamp of 0 is a stamp.
 *  4. keep_i = (support >= min_support).  With esvio_fe_filter_params:
 *     keep_i = (min_support == 0 || support >= min_support) && !refractory — min_support 0 skips steps 3 and 4's
 *     support test: every in-sensor event passes it.
 *  5. B[x + y*width] = t — always, kept or not.
 * The kept events are emitted in stream order, all 16 bytes of each record copied as they are.  B carries over from
 * call to call (the first events of a batch find the support the previous batch left).  An event stamped 0 supports
 * like any other: `none` is not stamp 0.  Nothing is assumed about the order of the stamps: non-monotonic stamps,
 * equal stamps and stamps stepping back a second give what the loop above gives.
 * Limits: 1 <= window_ns <= 2^62, 1 <= min_support <= 8.  With min_support 1 (and the strict <) this is the classic
 * software form of the filter (jAER's BackgroundActivityFilter; libcaer's dvsnoise with supportMin), restated from
 * recall: it is unpinned, and not claimed to be bit-equal to the DAVIS FPGA.  The sensor's refractory filter (off by
 * default in the reference's driver) is not part of it.
 * Steps 3b and 4's second form are that refractory filter in its software form, beside the background-activity filter
 * as in the reference's driver (DAVIS_ROS_Driver.cfg, off by default) and in every software noise filter (libcaer's
 * dvsnoise, jAER).  B is written by every in-sensor event — kept or not, refractory or not (step 5): ONE timestamp
 * map serves both tests, as libcaer's does, restated from recall like the rest: it is unpinned as well.  The
 * restatement is tests/ba_filter2_ref.py.  Old and new entry points on one handle advance the same planes.
 *
 * the filter stage: advances camera `cam`'s plane B by the n events of `ev` (space: ESVIO_FE_HOST — copied to the
 * device as they are, one copy — or ESVIO_FE_DEVICE, read in place) and writes the kept records, in order, to dst
 * (room for n records; ESVIO_FE_DEVICE: 16-byte aligned device memory, may be handed to every entry point that takes
 * device events, esvio_fe_set_next_batch included; ESVIO_FE_HOST: downloaded).  flags (optional, host, n bytes): keep_i.
 * *last_kept (optional): the last kept record (untouched if none).  n == 0 succeeds and touches nothing.
 * Orders itself on the main stream, waits for its own result, touches nothing of the tracker: made between two track
 * calls (announced batches or not) it changes no later tracking result.  Its scratch grows on first use (and with
 * esvio_fe_reserve, for a handle that has filtered before: the per-event scratch for max(max_left, max_right) events
 * and, with host_batches, the copy of a host source; the records behind a host dst grow on the first call that has
 * one): the second call of a size allocates nothing.
 * ESVIO_FE_EINVAL with a message, before any device work: window_ns or min_support outside the limits, cam outside
 * 0..1, a bad space, a null ev or dst with n > 0, a misaligned device dst, dst overlapping ev. */
int esvio_fe_filter_events(esvio_fe_handle h, int cam, const esvio_fe_event* ev, size_t n, int space,
                           int64_t window_ns, int min_support, esvio_fe_event* dst, int dst_space,
                           uint64_t* n_kept, uint8_t* flags, esvio_fe_event* last_kept, uint64_t* n_rejected);
/* The parameters of the rule above.  Limits: 0 <= min_support <= 8; 1 <= window_ns <= 2^62 unless min_support is 0
 * (then it is not read); 0 <= refractory_ns <= 2^62; reserved 0.  {window_ns, min_support, 0, 0} with min_support >= 1 is
 * esvio_fe_filter_events' rule, bit for bit. */
typedef struct esvio_fe_filter_params {
  int64_t window_ns;      /* 1..2^62; not read when min_support == 0 */
  int32_t min_support;    /* 0..8; 0: the support test (steps 3-4) is skipped, every in-sensor event passes it */
  int32_t reserved;       /* must be 0 */
  int64_t refractory_ns;  /* 0..2^62; 0: no refractory test */
} esvio_fe_filter_params;
/* the filter stage with esvio_fe_filter_params, on records (`ev`) or on caller-layout field arrays (`fields`): exactly
 * one of the two is non-null when n > 0, else ESVIO_FE_EINVAL.  Everything esvio_fe_filter_events states about dst,
 * flags, last_kept, n == 0, the ordering on the main stream, the scratch's growth, esvio_fe_reserve and argument errors
 * raised before any device work holds here unchanged (reserved != 0, a null prm and the limits above are such errors).
 * With ev: the kept records are copied whole, all 16 bytes, padding included.
 * With fields: `space` says where the FIELDS lie, with esvio_fe_convert_events' three source paths — device memory,
 * read in place; page-locked memory, read in place except records at or above 2^20 events; pageable memory, copied
 * once into the handle's scratch, only the bytes the fields span.  The 16-byte record of an event that is not kept is
 * never made: keys and stamps are computed from the fields, the kept records are built exactly as
 * esvio_fe_convert_events builds them, byte for byte, padding 0.  dst must not overlap a field.  An event that
 * conversion calls BAD fails the call with ESVIO_FE_EINVAL: *n_bad (optional) is exact, dst, flags and last_kept are
 * unspecified, CAMERA cam's PLANE IS AS IT WAS BEFORE THE CALL, and the next call works normally.  Descriptor errors
 * are esvio_fe_convert_events', raised before anything else.  (With ev, *n_bad is 0.) */
int esvio_fe_filter_batch(esvio_fe_handle h, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields,
                          size_t n, int space, const esvio_fe_filter_params* prm, esvio_fe_event* dst, int dst_space,
                          uint64_t* n_kept, uint8_t* flags, esvio_fe_event* last_kept, uint64_t* n_rejected,
                          uint64_t* n_bad);
/* all planes B back to `none` (esvio_fe_reset does the same as part of "as a freshly created handle") */
int esvio_fe_filter_reset(esvio_fe_handle h);
/* filter both cameras into buffers of the handle, then esvio_fe_track_event on the kept records with
 * cur_time = (double)sec + 1e-9 * (double)nsec of the last KEPT left event (what node:190 reads from a message the
 * sensor had already filtered); *cur_time_out (optional) returns it.  kept[0] == 0: nothing is tracked and nothing
 * of the tracker changes (node:150 returns early on an empty left message) — the call returns ESVIO_FE_OK, `out`
 * is untouched, both planes B have advanced.  Buffer lifetime and "not with announced batches" exactly as
 * esvio_fe_track_event_fields (two alternating pairs — the same two).
 * A caller whose publish decision reads the batch's last stamp (node:190-200 decides PUB_THIS_FRAME from the message's
 * last event) cannot know that stamp before the filter has run: it uses the two-step form — esvio_fe_filter_events
 * per camera into device memory with last_kept, decide, then esvio_fe_track_event on the device records. */
int esvio_fe_track_event_filtered(esvio_fe_handle h, const esvio_fe_event* left, size_t nL,
                                  const esvio_fe_event* right, size_t nR, int space, int64_t window_ns,
                                  int min_support, int pub_this_frame, esvio_fe_tracks* out,
                                  uint64_t kept[2], double* cur_time_out);

/* ---- the sensors' address filters and hot-pixel learning, on the device -------------------- */
/* The filter block the reference's drivers program into the camera has more members than the two above
 * (dependences/rpg_dvs_ros/davis_ros_driver/cfg/DAVIS_ROS_Driver.cfg:26-64, src/driver.cpp:403-488;
 * dvxplorer_ros_driver/cfg/DVXplorer_ROS_Driver.cfg:34-46): a pixel filter (eight silenced addresses, with
 * pixel_auto_train, "automatic filtering of 8 most active pixels"), a region of interest, polarity suppress / flatten.
 * Like the filter itself they are FPGA / sensor logic: there is nothing of the reference to be equal to, THIS TEXT IS
 * THE SPECIFICATION, the kernels equal its sequential reading (tests/addr_filter_ref.py) exactly.  Integers only.
 *
 * THE ADDRESS STAGE — step 1a of the filter rule above, between its steps 1 and 2.  An in-sensor event of camera cam
 * is REJECTED exactly as in step 1 (counted in *n_rejected, flag 0, not emitted, it NEITHER READS NOR WRITES B) when
 * the camera has an address filter and any of these holds: it lies outside the ROI; use_mask is set and its pixel is
 * in the camera's pixel mask; its polarity is suppressed.  A masked hot pixel therefore supports no neighbour and
 * stamps nothing — the difference from filtering first and dropping afterwards.  Steps 2-5 are unchanged.  A kept
 * record is copied whole as before, except that with flatten != 0 its byte 12 (the polarity) is 1 or 0; last_kept
 * shows the flattened record; in the fields form the record is built as esvio_fe_convert_events builds it, then its
 * polarity is replaced.
 * The stage runs wherever esvio_fe_filter_params run: esvio_fe_filter_events, esvio_fe_filter_batch (records and
 * fields), esvio_fe_track_event_filtered, esvio_fe_track_batch, esvio_fe_track_raw with a filter, the feed with a
 * filter.  {0, 0, 0, 0} filter parameters (no support test, no refractory test) give the address stage alone; with
 * filter == NULL nothing runs.
 * The filter and the mask are SETTINGS, like esvio_fe_set_detector's: they survive esvio_fe_reset and
 * esvio_fe_filter_reset.  A fresh handle has neither and allocates nothing for them; the mask is width*height bits per
 * camera, allocated by the first esvio_fe_set_pixel_mask call (or the first installing esvio_fe_hot_select).  use_mask
 * with no mask set rejects nothing.
 * ESVIO_FE_EINVAL with a message, before any device work, nothing changed: a ROI outside the sensor or inverted,
 * polarity or flatten outside 0..2, use_mask outside 0..1, reserved != 0, cam outside 0..1, a mask pair outside the
 * sensor, a null xy with n > 0. */
typedef struct esvio_fe_address_filter {
  uint16_t roi_x0, roi_y0, roi_x1, roi_y1; /* INCLUSIVE, as the drivers' start/end; x0<=x1<width, y0<=y1<height */
  int32_t polarity;  /* 0 both; 1 ON only; 2 OFF only.  ON = polarity byte != 0 */
  int32_t flatten;   /* 0 no; 1: kept records get polarity 1; 2: polarity 0.  Applied after suppression */
  int32_t use_mask;  /* 0 / 1: reject events of pixels in the camera's pixel mask */
  int32_t reserved;  /* 0 */
} esvio_fe_address_filter;                       /* 24 bytes */
int esvio_fe_set_address_filter(esvio_fe_handle h, int cam, const esvio_fe_address_filter* a); /* NULL: none */
int esvio_fe_set_pixel_mask(esvio_fe_handle h, int cam, const uint16_t* xy, size_t n);          /* host, n (x,y) pairs; n == 0 clears */
int esvio_fe_get_pixel_mask(esvio_fe_handle h, int cam, uint16_t* xy, size_t cap, size_t* n);   /* raster order; *n = pixels set, also when > cap (then EINVAL) */

/* HOT-PIXEL LEARNING.  Per camera: a count plane C[width*height] (uint32), N = the number of events counted, t_min
 * and t_max in integer ns (step 2's t) over the counted events.  Allocated by the first call.
 * esvio_fe_hot_learn: every in-sensor event does C[pixel] += 1; out-of-sensor events are ignored; the address stage
 * is NOT applied: learning sees the stream as it arrives.  Sources are esvio_fe_filter_batch's: records in host or
 * device memory, or fields in their three spaces (exactly one of ev / fields when n > 0).  A BAD event (the fields
 * form, by conversion's test) is not counted, every other event of the call is, and the call returns ESVIO_FE_EINVAL
 * with *n_bad (optional) exact.  A call that would take N to 2^32 or beyond is refused before any device work.  The
 * state is stream state: esvio_fe_hot_reset and esvio_fe_reset clear it, esvio_fe_filter_reset does not.
 * esvio_fe_hot_select, all in integers: span = t_max - t_min (0 while N == 0);
 *   T = max(min_count, min_rate_hz ? ceil(min_rate_hz * span / 10^9) : 0, mean_factor ? ceil(mean_factor * N / P) : 0),
 * P = width*height.  The hot pixels are those with C >= T, ordered by COUNT DESCENDING, THEN PIXEL INDEX y*width + x
 * ASCENDING; the first max_pixels are selected.  xy (host, optional, cap (x,y) pairs) and counts (host, optional, cap
 * values) receive them in that order; info (optional): events = N, span_ns, threshold = T, above = pixels with
 * C >= T, selected.  With install the selection becomes the camera's pixel mask, replacing it.  min_rate_hz > 0 with
 * span > 2^42 is ESVIO_FE_EINVAL; selected > cap with a non-null xy or counts is ESVIO_FE_EINVAL, nothing is
 * installed, info is filled.  N == 0 succeeds with nothing selected (with install: the empty mask).  The state is not
 * consumed: learning may go on and select may be called again.  The selection sorts on the device (the stage's own
 * scratch, allocated on first use, main stream only); the sort's bounded wait gives ESVIO_FE_EINTERNAL.
 * Both calls order themselves on the main stream and wait for their own result; they touch nothing of the tracker and
 * nothing of the filter's planes. */
int esvio_fe_hot_learn(esvio_fe_handle h, int cam, const esvio_fe_event* ev, const esvio_fe_event_fields* fields,
                       size_t n, int space, uint64_t* n_bad);
typedef struct esvio_fe_hot_params {
  uint32_t max_pixels;  /* 1..4096 */
  uint32_t min_count;   /* >= 1 */
  uint32_t min_rate_hz; /* 0: unused; <= 2^20 */
  uint32_t mean_factor; /* 0: unused; <= 2^20: a pixel must hold at least mean_factor times the mean count per pixel */
  int32_t install;      /* != 0: the selection becomes the camera's pixel mask (replacing it) */
  int32_t reserved;     /* 0 */
} esvio_fe_hot_params;
typedef struct esvio_fe_hot_info { uint64_t events, span_ns, threshold; uint32_t above, selected; } esvio_fe_hot_info;
int esvio_fe_hot_select(esvio_fe_handle h, int cam, const esvio_fe_hot_params* prm, uint16_t* xy, uint32_t* counts,
                        size_t cap, esvio_fe_hot_info* info);
int esvio_fe_hot_reset(esvio_fe_handle h);

/* ---- one batch call: records or fields, filtered or not, plain or motion-compensated ------ */
/* Every combination of {records, fields} per camera x {no filter, filter} x {plain, motion-compensated} through one
 * call; esvio_fe_track_event_fields and esvio_fe_track_event_filtered are this call with their arguments. */
typedef struct esvio_fe_batch {
  const esvio_fe_event *left, *right;                      /* records, or                                   */
  const esvio_fe_event_fields *left_fields, *right_fields; /* fields: per camera exactly one kind when n>0 */
  size_t nL, nR;
  int32_t space;                        /* where records / fields lie */
  int32_t pub_this_frame;
  const esvio_fe_filter_params* filter; /* NULL: no filter */
  const esvio_fe_motion* motion;        /* NULL: the plain overload; else the motion-compensated one */
  double cur_time;                      /* read when cur_time_from_batch == 0 */
  int32_t cur_time_from_batch;          /* != 0: (double)sec + 1e-9*(double)nsec of the last LEFT record the tracker is given */
  int32_t reserved;                     /* must be 0 */
} esvio_fe_batch;
typedef struct esvio_fe_batch_info {
  uint64_t kept[2], rejected[2], bad[2]; /* kept = records handed to the tracker; rejected: filled when a filter ran */
  double cur_time;                       /* the one used */
  int32_t tracked, reserved;             /* tracked 0: no left record was kept, nothing of the tracker changed */
} esvio_fe_batch_info;
/* No fields and no filter: the call IS esvio_fe_track_event (motion NULL) or esvio_fe_track_event_mc on the same
 * arguments, announced batches included (with cur_time_from_batch the last left record is read first: from host
 * memory directly, from device memory with a wait).
 * Any other combination: ESVIO_FE_EINVAL while batches are announced.  The records the tracker reads live in the
 * handle's two alternating buffer pairs — buffer lifetime exactly as esvio_fe_track_event_fields states it.  The
 * conversion and / or the filter chains of BOTH cameras are enqueued first, and the host waits ONCE before tracking
 * starts: in that wait it reads both cameras' result blocks (and, with cur_time_from_batch and no filter, the last left
 * record) — not once per camera, not once per stage.  A camera given as records beside the other's fields is copied
 * into the pair as it is.  Without a filter nL must be > 0.
 * A BAD event (esvio_fe_convert_events) in either camera: ESVIO_FE_EINVAL, info->bad exact, nothing tracked; with a
 * filter the plane of the camera that held the bad event is unchanged, and whether the other camera's plane has
 * advanced is unspecified (the error message says so).
 * Filter set and kept[0] == 0: ESVIO_FE_OK, tracked = 0, `out` untouched, both planes advanced (node:150 returns early
 * on an empty left message).
 * With motion, t_0 is read on the device from the first left record the tracker is given: after a filter that is the
 * first KEPT one.  info is optional.  Argument errors (a bad space, reserved != 0, a camera with both kinds or none
 * and n > 0, descriptor errors, the filter's limits) are ESVIO_FE_EINVAL before any device work. */
int esvio_fe_track_batch(esvio_fe_handle h, const esvio_fe_batch* b, esvio_fe_tracks* out, esvio_fe_batch_info* info);

/* ---- raw sensor streams: Prophesee EVT3 / EVT2 words -> event records, on the device ------- */
/* Prophesee sensors (the Gen3 VGA of the esio_DSEC and esvio_VECtor parameter sets: EVT2; the Gen4 HD, 1280x720: EVT3)
 * emit a bit-packed, stateful word stream — a .raw recording behind its ASCII header, and what the sensor's USB
 * transfers hold.  An event's row, time base and vector base live in EARLIER words, so no esvio_fe_event_fields can
 * express it.  The reference has no counterpart, and neither a specification nor a vendor decoder was at hand: the rule
 * below is RESTATED FROM RECALL of the published format descriptions, it is UNPINNED — not claimed to be bit-equal to
 * the vendor's decoder — and THIS TEXT IS THE SPECIFICATION; the kernels equal its sequential reading
 * (tests/evt_ref.py) exactly.
 *
 * Per handle and camera there is a decoder state.  It survives from call to call, so a chunk may end anywhere, in the
 * middle of a vector run too.  It is cleared by esvio_fe_decode_reset, and by esvio_fe_reset as part of "as a freshly
 * created handle".
 *
 * EVT3.  State: seen=0, th=0, wraps=0, tl=0, y=0, bx=0, bp=0.  Words are 16-bit little-endian, processed in order;
 * type = w >> 12:
 *   0x0 ADDR_Y       y = w & 0x7FF (bit 11 ignored)
 *   0x2 ADDR_X       one event (x = w & 0x7FF, y, p = (w>>11)&1, t)
 *   0x3 VECT_BASE_X  bx = w & 0x7FF; bp = (w>>11)&1
 *   0x4 VECT_12      for i = 0..11 ascending, if bit i of w is set: one event (x = (bx+i) & 0xFFFF, y, bp, t);
 *                    then bx = (bx+12) & 0xFFFF
 *   0x5 VECT_8       the same with 8 bits and +8
 *   0x6 TIME_LOW     tl = w & 0xFFF
 *   0x8 TIME_HIGH    v = w & 0xFFF; if seen && v < th && th - v >= 2048: wraps += 1 (a smaller back-step is a
 *                    back-step: time goes back, no wrap); then th = v, seen = 1; tl is kept
 *   every other type: ignored, counted in `other` (EXT_TRIGGER, OTHERS, CONTINUED_*: counted, not decoded)
 * t is in microseconds: t = wraps * 2^24 + th * 4096 + tl, taken at the word that emits.  An event emitted while
 * seen == 0 is not emitted: it is counted in `untimed`.
 *
 * EVT2.  State: seen=0, th=0, wraps=0.  Words are 32-bit little-endian; type = w >> 28:
 *   0x0 CD_OFF (p=0), 0x1 CD_ON (p=1): one event x = (w>>11)&0x7FF, y = w&0x7FF,
 *                    t = wraps * 2^34 + th * 64 + ((w>>22)&0x3F)
 *   0x8 TIME_HIGH    v = w & 0x0FFFFFFF, the same wrap rule with half range 2^27
 *   everything else: counted in `other`; `untimed` as for EVT3.
 *
 * EVT2.1 (the vectorised 64-bit format the Gen4.1 / IMX636 HD sensors offer beside EVT3; like the two above RESTATED
 * FROM RECALL and UNPINNED, this text being the specification and tests/evt21_ref.py its sequential reading).  State:
 * EVT2's (seen, th, wraps).  Words are 64-bit little-endian; type = w >> 60:
 *   0x0 EVT_NEG (p=0), 0x1 EVT_POS (p=1): bx = (w>>43)&0x7FF, y = (w>>32)&0x7FF, tlow = (w>>54)&0x3F,
 *                    mask = w & 0xFFFFFFFF; for i = 0..31 ascending, if bit i of mask is set: one event
 *                    (x = bx + i, y, p, t = wraps * 2^34 + th * 64 + tlow).  bx need not be 32-aligned (x reaches
 *                    2047 + 31).  A zero mask emits nothing and is counted nowhere.
 *   0x8 TIME_HIGH    v = (w>>32) & 0x0FFFFFFF, EVT2's wrap rule with half range 2^27
 *   everything else: counted in `other`; `untimed` counts one per set bit while seen == 0.
 * The half-swapped layout some files store these words in (two 32-bit words, high half first) is out of scope.
 *
 * Records.  ticks = t + t_offset_us (signed, |t_offset_us| <= 2^62); sec = ticks / 10^6, nsec = (ticks % 10^6) * 1000;
 * x and y are copied as 16-bit patterns (an out-of-sensor pixel is the SAE update's business, as in the conversion);
 * polarity 0 or 1, the padding bytes 0 — byte for byte what esvio_amd.events.make_events builds.  Events are emitted in
 * word order, and inside a VECT word in ascending i.  An event is BAD when ticks < 0 or sec >= 2^32 (in exact integers,
 * whatever the carried wrap count: a stamp that leaves 64 bits is BAD, it never wraps around): any BAD event fails
 * the call with ESVIO_FE_EINVAL, info->bad is exact and dst is unspecified.  More events than dst_cap also fail the call
 * with ESVIO_FE_EINVAL: info->events holds the exact number needed, dst is unspecified.  In both failures THE CAMERA'S
 * DECODER STATE IS AS IT WAS BEFORE THE CALL, and the next call works normally.  A trailing odd byte (EVT3) or a length
 * that is not a multiple of 4 (EVT2) or of 8 (EVT2.1) is an argument error, raised before any device work.
 *
 * Cutting the decoded stream into time-based batches is the next stage's business (esvio_fe_slice_events below); the
 * EXT_TRIGGER words of all three formats are decoded by esvio_fe_decode_triggers, a .raw file's ASCII header is read by
 * esvio_fe_raw_header (both below); libcaer / AEDAT 3.1 packet streams have a section of their own further down.  Out of scope: EVT4, the half-swapped EVT2.1 layout, the payloads of OTHERS /
 * CONTINUED words. */
#define ESVIO_FE_RAW_EVT2 2
#define ESVIO_FE_RAW_EVT3 3
#define ESVIO_FE_RAW_EVT21 21
typedef struct esvio_fe_raw_info {
  uint64_t events, untimed, other, bad, wraps; /* wraps: the camera's count after the call (before it, if it failed) */
  int64_t first_t_us, last_t_us;               /* ticks of the first / last emitted event; untouched if none */
} esvio_fe_raw_info;
/* the decode stage: camera `cam`'s state advanced by the n_bytes of `words`, the records written to dst.
 * space says where the words lie, with esvio_fe_convert_events' three source paths: ESVIO_FE_DEVICE is read in place
 * (at any alignment; 16-byte aligned words are read 16 bytes per lane); ESVIO_FE_HOST: page-locked memory the library's
 * runtime knows is read in place by the kernels, over PCIe, up to 256 KiB and copied first beyond that (every word is
 * read twice: KERNELS.md "Raw streams"); pageable memory is copied once into the handle's scratch, the 2 or 4 bytes
 * per word and nothing else.  dst: room for dst_cap records (ESVIO_FE_DEVICE: 16-byte aligned device memory, may be
 * handed to every entry point that takes device events, esvio_fe_set_next_batch included; ESVIO_FE_HOST: downloaded);
 * 12 * (n_bytes / 2) records (EVT3), n_bytes / 4 (EVT2) or 4 * n_bytes (EVT2.1) always suffice.  info is optional.  n_bytes == 0 succeeds and
 * touches nothing; n_bytes <= 2^28.
 * Orders itself on the main stream, waits for its own result and touches nothing of the tracker: made between two
 * track calls (announced batches or not) it changes no later tracking result.  Its scratch — 32 bytes per 4096 bytes
 * of words, the copy of a pageable source, the records behind a host dst — grows on first use, and with
 * esvio_fe_reserve for a handle that has decoded before (there for streams of up to 8 bytes per event): a second call
 * of a given size allocates nothing.
 * ESVIO_FE_EINVAL with a message, before any device work: an unknown format, cam outside 0..1, a bad space, null words
 * with n_bytes > 0, a null dst with dst_cap > 0, a misaligned device dst, |t_offset_us| > 2^62, a bad length. */
int esvio_fe_decode_raw(esvio_fe_handle h, int cam, int format, const void* words, size_t n_bytes, int space,
                        int64_t t_offset_us, esvio_fe_event* dst, size_t dst_cap, int dst_space,
                        esvio_fe_raw_info* info);
/* both cameras' decoder states back to the fresh state (the AEDAT and bag walkers' too) */
int esvio_fe_decode_reset(esvio_fe_handle h);
/* esvio_fe_track_batch for a host that has raw words: both cameras' chunks are decoded into the handle's two alternating
 * buffer pairs (buffer lifetime exactly as esvio_fe_track_event_fields states it) and tracked from there with
 * cur_time = (double)sec + 1e-9 * (double)nsec of the last LEFT record the tracker is given; `filter` (optional) and
 * `motion` (optional) as in esvio_fe_batch; with a filter the decoded records are filtered into the pair.  Both
 * cameras' decode chains are enqueued first — three launches for the two of them — and the host waits once before
 * filtering or tracking starts.
 * Capacity is the handle's business: a camera's buffer holds one record per word to begin with (always enough for EVT2
 * and for EVT3 without dense vectors); when the reduce pass reports more, the buffers grow to the reported count and the
 * emit launch alone is repeated — after that a stream of the same density allocates nothing.
 * info->kept = the events decoded (after a filter: kept), info->bad the BAD events; raw[cam] (optional) as
 * esvio_fe_decode_raw's info.  A BAD event in either camera: ESVIO_FE_EINVAL, nothing tracked, BOTH cameras' decoder
 * states as they were — as after every other failure of this call, the filter's or the tracker's included: the states
 * move only when the call returns ESVIO_FE_OK.  No left event (or, with a filter, none kept): ESVIO_FE_OK, tracked = 0, `out` untouched, the
 * decoder states (and the filter's planes) advanced.  Refused while batches are announced (decode into memory of your
 * own for that).  Argument errors as esvio_fe_decode_raw's and the filter's limits, before any device work. */
int esvio_fe_track_raw(esvio_fe_handle h, int format, const void* left, size_t left_bytes,
                       const void* right, size_t right_bytes, int space, int64_t t_offset_us,
                       int pub_this_frame, const esvio_fe_filter_params* filter, const esvio_fe_motion* motion,
                       esvio_fe_tracks* out, esvio_fe_batch_info* info, esvio_fe_raw_info raw[2]);

/* ---- external triggers: the EXT_TRIGGER words of a raw stream -> trigger records, on the device ---- */
/* In a stereo rig with frame cameras (DSEC, VECtor) the frame cameras' exposure signals are wired to the event sensors'
 * trigger inputs, and the sensor writes one EXT_TRIGGER word per edge into its event stream: the frames' stamps on the
 * events' own clock.  esvio_fe_decode_raw counts these words in `other`; this stage decodes them.  Like the formats
 * above the layouts are RESTATED FROM RECALL of the published descriptions and UNPINNED; this text is the specification,
 * tests/evt21_ref.py (decode_triggers) its sequential reading.
 *
 * A trigger word has type 0xA in its format's own type field:
 *   EVT3    id = (w>>8)&0xF,   value = w&1;       t = wraps * 2^24 + th * 4096 + tl, taken at the word
 *   EVT2    id = (w>>8)&0x1F,  value = w&1;       t = wraps * 2^34 + th * 64 + ((w>>22)&0x3F)
 *   EVT2.1  id = (w>>40)&0x1F, value = (w>>32)&1; t = wraps * 2^34 + th * 64 + ((w>>54)&0x3F)
 * TIME_HIGH (and EVT3's TIME_LOW) words act exactly as in the event decoder; every other word is skipped.  ticks, the
 * sec / nsec conversion and the BAD rule are the event records'.  A trigger met while seen == 0 is not written: it is
 * counted in `untimed`.  Triggers are written in word order; the record's padding bytes are 0.
 *
 * State: per handle and camera a decoder state OF ITS OWN (seen, th, wraps, tl), carried from call to call, cleared by
 * esvio_fe_decode_reset and esvio_fe_reset, and left as it was by every failed call.  Running the same chunks through
 * esvio_fe_decode_raw and through this call, in either order, therefore puts events and triggers on one time base.
 *
 * words / n_bytes / space / t_offset_us and their argument errors: as esvio_fe_decode_raw's, the three source paths
 * included.  dst: a HOST array with room for dst_cap records.  More triggers than dst_cap: ESVIO_FE_EINVAL,
 * info->triggers holds the number needed, the state is as it was; a BAD trigger: ESVIO_FE_EINVAL, info->bad exact, the
 * state as it was.  info is optional; first_t_us / last_t_us are untouched when no trigger was written.  Three launches
 * in the decode chain's shape (KERNELS.md "EVT2.1, triggers, windows at given stamps"); waits for its own result and
 * touches nothing of the tracker. */
typedef struct esvio_fe_trigger {
  uint32_t sec, nsec;
  uint8_t id, value;
  uint8_t _pad[6];
} esvio_fe_trigger;
typedef struct esvio_fe_trigger_info {
  uint64_t triggers, untimed, bad, wraps; /* wraps: the camera's trigger-decoder count after the call (before it, if it failed) */
  int64_t first_t_us, last_t_us;
} esvio_fe_trigger_info;
int esvio_fe_decode_triggers(esvio_fe_handle h, int cam, int format, const void* words, size_t n_bytes, int space,
                             int64_t t_offset_us, esvio_fe_trigger* dst, size_t dst_cap, esvio_fe_trigger_info* info);

/* ---- the .raw file's ASCII header (host only, no handle) ----------------------------------- */
/* A Prophesee .raw recording begins with text lines and goes on with the words.  The rule, RESTATED FROM RECALL and
 * UNPINNED like the formats: the header is the maximal run of lines from byte 0 each of which begins with '%' and ends
 * with '\n'; it ends in front of the first line that does not begin with '%', or behind a line "% end" (so payload
 * bytes that happen to begin with '%' behind it are payload).  Inside it, with any blanks between '%' and the key and a
 * trailing '\r' ignored:
 *   "% evt 2.0" / "% evt 2.1" / "% evt 3.0"        the format: ESVIO_FE_RAW_EVT2 / _EVT21 / _EVT3
 *   "% format EVT2|EVT21|EVT3[;key=value...]"       the format and, with width= / height= among the keys, the geometry;
 *                                                   it wins over "% evt" wherever the two lines stand
 *   "% geometry WxH"                                the geometry
 * out: payload_offset = the index of the first payload byte, format and width / height (0: not stated), complete.
 * complete == 0: the header's end does not lie inside the n bytes — they end inside a header line, or directly behind
 * one that is not "% end" (the next line may be another; n == 0 is this case).  Nothing behind the last whole line was
 * read, payload_offset is where the next line starts or started, format and geometry are those of the whole lines; read
 * more and call again (a caller at the end of its file has a header-only file).  ESVIO_FE_EINVAL: null bytes with
 * n > 0, null out. */
typedef struct esvio_fe_raw_header_info {
  uint64_t payload_offset;
  int32_t format;        /* 0: unknown */
  int32_t width, height; /* 0: unknown */
  int32_t complete;
} esvio_fe_raw_header_info;
int esvio_fe_raw_header(const void* bytes, size_t n, esvio_fe_raw_header_info* out);

/* ---- libcaer / AEDAT 3.1 packet streams: polarity events, IMU6 samples, special events ---- */
/* The DAVIS and DVXplorer sensors of the esvio, esio, esvio_ecmd and esvio_mvsec_flying parameter sets speak libcaer:
 * the three drivers the reference vendors (dependences/rpg_dvs_ros: davis_ros_driver, dvxplorer_ros_driver,
 * dvs_ros_driver) receive event PACKETS, and an AEDAT 3.1 recording is those packets written one behind the other, behind
 * a text header.  The PER-EVENT ARITHMETIC below is the reference driver's, cited by line: the polarity loop is
 * davis_ros_driver/src/driver.cpp:664-694 (the same lines at dvxplorer_ros_driver/src/driver.cpp:319-323), the IMU6 loop
 * is davis_ros_driver/src/driver.cpp:722-775.  libcaer's bit accessors are not in the reference's tree: THE PACKET AND
 * EVENT LAYOUTS ARE RESTATED FROM RECALL of libcaer / AEDAT 3.1 and UNPINNED — not claimed to be bit-equal to libcaer —
 * and THIS TEXT IS THE SPECIFICATION; tests/aedat_ref.py is its sequential reading, and the library equals it exactly.
 *
 * Packet stream.  All fields are little-endian.  A packet is a 28-byte header
 *   int16 eventType, int16 eventSource, int32 eventSize, int32 eventTSOffset, int32 eventTSOverflow,
 *   int32 eventCapacity, int32 eventNumber, int32 eventValid
 * and behind it eventCapacity * eventSize payload bytes (a 64-bit product).  The first eventNumber records of the payload
 * are events, the rest is padding and is skipped.  eventValid is not trusted: validity is bit 0 of each event's first
 * word.  Types:
 *   0 SPECIAL   eventSize 8,  eventTSOffset 4   decoded by esvio_fe_aedat_side
 *   1 POLARITY  eventSize 8,  eventTSOffset 4   decoded by esvio_fe_decode_aedat
 *   3 IMU6      eventSize 36, eventTSOffset 4   decoded by esvio_fe_aedat_side
 *   every other type (frames among them): skipped whole, counted in other_packets
 * A header is MALFORMED when eventSize <= 0, eventCapacity < 0, eventNumber < 0, eventNumber > eventCapacity, or a type
 * 0 / 1 / 3 packet's eventSize or eventTSOffset differs from the table.  A malformed header fails the call with
 * ESVIO_FE_EINVAL before any device work, and the state is as it was.  A packet is counted (polarity_packets,
 * other_packets) by the call in which its header's last byte arrives.
 *
 * Polarity event: uint32 data; int32 ts.  valid = data & 1, p = (data>>1) & 1, y = (data>>2) & 0x7FFF,
 * x = (data>>17) & 0x7FFF.  ts64 = ((int64)eventTSOverflow << 31) | (uint32)ts, in microseconds
 * (caerPolarityEventGetTimestamp64).  Record: ticks_ns = ts64 * 1000 + t_offset_ns, where t_offset_ns is the driver's
 * reset_time_ in NANOSECONDS, |t_offset_ns| <= 2^62 — nanoseconds, unlike the EVT calls' microseconds, because
 * reset_time_ is ros::Time::now() and the record must equal reset_time_ + Duration().fromNSec(ts64 * 1000)
 * (driver.cpp:685-686).  sec = ticks_ns / 10^9, nsec = ticks_ns % 10^9; x and y are copied as 16-bit patterns; polarity
 * is 0 or 1, the padding bytes 0 — byte for byte what esvio_amd.events.make_events builds.  Events go out in stream order.
 * BAD: an emitted event is BAD when ts < 0, eventTSOverflow < 0, ticks_ns < 0 or sec >= 2^32, decided in exact integers.
 * (ts64 >= 2^53 is always BAD under the offset limit, so an implementation may test that first and then stay inside 64
 * bits.)  A BAD event fails the call: info->bad is exact, dst is unspecified, the state is as it was.
 * Validity: by default an event with valid == 0 is dropped and counted in `invalid` — the format's rule; a dropped event
 * is not examined further and is never BAD.  With ESVIO_FE_AEDAT_KEEP_INVALID in `flags` every one of the eventNumber
 * events is emitted and `invalid` stays 0 — exactly what the reference's drivers do, which never look at the bit.
 *
 * Special event: uint32 data; int32 ts.  valid = data & 1 (dropped / kept as above), type = (data>>1) & 0x7F.  Type 1,
 * TIMESTAMP_RESET, is counted in `resets`.  Types 2 / 3 / 4 — external input rising / falling / pulse — become
 * esvio_fe_trigger records with the events' stamp rule (BAD included), id = type, value = (type != 3).  Every other type
 * is counted in `other_specials`.  Only a special that becomes a record has its stamp examined.
 *
 * IMU6 event: uint32 info; int32 ts; float ax, ay, az, gx, gy, gz, temp (36 bytes).  valid = info & 1.  The output is an
 * esvio_fe_imu_sample: the stamp as for events (BAD included), acc = (-ax, ay, -az) * 9.81 and
 * gyr = (-gx, gy, -gz) / 180.0 * M_PI, evaluated as driver.cpp:735-741 writes them: the float is negated first, then
 * widened to double, then the operations run left to right in double.  No bias is applied: bias is the driver's
 * calibration state (driver.cpp:766-771).
 *
 * State.  Per handle and camera there are TWO walker states, one for esvio_fe_decode_aedat (and the track / feed entry
 * points), one for esvio_fe_aedat_side.  Each holds the header bytes collected so far (0..27), the open packet's type,
 * event size and overflow, its events and payload bytes still to come, and the bytes of a record cut by the chunk's end
 * (up to 35).  A chunk may end anywhere: inside a header, inside a record, inside padding; a cut record is emitted by the
 * call that brings its last byte.  esvio_fe_decode_reset and esvio_fe_reset clear both states; every failed call leaves
 * them as they were.  The same chunks through both calls, in either order, give events, IMU samples and triggers on one
 * time base — the esvio_fe_decode_triggers arrangement.
 *
 * Source.  `bytes` is memory the HOST can read, pageable or pinned.  There is no `space` argument and no device source:
 * the packet chain is a linked list that only a sequential walk can follow, so the host walks it (one cache line per
 * packet), gathers the polarity records — and nothing else: a DAVIS346 frame packet of 180 KB never crosses PCIe — into
 * pinned scratch with a table of the runs of equal eventTSOverflow, and the device decodes that array one record per
 * lane (KERNELS.md "AEDAT 3.1").  A stream that lies in device memory would have to come back first.
 *
 * Frame packets (type 2) are decoded by a third call with a walker of its own: "AEDAT 3.1 frames" below.  To the two
 * calls of this section they stay other_packets.
 *
 * Out of scope: AEDAT 2.0 and AEDAT 4, IMU samples or triggers inside the feed (the side call beside it is the way). */
#define ESVIO_FE_AEDAT_KEEP_INVALID 1u
typedef struct esvio_fe_aedat_info {
  uint64_t events, invalid, bad;             /* emitted (a too small dst_cap: the number needed); dropped; BAD */
  uint64_t polarity_packets, other_packets;  /* headers completed by this call: type 1; neither 0, 1 nor 3 */
  int64_t first_t_us, last_t_us;             /* ticks_ns / 1000 of the first / last emitted event; untouched if none */
} esvio_fe_aedat_info;
typedef struct esvio_fe_imu_sample {
  uint32_t sec, nsec;
  double acc[3]; /* m/s^2 */
  double gyr[3]; /* rad/s */
} esvio_fe_imu_sample;
typedef struct esvio_fe_aedat_side_info {
  uint64_t imu, triggers;            /* samples / trigger records written (a too small capacity: the numbers needed) */
  uint64_t resets, other_specials;   /* TIMESTAMP_RESET specials; specials of every other type */
  uint64_t invalid, bad;             /* dropped specials and samples; BAD triggers and samples */
  uint64_t special_packets, imu_packets, other_packets; /* headers completed by this call: type 0; 3; neither 0, 1 nor 3 */
} esvio_fe_aedat_side_info;
/* The file header (host only, no handle): the maximal run of lines from byte 0 each of which begins with '#' and ends
 * with '\n'.  It ends behind the line "#!END-HEADER" (a trailing '\r' ignored), or in front of the first line that does
 * not begin with '#'.  A FIRST line "#!AER-DAT<a>.<b>" (a: decimal digits, b: one digit, a trailing '\r' ignored) gives
 * version = 10 a + b — "#!AER-DAT3.1": 31 —, anything else 0.  out->payload_offset, complete as in
 * esvio_fe_raw_header_info: complete == 0 when the n bytes end inside a line or behind one that is not the end line
 * (n == 0 is that case); nothing behind the last whole line is read.  Only version 31 is decoded below; the caller
 * checks.  ESVIO_FE_EINVAL: null bytes with n > 0, null out. */
typedef struct esvio_fe_aedat_header_info {
  uint64_t payload_offset;
  int32_t version;  /* 0: not stated */
  int32_t complete;
} esvio_fe_aedat_header_info;
int esvio_fe_aedat_header(const void* bytes, size_t n, esvio_fe_aedat_header_info* out);
/* the decode stage: camera `cam`'s event walker advanced by the n_bytes at `bytes`, the records written to dst (room for
 * dst_cap records; dst_space as esvio_fe_decode_raw's: ESVIO_FE_DEVICE, 16-byte aligned, or ESVIO_FE_HOST).  More
 * emitted events than dst_cap: ESVIO_FE_EINVAL, info->events holds the exact count needed, the state is as it was; the
 * sum of the chunk's eventNumber (plus one for a record the last chunk cut) always suffices.  n_bytes == 0 succeeds and
 * touches nothing; n_bytes <= 2^28.  info is optional.  Orders itself on the main stream, waits for its own result and
 * touches nothing of the tracker: made between two track calls it changes no later tracking result.  Its scratch — 8
 * pinned and 8 device bytes per polarity record, the run table, 4 bytes per tile, the records behind a host dst — grows
 * on first use and with esvio_fe_reserve for a handle that has decoded AEDAT before: a second call of a given size
 * allocates nothing.  ESVIO_FE_EINVAL with a message, before any device work: cam outside 0..1, flags with unknown bits,
 * null bytes with n_bytes > 0, a null dst with dst_cap > 0, a bad dst_space, a misaligned device dst,
 * |t_offset_ns| > 2^62, n_bytes > 2^28, a malformed header. */
int esvio_fe_decode_aedat(esvio_fe_handle h, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                          esvio_fe_event* dst, size_t dst_cap, int dst_space, esvio_fe_aedat_info* info);
/* the side call: camera `cam`'s side walker advanced by the same kind of chunk; IMU6 samples to imu (HOST, room for
 * imu_cap), external-input specials to trig (HOST, room for trig_cap), both in stream order.  More of either than its
 * capacity: ESVIO_FE_EINVAL, info->imu / info->triggers hold the numbers needed, the state is as it was.  A BAD sample or
 * trigger: ESVIO_FE_EINVAL, info->bad exact, the state as it was.  Runs on the host alone; argument errors as above. */
int esvio_fe_aedat_side(esvio_fe_handle h, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                        esvio_fe_imu_sample* imu, size_t imu_cap, esvio_fe_trigger* trig, size_t trig_cap,
                        esvio_fe_aedat_side_info* info);
/* esvio_fe_track_raw with the decode chain exchanged: both cameras' chunks are walked, both chains enqueued, the host
 * waits once, and the records are tracked from the handle's two alternating buffer pairs with cur_time = the stamp of the
 * last LEFT record the tracker is given; `filter` and `motion` as there.  Capacity is the host-known sum of eventNumber,
 * so no launch is ever repeated.  aedat[cam] (optional) as esvio_fe_decode_aedat's info.  A BAD event or a malformed
 * header in either camera: ESVIO_FE_EINVAL, nothing tracked, BOTH cameras' walker states as they were — the states move
 * only when the call returns ESVIO_FE_OK.  Refused while batches are announced. */
int esvio_fe_track_aedat(esvio_fe_handle h, const void* left, size_t left_bytes, const void* right, size_t right_bytes,
                         int64_t t_offset_ns, uint32_t flags, int pub_this_frame, const esvio_fe_filter_params* filter,
                         const esvio_fe_motion* motion, esvio_fe_tracks* out, esvio_fe_batch_info* info,
                         esvio_fe_aedat_info aedat[2]);

/* ---- AEDAT 3.1 frames: the DAVIS frame packets of the same stream -> trackImage's 8-bit gray, on the device ---- */
/* Five of the shipped parameter sets are DAVIS rigs, and in ESVIO mode the second feature stream is that sensor's own APS
 * frames: type-2 packets between the polarity, special and IMU6 packets of the stream above.  WHAT IS CITED: the
 * per-frame arithmetic is the driver's FRAME_EVENT branch, davis_ros_driver/src/driver.cpp:778-823 — the channel number
 * gives the encoding, 1 -> "mono8", 3 -> "rgb8", and nothing else gets one (:788-804); the pixel array is read linearly
 * and each 16-bit value becomes value >> 8 (:807-814); the stamp is reset_time_ + Duration().fromNSec(ts64 * 1000)
 * (:817-818); the exposure length is published beside it (:823).  An "rgb8" frame then goes through getImageFromMsg's
 * cv::COLOR_RGB2GRAY (feature_tracker/src/stereo_image_tracker_node.cpp:296-301), which is exactly the 15-bit rule that
 * "rosbag images" below states for class 3, on the byte triple (R, G, B) of value >> 8.  WHAT IS RESTATED FROM RECALL AND
 * UNPINNED, as for the other AEDAT types: libcaer's accessors are not in the reference's tree, so THE FRAME PACKET AND
 * FRAME EVENT LAYOUTS BELOW ARE RECALLED, not claimed to be bit-equal to libcaer, and THIS TEXT IS THE SPECIFICATION;
 * tests/aedat_frame_ref.py is its sequential reading, and the library equals it exactly.
 *
 * Packet.  Type 2, FRAME, with eventTSOffset 12.  The header's common checks are those of the section above.  A type-2
 * header is also MALFORMED when eventSize < 36, eventSize - 36 is odd, or eventTSOffset != 12.  Packets of types 0 / 1 / 3
 * get the table's checks of the section above and are skipped whole; every other type is skipped whole and counted in
 * other_packets.  A packet is counted (frame_packets, other_packets) by the call in which its header's last byte arrives.
 *
 * Frame event: eventSize bytes, little-endian.  A 36-byte head
 *   uint32 info; int32 ts_startframe, ts_endframe, ts_startexposure, ts_endexposure, lengthX, lengthY, positionX, positionY
 * and behind it uint16 pixels, row-major with the channels interleaved, up to eventSize - 36 bytes.  info: bit 0 valid,
 * bits 1-3 the channel number, bits 4-7 the colour filter, bits 8-14 the ROI id.  An emitted event is MALFORMED when
 * lengthX < 1, lengthY < 1, or lengthX * lengthY * channels * 2 > eventSize - 36, decided in exact integers (lengthX *
 * lengthY is below 2^62; an implementation may compare it with (eventSize - 36) / (2 * channels) rounded down, and a
 * channel number of 0 passes this check).  Then, REFUSED BY NAME like the bag images, the message naming the value: a
 * channel number other than 1 or 3 (the driver gives that frame no encoding), and a lengthX x lengthY that is not the
 * handle's width x height (no cv::resize, as stated there).  positionX / positionY, the colour filter and the ROI id are
 * recorded and otherwise ignored, as the driver ignores them.  Malformed and refused fail the call with ESVIO_FE_EINVAL
 * before any device work, the state as it was; they are decided, in this order, in the call that brings the head's last
 * byte.
 *
 * Pixels.  The frame's lengthX * lengthY * channels values are the first that many uint16 behind the head; bytes behind
 * them in the event are never read.  One channel: gray = value >> 8.  Three: (R, G, B) = the pixel's three values >> 8,
 * gray = (R * 9798 + G * 19235 + B * 3735 + (1 << 14)) >> 15.
 *
 * Stamp.  The frame's ts is the mid-exposure stamp, ts_startexposure + (ts_endexposure - ts_startexposure) / 2, computed
 * in 64-bit integers with the division truncating toward zero (caerFrameEventGetTimestamp, recalled).  ts64 and the
 * stamp then follow the polarity events' rule with the packet's eventTSOverflow, BAD included: ticks_ns = ts64 * 1000 +
 * t_offset_ns, BAD when ts < 0, eventTSOverflow < 0, ticks_ns < 0 or sec >= 2^32.  The stamp is taken, and BAD decided
 * (behind malformed and refused), with the t_offset_ns of the call that brings the head's last byte.  A BAD frame fails
 * the call: info->bad is exact, nothing is stored, the state is as it was.  exposure_us = ts_endexposure -
 * ts_startexposure in 64 bits.
 *
 * Validity, as for events: by default an event with valid == 0 is dropped and counted in `invalid`; it is not examined
 * further and is never BAD, malformed or refused.  With ESVIO_FE_AEDAT_KEEP_INVALID every one of the eventNumber events
 * is emitted.  The driver looks only at event 0 of a packet (caerFrameEventPacketGetEvent(frame, 0), :781) and never at
 * the valid bit; this call emits EVERY event in stream order and records each one's position within its packet in
 * `slot`.  THE ROWS WITH slot == 0 UNDER ESVIO_FE_AEDAT_KEEP_INVALID ARE EXACTLY THE DRIVER'S FRAMES.
 *
 * State.  Per handle and camera there is a THIRD walker state for esvio_fe_decode_aedat_frames, so the same chunks may go
 * through the event call, the side call and the frame call in any order.  A chunk may end anywhere, inside the 36-byte
 * head or inside the pixels; a frame is emitted by the call that brings its last PIXEL byte.  The pixel bytes of a cut
 * frame wait in a carry buffer the handle owns; a failed call leaves state and carry as they were.  esvio_fe_decode_reset
 * and esvio_fe_reset clear the frame walkers too.  In ESVIO mode the frame call is made on the image tracker's handle,
 * whose width and height are the sensor's.
 *
 * Source.  Host memory, as above.  The counting walk checks everything; the gathering walk copies each emitted frame's
 * lengthX * lengthY * channels * 2 pixel bytes, and nothing else, into pinned scratch, each frame from a 16-byte boundary;
 * one copy brings them and the descriptor table to the device and ONE launch of k_frame16_emit (KERNELS.md "AEDAT
 * frames") writes all frames of the call.
 *
 * Out of scope: the driver's auto-exposure (computeNewExposure), frames inside the feed, the node harnesses, and sizes
 * other than the handle's. */
typedef struct esvio_fe_aedat_frame { /* one emitted frame event */
  uint32_t stamp_sec, stamp_nsec;           /* the mid-exposure stamp: what the node pairs left and right by */
  int32_t ts_startframe, ts_endframe, ts_startexposure, ts_endexposure; /* the head's four raw stamps */
  int64_t exposure_us;                      /* ts_endexposure - ts_startexposure */
  int32_t length_x, length_y, position_x, position_y;
  int32_t channels, color_filter, roi;      /* info bits 1-3, 4-7, 8-14 */
  int32_t valid, slot;                      /* info bit 0; the event's position within its packet */
  int32_t ts_overflow;                      /* its packet's eventTSOverflow */
  uint64_t index;                           /* its image in dst, counted per call */
} esvio_fe_aedat_frame;
typedef struct esvio_fe_aedat_frame_info {
  uint64_t frames, invalid, bad;            /* emitted (too small a capacity: the number needed); dropped; BAD */
  uint64_t frame_packets, other_packets;    /* headers completed by this call: type 2; none of 0, 1, 2, 3 */
  uint32_t first_sec, first_nsec, last_sec, last_nsec; /* the first / last emitted frame's stamp; 0 if none */
} esvio_fe_aedat_frame_info;
/* the frame call: camera `cam`'s frame walker advanced by the n_bytes at `bytes`; the k-th emitted frame of the call
 * becomes the dense width * height gray image at dst + k * width * height (room for dst_cap IMAGES; dst_space:
 * ESVIO_FE_DEVICE, any alignment, or ESVIO_FE_HOST), and an esvio_fe_aedat_frame per emitted frame, in stream order, goes
 * to the HOST array frames (room for frames_cap).  More frames than dst_cap or frames_cap: ESVIO_FE_EINVAL, info->frames
 * holds the exact number needed, nothing is stored, the state is as it was.  n_bytes == 0 succeeds and touches nothing;
 * n_bytes <= 2^28.  info is optional.  Orders itself on the main stream, waits for its own result and touches nothing of
 * the tracker.  Its scratch — the pixel bytes pinned and on the device, the images behind a host dst — grows on first use
 * and with esvio_fe_reserve (one rgb frame of the handle's size) for a handle that has decoded frames before: a second
 * call of a given size allocates nothing.  ESVIO_FE_EINVAL with a message, before any device work: cam outside 0..1,
 * unknown bits in flags, null bytes with n_bytes > 0, a null dst with dst_cap > 0, null frames with frames_cap > 0, a bad
 * dst_space, |t_offset_ns| > 2^62, n_bytes > 2^28, a malformed header or event, a refused channel number or size, a BAD
 * stamp.
 * Tracking frame pairs: merge the two cameras' tables (esvio_amd.node.StereoImageTrackerNode.merge_frame_tables), pair
 * them as the node does (pair_images) and hand dst + index * width * height to
 * esvio_fe_track_image_space(..., ESVIO_FE_DEVICE, ...). */
int esvio_fe_decode_aedat_frames(esvio_fe_handle h, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns,
                                 uint32_t flags, uint8_t* dst, size_t dst_cap, int dst_space, esvio_fe_aedat_frame* frames,
                                 size_t frames_cap, esvio_fe_aedat_frame_info* info);
/* the conversion alone, for a host that holds caerFrameEventGetPixelArrayUnsafe's array of a live device: height x width
 * pixels (each 1 .. 8192, whatever the handle's size) of `channels` (1 or 3) uint16 values each, dense and row-major at
 * src (src_space ESVIO_FE_HOST: copied to the device first; ESVIO_FE_DEVICE: read in place, at any 2-byte alignment), to
 * the dense gray image dst (dst_space likewise; any alignment) by the pixel rule above.  Argument errors are
 * ESVIO_FE_EINVAL before any device work. */
int esvio_fe_convert_frame16(esvio_fe_handle h, const uint16_t* src, int src_space, uint32_t height, uint32_t width,
                             int32_t channels, uint8_t* dst, int dst_space);

/* ---- rosbag v2.0 recordings: dvs_msgs/EventArray events of both cameras, sensor_msgs/Imu samples ---- */
/* The reference is run on ROS bags and nothing else: its README ("3. Run on Dataset") says `rosbag play`, and the HKU
 * dataset and the DSEC / MVSEC / VECtor conversions its config/ sets are written for are bags that hold
 * dvs_msgs/EventArray messages on two topics and sensor_msgs/Imu on a third.  WHAT IS CITED: the event's wire order is
 * feature_tracker/src/dvs_msgs/Event.h:190-193 (x, y, ts, polarity), the message's is EventArray.h:222-225 (header,
 * height, width, events), the type name and MD5 are EventArray.h:145,158 ("dvs_msgs/EventArray",
 * "5e8beee5a6c107e504c2e78903c224b8"), the polarity rule is event_detector.cc:133 (ep ? 1 : 0).  WHAT IS RECALLED: the bag
 * container, std_msgs/Header and sensor_msgs/Imu serialization are ROS's and are not in the reference's tree: THE
 * CONTAINER AND THESE TWO LAYOUTS ARE RESTATED FROM RECALL of the rosbag 2.0 format and UNPINNED — not claimed to be
 * bit-equal to rosbag — and THIS TEXT IS THE SPECIFICATION; tests/bag_ref.py is its sequential reading, and the library
 * equals it exactly.
 *
 * Container.  All integers are little-endian.  The file starts with the 13 bytes "#ROSBAG V2.0\n"; the walkers below
 * start BEHIND them (esvio_fe_bag_header's payload_offset).  Behind them come RECORDS: uint32 header_len, the header,
 * uint32 data_len, the data.  A header is a sequence of FIELDS, each uint32 field_len followed by field_len bytes
 * "name=value": the name ends at the first '=', the value is binary.  Every header has a 1-byte field `op`:
 *   0x03 bag header    index_pos u64, conn_count u32, chunk_count u32         data: padding, skipped
 *   0x05 chunk         compression (a string), size u32                       data: with "none" a sequence of op 0x02 /
 *                                                                             0x07 records that ends exactly at data_len;
 *                                                                             size == data_len
 *   0x07 connection    conn u32, topic                                        data: a connection header in the same field
 *                                                                             encoding: type, md5sum (message_definition,
 *                                                                             callerid, latching, topic are passed over)
 *   0x02 message data  conn u32, time (u32 sec, u32 nsec)                     data: the serialized message
 *   0x04 index data, 0x06 chunk info                                          skipped by length, fields not examined
 *   every other op                                                            skipped by length, counted in other_records
 * Fields a record does not need are ignored; of a repeated field the last one counts.  Inside a chunk only op 0x02 and
 * 0x07 may appear.  Connection records also appear outside chunks (at index_pos); a message record outside a chunk is
 * read like one inside.  `chunks`, `other_records` and `other_messages` count a record in the call that brings the last
 * byte of its data_len; `connections` counts every connection record in the call that brings its last data byte.
 *
 * Roles.  esvio_fe_bag_set_topics names up to three topics: left events, right events, IMU (NULL: none; the strings are
 * copied; each at most 255 bytes, not empty, no two equal, else ESVIO_FE_EINVAL).  The call clears both walker states.
 * Without it no topic has a role.  A connection's role is decided by the `topic` field of its record HEADER.  A
 * connection with a role enters the handle's connection table (conn id -> role) when its record's last data byte
 * arrives; its data must then hold `type` == "dvs_msgs/EventArray" and `md5sum` == the MD5 above for an event topic, and
 * `type` == "sensor_msgs/Imu" for the IMU topic (no MD5 is checked there: none can be cited), else the stream is
 * MALFORMED and the message names the topic.  A connection record whose conn id is in the table must give the same role
 * (the same topic), else malformed; one without a role whose id is not in the table is passed over.  A message whose
 * conn is not in the table is skipped and counted in other_messages.
 *
 * EventArray message data:  u32 seq, u32 stamp.sec, u32 stamp.nsec, u32 L, L bytes frame_id, u32 height, u32 width, u32 n,
 * then n * 13 bytes: uint16 x, uint16 y, uint32 sec, uint32 nsec, uint8 polarity.  data_len == 28 + L + 13 n must hold
 * exactly.  Record: x and y copied as 16-bit patterns, sec and nsec copied, polarity = (wire byte != 0), the padding
 * bytes 0 — byte for byte what esvio_amd.events.make_events builds.  Every wire event is emitted, in each camera's stream
 * order.  An event is BAD when nsec >= 10^9; a BAD event fails the call: the info's bad is exact, dst is unspecified.
 *
 * Imu message data: the same header (seq, stamp, L, frame_id), then 37 float64: orientation 4, its covariance 9,
 * angular_velocity 3, covariance 9, linear_acceleration 3, covariance 9.  data_len == 16 + L + 296 exactly.  Output: an
 * esvio_fe_imu_sample with the header stamp, gyr = angular_velocity, acc = linear_acceleration, the doubles copied bit
 * for bit.  A sample is BAD when stamp.nsec >= 10^9.
 *
 * MALFORMED, besides the length rules above: header_len > 4096; a field that overruns its header (or, in connection
 * data, its data); a field without '='; a header without `op` or with an `op` not 1 byte long; a missing required field
 * or one of the wrong length; a `topic` longer than 255 bytes; `type` or `md5sum` of a connection with a role missing or
 * different; more than 64 connections with a role; an op other than 0x02 / 0x07 inside a chunk, or a record there that
 * overruns the chunk; a chunk whose `compression` is not "none" — that message tells the user to run `rosbag decompress`:
 * silently skipping data is worse than refusing.  A malformed stream fails the call with ESVIO_FE_EINVAL before any
 * device work, whatever else the chunk holds, in the call that brings the last byte of the offending item (a length
 * word, a header, a connection field's first 264 bytes or its end, a connection's data, a message's fixed part).
 *
 * State.  Each handle has TWO walker states, one for esvio_fe_decode_bag and esvio_fe_feed_push_bag, one for
 * esvio_fe_bag_side; a state is per handle, not per camera: a bag interleaves both.  Each holds the record phase and the
 * partial header (at most 4 KB), the connection table, the open chunk's and the open message's bytes still to come, the
 * <= 12 bytes of an event cut by the call's end, and per camera the number of events emitted since the last reset.  A
 * call's bytes may end anywhere.  Events are emitted as their last byte arrives; a message is listed, and an IMU sample
 * written, by the call that brings its last byte.  Every failed call leaves the states as they were — malformed input, a
 * BAD event or sample, too small a destination or table (the exact counts needed come back in the info).
 * esvio_fe_decode_reset and esvio_fe_reset clear both states (the topics stay).  The same bytes through both calls, in
 * either order, give events and samples on one time base: the stamps are the recording's own.
 *
 * Source.  `bytes` is memory the HOST can read.  The records of a bag are a chain that only a sequential walk can follow,
 * so the host walks it (esvio_amd/csrc/fe_bag.h): a counting walk over a copy of the state checks everything and sizes
 * the outputs, a gathering walk copies the event arrays — and nothing else: images, IMU, index and connection data never
 * cross PCIe — densely per camera into pinned scratch, one copy brings them to the device, and one kernel turns both
 * cameras' 13-byte wire events into records, one per lane (KERNELS.md "ROS bags").
 *
 * Out of scope: bz2 / lz4 chunks, bag format 1.2, seeking by the index (the walk is sequential), compressed image topics
 * (sensor_msgs/CompressedImage) and every sensor_msgs/Image encoding or size that "rosbag images" below refuses,
 * prophesee_event_msgs and other event message types, the odometry topic, IMU and images inside the feed (the side call
 * and the image call beside it are the way), announced batches, writing bags. */
typedef struct esvio_fe_bag_topics {
  const char* left;   /* dvs_msgs/EventArray, camera 0 */
  const char* right;  /* dvs_msgs/EventArray, camera 1 */
  const char* imu;    /* sensor_msgs/Imu */
} esvio_fe_bag_topics;
int esvio_fe_bag_set_topics(esvio_fe_handle h, const esvio_fe_bag_topics* topics);
/* The magic and the bag header record (host only, no handle).  payload_offset = 13 once the magic is there (the walkers
 * start at it and pass over the op 0x03 record themselves), version = 20; index_pos, conn_count, chunk_count from the
 * record; complete == 1 once the n bytes hold the record's header and data_len, else the other fields past what was
 * read are 0.  ESVIO_FE_EINVAL: null bytes with n > 0, null out, bytes that are no prefix of the magic, a first record
 * that is malformed or not op 0x03. */
typedef struct esvio_fe_bag_header_info {
  uint64_t payload_offset, index_pos;
  uint32_t conn_count, chunk_count;
  int32_t version;  /* 20 once the magic is complete, else 0 */
  int32_t complete;
} esvio_fe_bag_header_info;
int esvio_fe_bag_header(const void* bytes, size_t n, esvio_fe_bag_header_info* out);
typedef struct esvio_fe_bag_message { /* one completed EventArray message */
  int32_t cam;                   /* 0 left, 1 right */
  uint32_t seq;                  /* header.seq */
  uint32_t stamp_sec, stamp_nsec; /* header.stamp: what the node pairs left and right by */
  uint32_t time_sec, time_nsec;  /* the record's `time` */
  uint32_t height, width;
  uint64_t first;                /* index of its first event in the camera's emitted stream since the last reset */
  uint64_t count;                /* n */
} esvio_fe_bag_message;
typedef struct esvio_fe_bag_cam_info {
  uint64_t events, bad, messages; /* emitted (too small a dst_cap: the number needed); BAD; messages completed */
  uint32_t first_sec, first_nsec, last_sec, last_nsec; /* the first / last emitted event's stamp; untouched if none */
} esvio_fe_bag_cam_info;
typedef struct esvio_fe_bag_info {
  esvio_fe_bag_cam_info cam[2];
  uint64_t other_messages, other_records, chunks, connections;
} esvio_fe_bag_info;
typedef struct esvio_fe_bag_side_info {
  uint64_t imu, bad; /* samples written (too small an imu_cap: the number needed); BAD samples */
  uint64_t other_messages, other_records, chunks, connections;
} esvio_fe_bag_side_info;
/* the decode stage: the event walker advanced by the n_bytes at `bytes`; camera cam's records go to dst[cam] (room for
 * dst_cap[cam]; dst_space for both: ESVIO_FE_DEVICE, 16-byte aligned, or ESVIO_FE_HOST), an esvio_fe_bag_message per
 * completed event message, in stream order, to the HOST array msgs (room for msgs_cap).  More events than a dst_cap or
 * more messages than msgs_cap: ESVIO_FE_EINVAL, info->cam[].events / .messages hold the exact numbers needed, nothing is
 * stored in a dst that is too small, the state is as it was.  flags must be 0.  n_bytes == 0 succeeds and touches
 * nothing; n_bytes <= 2^28.  info is optional.  Orders itself on the main stream, waits for its own result and touches
 * nothing of the tracker, as esvio_fe_decode_aedat.  Its scratch — 13 pinned and 13 device bytes per event, the records
 * behind a host dst — grows on first use and with esvio_fe_reserve for a handle that has decoded a bag before: a second
 * call of a given size allocates nothing.  ESVIO_FE_EINVAL with a message, before any device work: unknown bits in
 * flags, null bytes with n_bytes > 0, a null dst[cam] with dst_cap[cam] > 0, null msgs with msgs_cap > 0, a bad
 * dst_space, a misaligned device dst, n_bytes > 2^28, a malformed stream.
 * Tracking message pairs: pair left and right messages by header stamp and hand the slices dst[cam] + first .. + count
 * to esvio_fe_track_event(..., ESVIO_FE_DEVICE, ...) with cur_time = the last left event's stamp, as the node does. */
int esvio_fe_decode_bag(esvio_fe_handle h, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_event* const dst[2],
                        const size_t dst_cap[2], int dst_space, esvio_fe_bag_message* msgs, size_t msgs_cap,
                        esvio_fe_bag_info* info);
/* the side call: the side walker advanced by the same kind of chunk; the IMU samples, in stream order, to imu (HOST, room
 * for imu_cap).  More than imu_cap, or a BAD sample: ESVIO_FE_EINVAL, info->imu / info->bad exact, the state as it was.
 * Runs on the host alone; argument errors as above. */
int esvio_fe_bag_side(esvio_fe_handle h, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_imu_sample* imu,
                      size_t imu_cap, esvio_fe_bag_side_info* info);

/* ---- rosbag images: sensor_msgs/Image messages of two topics -> trackImage's 8-bit gray, on the device ---- */
/* The ESVIO-mode parameter sets name image_left_topic / image_right_topic beside the event and IMU topics, and their bags
 * hold all five.  WHAT IS CITED: which encodings the node takes and what it does with each is getImageFromMsg,
 * feature_tracker/src/stereo_image_tracker_node.cpp:257-318 — "8UC1" is relabelled mono8 and copied (:261-275), "8UC3" is
 * relabelled bgr8 and goes through cv::COLOR_BGR2GRAY (:276-290), "mono8" is copied (:291-295), "rgb8" goes through
 * cv::COLOR_RGB2GRAY (:296-301), "bgr8" through cv::COLOR_BGR2GRAY (:302-307); the size check is :314-316; left and right
 * are paired by header.stamp within +-1 s and msg_timestamp is the left stamp (:219-246).  WHAT IS RECALLED AND UNPINNED,
 * as the container above: the sensor_msgs/Image wire layout, what cv_bridge::toCvCopy does for an unchanged encoding, and
 * cv::cvtColor's 8-bit gray.  THIS TEXT IS THE SPECIFICATION; tests/bag_image_ref.py is its sequential reading.
 *
 * Image message data: the std_msgs/Header as above (u32 seq, u32 stamp.sec, u32 stamp.nsec, u32 L, L bytes frame_id),
 * u32 height, u32 width, u32 Le, Le bytes encoding, u8 is_bigendian, u32 step, u32 D, D bytes data.  Well-formed:
 * data_len == 37 + L + Le + D exactly, D == step * height exactly, height >= 1 and width >= 1, Le <= 32,
 * step >= width * bpp (bpp 1 for the mono class, 3 for the colour classes); else the stream is MALFORMED and the message
 * names the topic.  The connection's `type` must be "sensor_msgs/Image"; no MD5 is checked, as for the IMU: none can be
 * cited.  is_bigendian is recorded and otherwise ignored: every accepted encoding has 8 bits per channel.
 *
 * Pixels.  toCvCopy with an unchanged encoding: row r is the width * bpp bytes at data + r * step, the rows packed
 * densely; bytes behind them in a row are never read.  Classes: 1 = "mono8" | "8UC1": the byte; 2 = "bgr8" | "8UC3":
 * (B, G, R) = the pixel's three bytes; 3 = "rgb8": (R, G, B).  Gray, as recalled for OpenCV 4.2's RGB2Gray<uchar>:
 *     gray = (R * 9798 + G * 19235 + B * 3735 + (1 << 14)) >> 15
 * THIS RULE IS THE 15-BIT FORM.  OpenCV 3's constants (4899 / 9617 / 1868, + (1 << 13), >> 14) give another byte on some
 * pixels — (R, G, B) = (0, 0, 250) is 28 here and 29 there; tests/test_image_msg_vs_cv2.py compares with the cv2 at hand.
 *
 * REFUSED BY NAME, with ESVIO_FE_EINVAL, before any device work, the state as it was, in the call that brings the last
 * byte of the message's fixed part: every other encoding (the reference's else branch hands those to cv_bridge's
 * converters, which are not in its tree; the message names the encoding and the topic), and a message whose width x
 * height is not the handle's (the reference calls cv::resize there, :314-316; no shipped parameter set triggers it, its
 * 8-bit INTER_LINEAR can only be recalled, and a silently different resize is worse than a refusal).
 *
 * Roles and state.  esvio_fe_bag_set_image_topics names the left and the right image topic (NULL: none; the string rules of
 * esvio_fe_bag_set_topics; no image topic may equal a topic that has a role from esvio_fe_bag_set_topics, else
 * ESVIO_FE_EINVAL).  It clears the image walker's state only.  The handle has a THIRD walker state for
 * esvio_fe_decode_bag_images, so the same bytes may go through the event call, the side call and the image call in any
 * order; the image walk sees only the image topics (event and IMU messages are other_messages to it) and the other two
 * walks see only theirs.  In ESVIO mode the image call is made on the image tracker's handle — width and height are the
 * frame camera's — where no event topic need be set.  The bytes of a payload that a call's end cuts wait in a carry
 * buffer the handle owns; a failed call leaves state and carry as they were.  esvio_fe_decode_reset and esvio_fe_reset
 * clear the image state too; the topics stay.
 *
 * Source.  The counting walk checks everything; the gathering walk copies each completed message's D payload bytes, and
 * nothing else, into pinned scratch, each from a 16-byte boundary; one copy brings them and the descriptor table to the
 * device and ONE launch of k_image_emit (KERNELS.md "ROS bag images") writes all images of both cameras. */
typedef struct esvio_fe_bag_image { /* one completed Image message */
  int32_t cam;                     /* 0 left, 1 right */
  uint32_t seq;                    /* header.seq */
  uint32_t stamp_sec, stamp_nsec;  /* header.stamp: what the node pairs left and right by */
  uint32_t time_sec, time_nsec;    /* the record's `time` */
  uint32_t height, width, step;
  int32_t encoding;                /* 1 mono8 | 8UC1, 2 bgr8 | 8UC3, 3 rgb8 */
  int32_t is_bigendian;
  uint64_t index;                  /* its image in dst[cam], counted per call */
} esvio_fe_bag_image;
typedef struct esvio_fe_bag_image_cam_info {
  uint64_t images; /* messages completed (too small a dst_cap: the number needed) */
  uint32_t first_sec, first_nsec, last_sec, last_nsec; /* the first / last completed message's header stamp; 0 if none */
} esvio_fe_bag_image_cam_info;
typedef struct esvio_fe_bag_image_info {
  esvio_fe_bag_image_cam_info cam[2];
  uint64_t other_messages, other_records, chunks, connections;
} esvio_fe_bag_image_info;
int esvio_fe_bag_set_image_topics(esvio_fe_handle h, const char* left, const char* right);
/* the image call: the image walker advanced by the n_bytes at `bytes`; camera cam's k-th completed message of the call
 * becomes the dense width * height gray image at dst[cam] + k * width * height (room for dst_cap[cam] IMAGES; dst_space
 * for both: ESVIO_FE_DEVICE, any alignment, or ESVIO_FE_HOST), an esvio_fe_bag_image per completed message, in stream
 * order, to the HOST array msgs (room for msgs_cap).  More images than a dst_cap or more messages than msgs_cap:
 * ESVIO_FE_EINVAL, info->cam[].images hold the exact numbers needed, nothing is stored, the state is as it was.  flags
 * must be 0.  n_bytes == 0 succeeds and touches nothing; n_bytes <= 2^28.  info is optional.  Orders itself on the main
 * stream, waits for its own result and touches nothing of the tracker.  Its scratch — the payload bytes pinned and on the
 * device, the images behind a host dst — grows on first use and with esvio_fe_reserve (one stereo pair of rgb8 frames of
 * the handle's size) for a handle that has decoded images before: a second call of a given size allocates nothing.
 * ESVIO_FE_EINVAL with a message, before any device work: unknown bits in flags, null bytes with n_bytes > 0, a null
 * dst[cam] with dst_cap[cam] > 0, null msgs with msgs_cap > 0, a bad dst_space, n_bytes > 2^28, a malformed stream, a
 * refused encoding or size.
 * Tracking frame pairs: pair left and right entries as the node does (esvio_amd.node.StereoImageTrackerNode.pair_images)
 * and hand dst[cam] + index * width * height to esvio_fe_track_image_space(..., ESVIO_FE_DEVICE, ...). */
int esvio_fe_decode_bag_images(esvio_fe_handle h, const void* bytes, size_t n_bytes, uint32_t flags, uint8_t* const dst[2],
                               const size_t dst_cap[2], int dst_space, esvio_fe_bag_image* msgs, size_t msgs_cap,
                               esvio_fe_bag_image_info* info);
/* the conversion alone: one image of height x width pixels (each 1 .. 8192, whatever the handle's size) of class
 * `encoding` (1, 2, 3 as above), its rows `step` bytes apart at src (src_space ESVIO_FE_HOST: copied to the device first;
 * ESVIO_FE_DEVICE: read in place, at any alignment), to the dense gray image dst (dst_space likewise; any alignment).
 * step >= width * bpp, and the source's bytes up to the last row's last pixel, (height - 1) * step + width * bpp, are at
 * most 2^28.  Argument errors are ESVIO_FE_EINVAL before any device work. */
int esvio_fe_convert_image(esvio_fe_handle h, const void* src, int src_space, uint32_t height, uint32_t width, uint32_t step,
                           int32_t encoding, uint8_t* dst, int dst_space);
/* esvio_fe_track_image whose dense width * height images lie in `space`: ESVIO_FE_HOST is esvio_fe_track_image itself;
 * ESVIO_FE_DEVICE: device memory, any alignment, re-pitched into level 0 (with equalize: into the raw slot in front of
 * CLAHE) on the device — the pixels never come to the host.  The results are bit-identical for the same bytes. */
int esvio_fe_track_image_space(esvio_fe_handle h, double cur_time, const uint8_t* img_left, const uint8_t* img_right,
                               int space, int pub_this_frame, esvio_fe_tracks* out);

/* ---- text event files: "t x y p" / "x y p t" lines -> event records, on the device ---------- */
/* The third container the reference's own tooling writes events in, beside rosbag and the libcaer stream.  Its tree
 * ships three writers, and their lines are the formats below:
 *   dvs_file_writer/scripts/extract_davis_bag_files.py  events.txt: "<secs>.<nsecs, 9 digits> <x> <y> <0|1>\n"
 *                                                       (timestamp_str, and the loop over msg.events) — the Event
 *                                                       Camera Dataset's events.txt; beside it imu.txt
 *                                                       "t ax ay az gx gy gz" and images.txt "t path"
 *   dvs_file_writer/scripts/extract_dvs_bag_files.py    "<x> <y> <p> <t_us>\n" (to_nsec() / 1000, integer division)
 *   dvs_file_writer/src/writer.cpp                      "<x> <y> <p> <t_us>" and std::endl
 * The second form, with commas, is also what a Prophesee CSV export holds ("x,y,p,t", microseconds).  A stamp is two
 * integers printed in decimal, so the decode is exact integer arithmetic; THIS TEXT IS THE SPECIFICATION, tests/text_ref.py
 * is its sequential reading, and Python's int() and decimal.Decimal are the oracle of its numbers.
 *
 * Format.  esvio_fe_text_format: order = ESVIO_FE_TEXT_TXYP or _XYPT; time = ESVIO_FE_TEXT_SEC_DECIMAL, _INT_US or
 * _INT_NS; flags = ESVIO_FE_TEXT_END (this chunk ends the stream) | ESVIO_FE_TEXT_SKIP_MALFORMED (malformed lines are
 * dropped and counted instead of failing the call); reserved = 0.  The davis extractor is {TXYP, SEC_DECIMAL}; the dvs
 * extractor, writer.cpp and a Prophesee CSV are {XYPT, INT_US}.
 *
 * Lines.  A line ends at '\n'; a '\r' directly before the '\n' belongs to the terminator; the body is what lies before
 * the terminator.  The body is classified in this order:
 *   1. more than 64 bytes: MALFORMED;
 *   2. leading and trailing separator bytes — space, tab, comma — are stripped; nothing left: BLANK;
 *   3. first byte '#' or '%': COMMENT;
 *   4. split on runs of one or more separator bytes; anything other than exactly four tokens: MALFORMED;
 *   5. the tokens, in the format's order; any byte not listed here, in any token, is MALFORMED ('+', 'e', 'E', NUL ...):
 *        x, y   1 to 5 decimal digits, value <= 65535
 *        p      exactly "0", "1" or "-1"; "-1" gives polarity 0
 *        t, SEC_DECIMAL       1 to 10 digits I, optionally followed by '.' and at least one digit F:
 *                             ns = I * 10^9 + (the first nine digits of F, padded on the right with zeros); digits
 *                             behind the ninth must be digits and are dropped — truncation, not rounding (the cited
 *                             writer never emits them)
 *        t, INT_US / INT_NS   1 to 19 digits, read in exact integers: ns = v * 1000 (INT_US), ns = v (INT_NS)
 * Stamps.  ticks = ns + t_offset_ns (signed, |t_offset_ns| <= 2^62); sec = ticks / 10^9, nsec = ticks % 10^9.  An event
 * line is BAD when ticks < 0 or sec >= 2^32, decided in exact integers: a 19-digit value never wraps, it is BAD.
 * Records.  x, y, sec, nsec, polarity 0 or 1, the padding bytes 0 — byte for byte what esvio_amd.events.make_events
 * builds —, in line order.  x and y are not compared with the sensor size: that stays the SAE update's business, as in
 * the other decoders.
 *
 * State.  Per handle and camera: the unterminated tail of the stream so far — at most 65 bytes: 64 of body and one
 * '\r' — or the flag "inside a line whose body has already passed 64 bytes", with the number of that line's bytes so
 * far; the rest of such a line is discarded up to its terminator.  A line is classified and counted in the call that
 * holds its terminator.  With ESVIO_FE_TEXT_END a non-empty tail is a line (a '\r' at its end, no '\n' behind it, is a
 * byte of its body), a line still being discarded is a malformed line, and the state is fresh afterwards.  The state is
 * cleared by esvio_fe_decode_reset and esvio_fe_reset.
 *
 * Failures.  ESVIO_FE_EINVAL for a malformed line without SKIP_MALFORMED, for any BAD line, for more events than dst_cap
 * (a BAD line counts among `events`).  In all three every count of info is exact and `events` holds the number needed,
 * dst is unspecified — records beyond the first min(events, dst_cap) are never touched, and nothing at all is stored
 * when events > dst_cap —, THE CAMERA'S STATE IS AS IT WAS BEFORE THE CALL and the next call works normally.
 * first_t_ns and last_t_ns are filled by a call that succeeds; carried is the tail's length behind such a call, and
 * on a refused call — an argument error included — the tail's length as before the call.
 * Sizes.  n_bytes <= 2^28; n_bytes == 0 without END touches nothing; (n_bytes + 65) / 8 + 1 records always suffice (the
 * shortest event line is 8 bytes).
 * Out of scope: exponent notation (numpy's default savetxt format), a missing integer part (".5"), more than four
 * columns, quoted fields, header lines that are neither blank nor comments (without SKIP_MALFORMED they fail the call,
 * with it they are counted), compressed text. */
#define ESVIO_FE_TEXT_TXYP 1
#define ESVIO_FE_TEXT_XYPT 2
#define ESVIO_FE_TEXT_SEC_DECIMAL 1
#define ESVIO_FE_TEXT_INT_US 2
#define ESVIO_FE_TEXT_INT_NS 3
#define ESVIO_FE_TEXT_END 1u
#define ESVIO_FE_TEXT_SKIP_MALFORMED 2u
typedef struct esvio_fe_text_format {
  int32_t order, time;
  uint32_t flags, reserved;
} esvio_fe_text_format;
typedef struct esvio_fe_text_info {
  uint64_t events, lines, comments, blank, malformed, bad; /* lines = events + comments + blank + malformed */
  int64_t first_malformed;       /* byte offset of the first malformed line's first byte, relative to this call's `bytes`:
                                    negative when the line began in the carried state; untouched if there is none; filled
                                    with SKIP_MALFORMED too */
  int64_t first_t_ns, last_t_ns; /* ticks of the first / last event; untouched if none */
  uint32_t carried;              /* the length of the tail after the call */
  uint32_t reserved;
} esvio_fe_text_info;
/* the decode stage: camera `cam`'s state advanced by the n_bytes of `bytes`, the records written to dst.  The source's
 * three paths are esvio_fe_decode_raw's: ESVIO_FE_DEVICE is read in place, at any alignment; ESVIO_FE_HOST: page-locked
 * memory the library's runtime knows is read in place up to 256 KiB and copied first beyond that (every byte is read
 * twice), pageable memory is copied once into the handle's scratch.  dst, dst_space, info as esvio_fe_decode_raw's.
 * Orders itself on the main stream, waits for its own result and touches nothing of the tracker.  Its scratch — 32 bytes
 * per 4096 bytes of text, the copy of a pageable source, the records behind a host dst (min(dst_cap, the bound above) of
 * them) — grows on first use, and with esvio_fe_reserve for a handle that has decoded text before (there for lines of
 * 16 bytes and more).  ESVIO_FE_EINVAL with a message, before any device work: a null or unknown format, reserved != 0,
 * unknown flags, cam outside 0..1, a bad space, null bytes with n_bytes > 0, a null dst with dst_cap > 0, a misaligned
 * device dst, |t_offset_ns| > 2^62, n_bytes > 2^28. */
int esvio_fe_decode_text(esvio_fe_handle h, int cam, const esvio_fe_text_format* fmt, const void* bytes, size_t n_bytes,
                         int space, int64_t t_offset_ns, esvio_fe_event* dst, size_t dst_cap, int dst_space,
                         esvio_fe_text_info* info);
/* esvio_fe_track_raw's contract for text: both cameras' chains are enqueued first — three launches for the two of them
 * —, the host waits once, cur_time comes from the last LEFT record, the cameras' states move only when the call returns
 * ESVIO_FE_OK; a malformed line (without SKIP_MALFORMED) or a BAD line in either camera: ESVIO_FE_EINVAL, nothing
 * tracked, both states as they were.  text[cam] (optional) as esvio_fe_decode_text's info.  Refused while batches are
 * announced. */
int esvio_fe_track_text(esvio_fe_handle h, const esvio_fe_text_format* fmt, const void* left, size_t left_bytes,
                        const void* right, size_t right_bytes, int space, int64_t t_offset_ns, int pub_this_frame,
                        const esvio_fe_filter_params* filter, const esvio_fe_motion* motion, esvio_fe_tracks* out,
                        esvio_fe_batch_info* info, esvio_fe_text_info text[2]);
/* the side files of the davis extractor, whole files in host memory, no handle, no device work.  Lines, blank lines and
 * comments as above (a last line may lack its terminator; a line holds up to 4096 bytes); the stamp is the SEC_DECIMAL
 * token with t_offset_ns applied, BAD as above.
 * imu.txt, "t ax ay az gx gy gz": acc = (ax, ay, az), gyr = (gx, gy, gz), each the double nearest to its decimal text,
 * read independently of the locale (a fixed or exponent form, "inf", "nan"; no leading '+').
 * images.txt, "t path": stamps_ns[i] = ticks; the path is bytes[path_off[i], path_off[i] + path_len[i]): what follows the
 * stamp and its spaces or tabs, up to the line's end without trailing separator bytes.
 * ESVIO_FE_EINVAL: a line that does not read or is BAD (*n_out: the entries in front of it), more entries than cap
 * (*n_out: the number needed; the first cap are written), null pointers. */
int esvio_fe_text_imu(const void* bytes, size_t n, int64_t t_offset_ns, esvio_fe_imu_sample* out, size_t cap, size_t* n_out);
int esvio_fe_text_images(const void* bytes, size_t n, int64_t t_offset_ns, int64_t* stamps_ns, uint64_t* path_off,
                         uint32_t* path_len, size_t cap, size_t* n_out);

/* ---- stream slicing: a record stream cut into fixed-rate windows, on the device ------------ */
/* trackEvent takes one batch per camera and call; a recording or a sensor transfer is a long stream whose batch edges
 * are points in time.  The reference cuts its streams off line, dependences/events_repacking_helper/src/
 * EventMessageEditor.cpp: every event topic is re-chunked at 30 Hz, the message's header.stamp is the window's END (:25),
 * the node pairs left and right by it (stereo_event_tracker_node.cpp:382-403) and its publish decision reads it
 * (:155-188).  This stage does that cut on the device, per camera, with state that survives from call to call, so a chunk
 * may end anywhere.  The rule below is the specification; its sequential reading is tests/slice_ref.py
 * (slice_windows), the reference's own loop as it is written is repack() beside it.
 *
 * Times.  The stamp of an event is ts = (double)sec + 1e-9 * (double)nsec — ros::Time::toSec(): two roundings, no FMA.
 * Time(d) of a double is roscpp's ros::Time::fromSec: sec = floor(d), nsec = round((d - sec) * 1e9) (halves away from
 * zero), and nsec == 10^9 carries into sec.  toSec(Time) is the expression above.  Time() is RESTATED FROM RECALL of
 * roscpp: the CONTROL FLOW of the reference's loop is pinned by recordings of its compiled code
 * (tests/golden/repack_ref_*.npz), this rounding is not — the recordings were made against a stand-in ros::Time that
 * restates it the same way.  period = 1.0 / frequency in double; 1e-3 <= frequency <= 1e6.
 *
 * Boundaries.  Per camera E_0 = Time(ts_origin + period), E_{k+1} = Time(toSec(E_k) + period).  ts_origin is the stamp
 * of the first event the camera's slicer ever sees (the reference's bFirstMessage_ rule) or, with has_origin, the stamp
 * of esvio_fe_slice_params.origin — the project's own option, so that two cameras share their windows.  The chain
 * depends on no event after the first: the host computes it.  E_k whose sec leaves 32 bits is no boundary: an event at
 * or beyond it fails the call (ESVIO_FE_EINVAL).
 *
 * Windows.  The carried state is the origin, m — the number of windows closed so far — and whether a first event was
 * seen.  For the events of a call in stream order, with m_start the count before the call and m_{-1} = m_start:
 *   c_i = m_start + #{k >= m_start : toSec(E_k) <= ts_i};   m_i = max(m_{i-1}, c_i);   event i belongs to window m_i.
 * So an event at or after the boundary closes the window (the reference's >=); an event that steps back in time stays
 * in the open window (where the reference's push_back puts it); equal and non-monotonic stamps need no special case;
 * an event before an explicit origin belongs to window 0; a jump over whole windows closes each of them, the skipped
 * ones empty.  The window open at the end of a call is NOT closed — the reference never writes its tail either, and a
 * stream's end is the caller's business: esvio_fe_slice_flush closes it.  m_i is a prefix maximum, which is associative:
 * slice(whole) = slice(part 1) then slice(part 2) at every cut.
 *
 * Against the reference.  EventMessageEditor::insertEvent advances by at most ONE window per event:
 * b_i = b_{i-1} + [c_i > b_{i-1}].  Both rules give the same windows and the same header stamps E_k on every stream in
 * which no event jumps a whole window (c_i <= m_{i-1} + 1 for all i).  After a longer gap the reference's windows lag
 * behind their own header stamps — a message stamped E_k then holds events from behind E_k — until enough events have
 * come; there the rule above is THE PROJECT'S OWN, chosen so that the end stamp of a window stays true (the node's
 * publish decision and its left / right pairing read nothing else).
 *
 * Per call at most ESVIO_FE_SLICE_MAX_WINDOWS windows are closed: the call's range is the boundaries E_{m_start} ..
 * E_{m_start + 4096}, and an event at or beyond the last of them fails the call with ESVIO_FE_EINVAL.  After that
 * failure, and after every other one, THE CAMERA'S STATE IS AS IT WAS BEFORE THE CALL (the same events in smaller calls
 * work): the state lives on the host, the device works on counts relative to it, and the host takes the result over
 * only once the call is known to succeed. */
#define ESVIO_FE_SLICE_MAX_WINDOWS 4096
typedef struct esvio_fe_slice_params {
  double frequency;       /* windows per second, 1e-3 .. 1e6 */
  esvio_fe_event origin;  /* has_origin != 0: ts_origin is this record's stamp (x, y, polarity are not read) */
  int32_t has_origin;     /* 0: ts_origin is the stamp of the camera's first event */
  int32_t reserved;       /* must be 0 */
} esvio_fe_slice_params;
typedef struct esvio_fe_slice_info {
  uint64_t closed;        /* windows this call closed (a failed call: 0, or with too small a cuts_cap the number needed) */
  uint64_t first_window;  /* index of the first of them = the camera's count before the call */
  uint64_t count;         /* the camera's count after the call (a failed call: before it) */
  uint64_t open_events;   /* events in the window left open, earlier calls' included */
  uint32_t first_sec, first_nsec; /* E of the first closed window (untouched when closed == 0) */
  uint32_t last_sec, last_nsec;   /* E of the last closed window  (untouched when closed == 0) */
} esvio_fe_slice_info;
/* the slicer stage: camera `cam`'s state advanced by the n records of `ev` (space: ESVIO_FE_HOST — copied to the device
 * as they are, one copy — or ESVIO_FE_DEVICE, 16-byte aligned, read in place; n <= 2^30).  cuts (host, room for cuts_cap
 * entries): cuts[j] is the index in `ev` of the first event that does not belong to the j-th window this call closed —
 * window first_window + j is [cuts[j-1], cuts[j]) of this call's events, behind whatever earlier calls left open of it;
 * entries are non-decreasing, skipped windows repeat an index; entries behind `closed` are not touched.  More closed
 * windows than cuts_cap: ESVIO_FE_EINVAL, info->closed holds the number needed, the state is as it was.
 * A camera's frequency and origin are fixed by its first call with n > 0; a later call with other parameters is
 * ESVIO_FE_EINVAL (esvio_fe_slice_reset first).  n == 0 succeeds, touches nothing and reports the state.
 * Orders itself on the main stream, waits for its own result (for a device source the very first call without has_origin
 * also reads ev[0] first) and touches nothing of the tracker: made between two track calls (announced batches or not)
 * it changes no later tracking result.  ESVIO_FE_EINVAL while a feed is open on the handle (below).  Three launches, none of which waits on the device for another workgroup
 * (KERNELS.md "Stream slicing").  Its scratch — 4 bytes per 1024 events, the copy of a host source, the boundary table
 * (128 KiB per camera, refilled every ~12000 windows) — grows on first use: a second call of a size allocates nothing.
 * ESVIO_FE_EINVAL with a message, before any device work: cam outside 0..1, a bad space, a null prm, reserved != 0, a
 * frequency outside the limits, null ev with n > 0, a misaligned device ev, null cuts with cuts_cap > 0. */
int esvio_fe_slice_events(esvio_fe_handle h, int cam, const esvio_fe_event* ev, size_t n, int space,
                          const esvio_fe_slice_params* prm, uint64_t* cuts, size_t cuts_cap, esvio_fe_slice_info* info);
/* closes camera `cam`'s open window, empty or not (the end of a stream): closed = 1, first_window = its index,
 * first / last = its E, open_events = 0.  A camera that has seen no event has no boundaries yet: closed = 0. */
int esvio_fe_slice_flush(esvio_fe_handle h, int cam, esvio_fe_slice_info* info);
/* both cameras' slicer states back to the fresh state (esvio_fe_reset does the same as part of "as a freshly created
 * handle") */
int esvio_fe_slice_reset(esvio_fe_handle h);
/* Windows that end at GIVEN stamps — the frames' — instead of at first event + k / frequency.  In ESVIO mode the
 * reference's estimator pops the front image-feature message and the front event-feature message as a pair, with no
 * stamp check between them, integrates the IMU up to the image's stamp and treats the event features as observed then
 * (esvio_estimator/src/stereo_estimator_node.cpp:143-167): a caller that has the frame stamps — from
 * esvio_fe_decode_triggers, or from a dataset's timestamp file — wants its event windows to end there.
 *
 * bounds: a HOST array of n_bounds <= ESVIO_FE_SLICE_MAX_WINDOWS records of which only sec / nsec are read:
 * b_k = (double)sec + 1e-9 * (double)nsec.  They must be non-decreasing (else ESVIO_FE_EINVAL before any device work)
 * and are the ends of windows m_start, m_start + 1, ..., m_start being the camera's closed count at the call.  With
 * m_{-1} = m_start:
 *   c_i = m_start + #{k : b_k <= ts_i};   m_i = max(m_{i-1}, c_i);   event i belongs to window m_i.
 * So an event at a boundary closes the window, equal boundaries give empty windows, an event that steps back stays in
 * the open window, and events at or beyond the last given boundary belong to the open window m_start + n_bounds — that
 * is no failure: the caller passes bounds + closed, and newer boundaries behind them, next time.  Associative like its
 * sibling: slice_at(whole, B) = slice_at(part 1, B) then slice_at(part 2, B + closed_1) at every cut.  The sequential
 * reading is tests/slice_at_ref.py.
 * ev / n / space, cuts / cuts_cap and info exactly as esvio_fe_slice_events'; first_ / last_sec / nsec are the closing
 * boundaries' own words, copied.  n_bounds == 0 is allowed (bounds may then be null): nothing closes.
 * Mode: a camera's first call with n > 0 of either entry point fixes fixed-rate or explicit mode; the other entry point
 * is ESVIO_FE_EINVAL until esvio_fe_slice_reset.  ESVIO_FE_EINVAL while a feed is open, like its sibling (the feed
 * itself cuts at fixed rate only).  esvio_fe_slice_flush in explicit mode closes the open window — closed = 1,
 * first_window = its index, open_events = 0 — and leaves the four stamp fields untouched: the window has no boundary.
 * The three launches are esvio_fe_slice_events' own, over a table of the caller's stamps. */
int esvio_fe_slice_events_at(esvio_fe_handle h, int cam, const esvio_fe_event* ev, size_t n, int space,
                             const esvio_fe_event* bounds, size_t n_bounds, uint64_t* cuts, size_t cuts_cap,
                             esvio_fe_slice_info* info);

/* ---- the feed: chunks of a stereo stream in, time-aligned windows tracked where they lie ---- */
/* A small layer over the stages above for a caller that holds a recording or a sensor transfer, not batches: chunks of
 * records, fields or raw words go in per camera, at any chunk size (a raw chunk may end inside a vector run), optionally
 * through the noise filter; esvio_fe_track_event calls on fixed-rate windows come out.  The records never leave the
 * device.  The reference's counterpart is the off-line re-chunking above plus the node's pairing of left and right
 * messages by header.stamp (stereo_event_tracker_node.cpp:382-403); with a shared origin the window INDEX pairs the
 * cameras here, the node's 0.2 s tolerance has nothing to do.
 *
 * esvio_fe_feed_open: prm as esvio_fe_slice_params — both cameras share the origin: the explicit one, else the stamp of
 * the first LEFT record the feed appends (a right push before that is ESVIO_FE_EINVAL).  filter: NULL, or the
 * parameters every pushed chunk is filtered with (copied).  Opening resets both cameras' slicer states; one feed per
 * handle (a second open is ESVIO_FE_EINVAL; esvio_fe_feed_close first).  esvio_fe_reset empties an open feed — no
 * records, no windows, the origin as esvio_fe_feed_open left it — and keeps it open.  An open feed owns both cameras'
 * slicer states — its window queue counts in them: esvio_fe_slice_events, esvio_fe_slice_flush and esvio_fe_slice_reset
 * are ESVIO_FE_EINVAL while it is open.
 *
 * A push appends what it produces to camera cam's accumulation buffer, on the device: the existing convert, filter and
 * decode chains write at the append position (records without a filter are copied there); then the slicer runs over the
 * appended records and the windows it closes are queued.  info (optional): the records appended, the filter's rejected
 * count, the BAD events, the windows this push closed, the camera's closed and untracked windows.
 * A push waits for the result blocks of the chains it ran — the decode's, the conversion's or the filter's, the
 * slicer's — and for nothing else.
 * Failures: argument errors are raised before any device work.  A BAD event (esvio_fe_convert_events,
 * esvio_fe_decode_raw), a slicer failure or a HIP error appends nothing, queues nothing and leaves the camera's decoder
 * and slicer states as they were; so is the filter's plane after a BAD event.  Only a slicer failure BEHIND a filter
 * (a chunk that jumps ESVIO_FE_SLICE_MAX_WINDOWS windows) finds the camera's plane advanced by the chunk:
 * esvio_fe_filter_reset is then the caller's business.
 *
 * esvio_fe_feed_peek: whether a window is closed in BOTH cameras and not yet tracked, and for the oldest such window its
 * index, its end stamp E_k — the reference's header.stamp, the msg_timestamp the node's publish decision reads
 * (node:155-188): the caller decides pub_this_frame before it tracks — and both cameras' counts.
 * esvio_fe_feed_track tracks that window from the accumulation buffers where they lie (ESVIO_FE_DEVICE; with `motion`
 * the motion-compensated overload), with cur_time = (double)sec + 1e-9 * (double)nsec of the window's last LEFT record
 * (node:190), read from the device first.  An empty left window is consumed with tracked = 0 and `out` untouched
 * (node:150); no window ready is ESVIO_FE_EINVAL.  info as esvio_fe_track_batch's: kept = the counts, cur_time, tracked.
 * Buffer lifetime: each camera has TWO buffers.  The records a track call reads stay untouched until everything that
 * call enqueued on any of the handle's streams has finished: appends write behind every record a track call was ever
 * given; when a chunk does not fit behind them, the untracked tail moves to the front of the camera's OTHER buffer
 * (grown first if it is too small) on the main stream, behind the events recorded on the side streams when the last
 * track call that read that buffer returned — the mechanism of esvio_fe_track_event_fields' alternating pairs.  Closing
 * a feed and opening one again rewinds the append position to the front of the current buffers: the first append
 * behind it waits, on the device, for those same events.  A buffer
 * grows to 5/4 of what it has to hold: a second stream of the same density allocates nothing; esvio_fe_reserve, for a
 * handle with an open feed, makes the buffers large enough for 2 * max_events records per camera.
 * Every feed entry point is refused while batches are announced. */
typedef struct esvio_fe_feed_info {
  uint64_t appended, rejected, bad; /* records appended; rejected: filled when a filter ran; BAD events */
  uint64_t closed, queued;          /* windows this push closed; the camera's closed and untracked windows after it */
} esvio_fe_feed_info;
typedef struct esvio_fe_feed_window {
  int32_t ready, reserved;     /* ready 0: nothing else is filled */
  uint64_t index;              /* k */
  uint32_t end_sec, end_nsec;  /* E_k */
  uint64_t count[2];           /* left, right */
} esvio_fe_feed_window;
int esvio_fe_feed_open(esvio_fe_handle h, const esvio_fe_slice_params* prm, const esvio_fe_filter_params* filter);
int esvio_fe_feed_push_events(esvio_fe_handle h, int cam, const esvio_fe_event* ev, size_t n, int space,
                              esvio_fe_feed_info* info);
int esvio_fe_feed_push_fields(esvio_fe_handle h, int cam, const esvio_fe_event_fields* fields, size_t n, int space,
                              esvio_fe_feed_info* info);
int esvio_fe_feed_push_raw(esvio_fe_handle h, int cam, int format, const void* words, size_t n_bytes, int space,
                           int64_t t_offset_us, esvio_fe_feed_info* info);
/* esvio_fe_feed_push_raw for an AEDAT 3.1 chunk (host memory; it may end anywhere): the polarity events are appended,
 * everything else is skipped; failures as esvio_fe_decode_aedat's, with nothing appended and the walker as it was */
int esvio_fe_feed_push_aedat(esvio_fe_handle h, int cam, const void* bytes, size_t n_bytes, int64_t t_offset_ns, uint32_t flags,
                             esvio_fe_feed_info* info);
/* a chunk of rosbag v2.0 bytes (host memory; it may end anywhere; the rule: "rosbag v2.0 recordings" above): the chunk's
 * LEFT events are appended before its RIGHT events, whatever their order in the bytes, then each camera's slicer runs;
 * info[cam] as the other push calls'.  The origin rule holds: a chunk that brings right events while no origin exists
 * and no left event with them is ESVIO_FE_EINVAL, nothing appended, the walker as it was — push a longer chunk, or open
 * the feed with an explicit origin.  Failures as esvio_fe_feed_push_aedat's, for both cameras together: nothing is
 * appended to either, the walker is as it was.  Refused while batches are announced. */
int esvio_fe_feed_push_bag(esvio_fe_handle h, const void* bytes, size_t n_bytes, uint32_t flags, esvio_fe_feed_info info[2]);
/* esvio_fe_feed_push_raw for a chunk of a text event file ("text event files" above; it may end anywhere): the event
 * lines' records are appended; failures as esvio_fe_decode_text's (a malformed line without SKIP_MALFORMED, a BAD
 * line), with nothing appended and the camera's text state as it was */
int esvio_fe_feed_push_text(esvio_fe_handle h, int cam, const esvio_fe_text_format* fmt, const void* bytes, size_t n_bytes,
                            int space, int64_t t_offset_ns, esvio_fe_feed_info* info);
int esvio_fe_feed_peek(esvio_fe_handle h, esvio_fe_feed_window* out);
int esvio_fe_feed_track(esvio_fe_handle h, int pub_this_frame, const esvio_fe_motion* motion, esvio_fe_tracks* out,
                        esvio_fe_batch_info* info);
int esvio_fe_feed_close(esvio_fe_handle h);

/* ---- event images: detector.cur_event_mat_left/right on the device ------------------------ */
/* Every parameter set the reference ships has show_track: 1.  With it trackEvent keeps two CV_8UC3 images,
 * detector.cur_event_mat_left/right: zeroed at feature_tracker.cpp:352-353 (:624-625 in the motion-compensated
 * overload), one pixel written by every createSAE_* call (event_detector.cc:145-146, :164-165, :208-209, :226-227);
 * feature_img is hconcat(left, right) with markers on it (feature_tracker.cpp:1107), the left image unchanged is
 * event_loop in the motion-compensated overload (:863, :1161), and the node publishes them
 * (stereo_event_tracker_node.cpp:64-99, :257-265).  This is the event-proportional part of show_track — one write per
 * event, in stream order — and the part this library takes; the rule below is those lines, in integers.
 *
 * Per handle and camera there is an image E_cam: `height` rows of `width` pixels of 3 bytes (B, G, R), dense and
 * row-major.  It exists only while the setting is on.  For the events of a call, in stream order:
 *   Pixel.   The pixel of event i is the pixel at which that call's SAE update writes event i: for the plain overload
 *            the event's own pixel; for the motion-compensated overload the warped pixel (event_detector.cc:128-129
 *            feeds both :135 and :145), for both cameras.  An event the SAE update skips (x >= width or y >= height;
 *            the warp itself drops none: where the warped pixel leaves the sensor the event keeps its own) writes
 *            nothing.
 *   Colour.  E[pixel] = (255, 0, 0) if the event's polarity byte is non-zero, else (0, 0, 255).
 *   Order.   Later events overwrite earlier ones.  Stamps are never looked at: equal, decreasing or stepping-back
 *            stamps change nothing.  ignore_polarity and feature_filter_threshold play no part.
 * What each call does to the images:
 *   Stage calls (esvio_fe_create_sae, _stereo, _stereo_mc) ACCUMULATE: they apply the rule to the images as they are
 *     and clear nothing — what the reference's createSAE_* do to whatever Mat is there.
 *   Plain track calls — esvio_fe_track_event, esvio_fe_track_event_mc and everything that ends in them: _fields,
 *     _filtered, esvio_fe_track_batch, esvio_fe_track_raw, esvio_fe_track_aedat, esvio_fe_feed_track — set both images
 *     to zero, then apply the rule to the arrays their SAE update consumes (filtered calls: the kept records).
 *   A call that skips a camera's SAE update leaves that camera's image zero: nR = 0, the one-shot right image of
 *     esvio_fe_import_image, a batch committed by esvio_fe_sae_slice_commit (both cameras).
 *   esvio_fe_reset zeroes both images; the setting survives, like esvio_fe_set_detector's.  esvio_fe_track_image
 *     ignores the setting.  The time-slice entry points that run on scratch planes (esvio_fe_sae_slice_last, _apply)
 *     write nothing.
 *
 * esvio_fe_set_event_images(on) waits for the handle's streams and, for on != 0, allocates everything the feature
 * needs — on == 1: 14 bytes per pixel for the two cameras and 6 for the canvas; pixel-proportional only, so no later
 * call allocates for it — and leaves both images zero; on == 0 releases the memory.  A handle that never turns the
 * setting on allocates nothing and launches nothing for it.
 * on == ESVIO_FE_EVENT_IMAGES_AHEAD (2): the images follow announced batches.  esvio_fe_set_next_batch and _mc are
 *   accepted, and an announced batch's prefetch sequence — which runs whole frames ahead of the batch's track call, on
 *   the prefetch stream — applies "zero, then the rule" (the warped pixels for _mc, in both forms of the update; a zero
 *   right image for nR = 0) to an image set of the BATCH's.  There is one set (both cameras, 14 bytes per pixel, its
 *   mark planes included) for the frame being tracked and one per batch that can be prefetched, three: 4 x 14 + 6 =
 *   62 bytes per pixel, all allocated by this call — which is why it is a mode of its own: mode 1 keeps its 20.  After
 *   ANY track call returns — a plain one, one that takes up an announced batch, a lazily returned one — the getters
 *   give the images of the batch that call tracked: never those of a batch announced or prefetched later, although
 *   its update has run, and byte for byte what mode 1 gives for the same batches tracked by plain calls.  A getter
 *   waits for the writes to that one set and not for later batches' prefetch work.  A set is rewritten whole by the
 *   batch that gets it next, so frames whose images nobody fetches leave nothing behind.  esvio_fe_reset zeroes every
 *   set.  Stage calls and esvio_fe_clear_event_images work on the set the getters read.  Everything else is mode 1's.
 *   No stream is added: a stream takes a hardware queue from the process's pool.  What the mode costs the replay
 *   schedule is measured in KERNELS.md "Event images".
 * esvio_fe_clear_event_images is the Mat::zeros of feature_tracker.cpp:352-353 for a host that drives the stage calls
 * itself.
 * The getters: dst is host memory of any kind, or device memory (`space`); esvio_fe_get_event_image writes
 * width*height*3 bytes, esvio_fe_get_event_canvas hconcat(left, right) (:1107): height rows of 2*width*3 bytes.  A
 * getter orders itself behind every write to the image on whichever stream made it (in a plain track call the right
 * camera's update runs on the stereo stream), waits for its own result and touches nothing of the tracker.  After a
 * lazily returned call (esvio_fe_set_lazy_new_stereo) the getters already give that batch's images: they read
 * events, not LK results.
 * ESVIO_FE_EINVAL with a message, before any device work: a getter or esvio_fe_clear_event_images while the setting is
 * off; cam outside 0..1; a null dst; a bad space; esvio_fe_set_event_images with a value other than 0, 1, 2, or
 * with any value while batches are announced; esvio_fe_set_next_batch and _mc while the setting is 1.  (The kernel's
 * per-pixel key holds the event's index in its camera's array in 31 bits; every entry point above already refuses
 * batches of 2^31 events and more.)
 * Out of scope: the time-surface and esvio_fe_get_sae taps of the tracked frame under announced batches (they keep
 * their "latest prefetched batch" meaning); the markers, arrows and the two gray canvases (feature_img_two, pointfeature_img_two), which the host composes from
 * esvio_fe_get_time_surface / esvio_fe_export_image with the cv::circle and cv::arrowedLine calls it already has — at
 * most 300 of them a frame; the time-sliced and camera splits beyond "skipped camera = zero image";
 * prev_event_mat_left (written and never read in the reference); sensor_msgs serialisation. */
#define ESVIO_FE_EVENT_IMAGES_AHEAD 2
int esvio_fe_set_event_images(esvio_fe_handle h, int on); /* 0, 1 as above; 2: the images follow announced batches */
int esvio_fe_clear_event_images(esvio_fe_handle h);
int esvio_fe_get_event_image(esvio_fe_handle h, int cam, uint8_t* dst, int space);
int esvio_fe_get_event_canvas(esvio_fe_handle h, uint8_t* dst, int space);

/* ---- keyframes: the image passes of the loop-closure keyframe (pose_graph) -------------------- */
/* Every shipped parameter set has loop_closure: 1, and the image behind it is the left frame-camera topic
 * (loop_closure_topic, config/.../esvio.yaml), which this library already holds as dense gray on the device
 * (esvio_fe_decode_bag_images, esvio_fe_convert_image, esvio_fe_track_image_space).  For every keyframe
 * KeyFrame::KeyFrame (pose_graph/src/keyframe.cpp:34-63) runs, on one CPU core: cv::GaussianBlur(9x9, sigma 2) of the
 * frame — twice, with the same result, inside DVision::BRIEF::compute (ThirdParty/DVision/BRIEF.cpp:46-62; from
 * computeWindowBRIEFPoint, keyframe.cpp:116-127, and computeBRIEFPoint, :133-161) —, cv::FAST(image, keypoints, 20,
 * true) (:138), 256 BRIEF tests per window point and keypoint (BRIEF.cpp:84-106), liftProjective of every keypoint
 * (:153-160), and for every loop candidate the brute-force Hamming search searchByBRIEFDes / searchInAera (:183-232).
 * These calls are those passes.  DBoW2's words, database and query are the next group ("loop detection" below); PnP, the
 * 4-DoF optimisation, the cv::resize of pose_graph_node.cpp:418-420 and the 80 x 60 thumbnail stay with the host.  This text is the specification; all of it is integer arithmetic except
 * one float addition.
 *
 * B(I), the blur — cv::GaussianBlur(I, Size(9,9), 2, 2) for CV_8UC1, BORDER_REFLECT_101:
 *   taps c = {7, 17, 32, 46, 52, 46, 32, 17, 7}, sum 256: getGaussianKernel(9, 2.0) x 256, rounded (plain rounding and
 *   error-diffused rounding give the same nine values);
 *   B[y][x] = (sum_j sum_i c_j c_i I[r(y+j-4)][r(x+i-4)] + 32768) >> 16, r the reflect-101 index (-1 -> 1, n -> n-2);
 *   no rounding between the two passes: the row pass is exact in 16 bits.
 *   This is OpenCV 4.2's fixed-point 8-bit path RESTATED FROM RECALL: it is UNPINNED — no vector of a compiled OpenCV
 *   backs it here (tests/test_kf_vs_cv2.py is the kit that pins it where cv2 is at hand).
 * F(I, t), the corners — cv::FAST(I, kps, t, true), TYPE_9_16:
 *   for 3 <= x < W-3, 3 <= y < H-3 a pixel is a corner at barrier b when 9 contiguous of the 16 pixels of the radius-3
 *   ring (circular; the ring of esvio_fe_fast_corners) are all > I + b or all < I - b;
 *   score = the largest b at which it still is one: max over the 16 arcs of the arc's min |difference|, minus 1; the
 *   score of every pixel that is no corner at barrier t is 0;
 *   kept: the corners at barrier t whose score is strictly greater than all 8 neighbours' scores — so a corner of
 *   score 0 (possible at t = 0 only) is never kept; order: raster (y, then x);
 *   a kept corner is cv::KeyPoint(x, y, 7.f, -1, score): the calls return (float)x, (float)y and the score.
 *   RESTATED FROM RECALL and UNPINNED like B (the same kit); stated this way it is a definition a test can brute-force.
 * D(Bimg, p), the descriptor — BRIEF::compute(..., treat_image = false), BRIEF.cpp:84-106, with the pattern of
 *   brief_pattern.yml as BriefExtractor loads it (keyframe.cpp:623-640): 256 tests (x1, y1, x2, y2)_i;
 *   X1 = (int)(p.x + (float)x1_i): ONE float addition rounded to nearest, then truncation toward zero, and so for the
 *   other three — p.x + x1 = -0.5 gives 0 and is inside, -1.0 is outside, 0.99999994f + 24 is 25;
 *   bit i = 1 exactly when all four coordinates lie inside the image and Bimg[Y1][X1] < Bimg[Y2][X2];
 *   output: 8 little-endian uint32 per point, bit i in word i >> 5 at bit i & 31 — boost::dynamic_bitset's bit i, so
 *   DBoW2 takes the words unchanged;
 *   the reference converts a non-finite coordinate with undefined behaviour; here a point with a non-finite
 *   coordinate, or with |coordinate| >= 32768, gets the all-zero descriptor.
 * M(Q, T), the match — searchInAera, keyframe.cpp:183-212: for a query q, dist = min_i popcount(q xor T_i), idx the
 *   FIRST i that reaches it; only distances below ESVIO_FE_KF_BEST_INIT qualify, otherwise idx = -1, dist = 128;
 *   status = (idx >= 0 && dist < ESVIO_FE_KF_MATCH_DIST).
 *
 * Images are width*height bytes of the handle's size, dense; every other size has to be brought to it by the host.
 * ESVIO_FE_HOST images are copied to the device first, ESVIO_FE_DEVICE images are read in place.  img == NULL: the
 * plane esvio_fe_export_image(h, cam, ...) returns (cam 0 except in esvio_fe_kf_describe), read in place and ordered
 * after the work that renders it; refused when cfg.equalize != 0 — the pose graph sees the raw frame, not the CLAHE
 * image.  Every call orders itself on the main stream, waits for its own result and touches nothing of the tracker:
 * made between two track calls, announced batches or not, it changes no later result.  Scratch (the blurred plane, the
 * FAST map and lists — esvio_fe_fast_corners' own —, point and descriptor buffers) is allocated on first use; the
 * second call of a size allocates nothing.  Descriptors in ESVIO_FE_DEVICE memory are 16-byte aligned (esvio_fe_mem_alloc's
 * are).  ESVIO_FE_EINVAL with a message, before any device work: a bad space; a threshold outside 0..255; a negative
 * count or capacity, n or nq above 2^20, nt above 2^20; a null buffer with a non-zero count; dst overlapping img; a
 * device descriptor pointer that is not 16-byte aligned; a descriptor call before esvio_fe_kf_set_pattern; cam outside
 * 0..1.  A null handle: ESVIO_FE_EINVAL.
 *
 * esvio_fe_kf_set_pattern: the four arrays of the pattern file (host int32, n must be 256, every |value| <= 127; the
 *   host parses the YAML).  A setting like esvio_fe_set_detector's: it survives esvio_fe_reset.
 * esvio_fe_kf_blur: dst = B(img), width*height bytes in dst_space.
 * esvio_fe_kf_fast: F(img, threshold).  *n_out is always the full count; at most `capacity` entries, the first ones,
 *   are written to out_xy (x, y float pairs) and out_score (may be NULL).  *n_detected (may be NULL): the corners at the
 *   barrier before the non-max.
 * esvio_fe_kf_brief: D(blurred, p) at the n (x, y) float pairs of pts (host) -> n x 8 words in desc_space.
 * esvio_fe_kf_match: M for nq queries against nt train descriptors, both in `space`; idx, dist (int32) and status
 *   (bytes) on the host.  nq == 0 and nt == 0 succeed; with nt == 0 every result is -1 / 128 / 0.
 * esvio_fe_kf_describe: the two compute*BRIEFPoint calls of the constructor — ONE blur; F on the UNBLURRED image;
 *   D at the window points and at the kept corners on the blurred image; kp_norm[i] = (float)(x/z), (float)(y/z) of
 *   liftProjective(kp_xy[i]) in double with cfg.cam[cam] (keyframe.cpp:156-158).  out: caller-owned buffers;
 *   window_desc (n_window x 8 words) and kp_desc in desc_space — device memory, so that a later esvio_fe_kf_match reads
 *   them in place, or host —, kp_xy / kp_score / kp_norm on the host; kp_capacity and n_kp as capacity and *n_out of
 *   esvio_fe_kf_fast (every kp_* buffer holds the first min(n_kp, kp_capacity) corners; a NULL kp_* buffer is not
 *   written).  The binding in keyframe.cpp: INTEGRATION.md. */
#define ESVIO_FE_KF_BEST_INIT 128
#define ESVIO_FE_KF_MATCH_DIST 80
typedef struct esvio_fe_kf_out {
  uint32_t* window_desc; /* [n_window][8], desc_space */
  float* kp_xy;          /* [kp_capacity][2], host */
  int32_t* kp_score;     /* [kp_capacity], host */
  float* kp_norm;        /* [kp_capacity][2], host */
  uint32_t* kp_desc;     /* [kp_capacity][8], desc_space */
  int32_t kp_capacity;
  int32_t n_kp;          /* out: the full count */
  int32_t n_detected;    /* out: corners before the non-max */
  int32_t desc_space;    /* ESVIO_FE_HOST / ESVIO_FE_DEVICE */
} esvio_fe_kf_out;
int esvio_fe_kf_set_pattern(esvio_fe_handle h, const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2,
                            int n);
int esvio_fe_kf_blur(esvio_fe_handle h, const uint8_t* img, int space, uint8_t* dst, int dst_space);
int esvio_fe_kf_fast(esvio_fe_handle h, const uint8_t* img, int space, int threshold, float* out_xy, int32_t* out_score,
                     int32_t capacity, int32_t* n_out, int32_t* n_detected);
int esvio_fe_kf_brief(esvio_fe_handle h, const uint8_t* blurred, int space, const float* pts, int n, uint32_t* desc,
                      int desc_space);
int esvio_fe_kf_match(esvio_fe_handle h, const uint32_t* query, int nq, const uint32_t* train, int nt, int space,
                      int32_t* idx, int32_t* dist, uint8_t* status);
int esvio_fe_kf_describe(esvio_fe_handle h, int cam, const uint8_t* img, int space, const float* window_pts, int n_window,
                         int fast_threshold, esvio_fe_kf_out* out);

/* ---- loop detection: DBoW2 words, database and L1 query (pose_graph) --------------------------- */
/* What the keyframe's descriptors are computed for: PoseGraph::detectLoop (pose_graph/src/pose_graph.cpp:331-406) hands
 * keyframe->brief_descriptors to DBoW2 — db.query(desc, ret, 4, frame_index - 50), db.add(desc), and a rule on the
 * scores that names the loop candidate or -1.  These calls are that step, so that a keyframe's way from the frame
 * (esvio_fe_kf_describe, descriptors left in device memory) to the candidate (esvio_fe_kf_match) stays on the device.
 * PnP, the 4-DoF optimisation and the DEBUG_IMAGE canvases stay with the host; so do the direct index / FeatureVector
 * (use_di is false, pose_graph.cpp:49), scorings other than L1, delete_entry and the text vocabulary format
 * (creating a vocabulary is the group after this one, "C").  This text is the specification.  Everything is integer arithmetic plus IEEE double additions,
 * subtractions and one division in a stated order; no rule has a product.
 * WHAT IS PINNED: BowVector's addWeight / addIfNotExist / normalize(L1) (ThirdParty/DBoW/BowVector.cpp:34-84) are held
 * to outputs of that file compiled unchanged (tests/golden/bow_vector_ref.npz).  The rest of DBoW2 includes OpenCV and
 * boost; its rules are CITED BY LINE AND RESTATED here, unpinned.  Every vocabulary in these calls' own tests and
 * measurements is synthetic: the shipped brief_k10L6.bin is not at hand ("C" below trains one from descriptors).
 *
 * V, the vocabulary file — ThirdParty/VocabularyBinary.hpp:12-45, VocabularyBinary.cpp:29-37, TemplatedVocabulary.h:
 *   1509-1561 (loadBin): 24 bytes {k, L, scoringType, weightingType, nNodes, nWords}, little-endian int32; nNodes records
 *   of 48 bytes {int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]}; nWords records of 8 bytes {int32
 *   nodeId, int32 wordId}.  Node 0 is the root and is not in the file.  A node's children are in the order in which their
 *   records appear (children.push_back), whatever their ids.  Descriptor bit i is bit i & 63 of descriptor[i >> 6] — the
 *   bit esvio_fe_kf_brief's eight uint32 hold it at, so the words go in unchanged.  weightingType 0..3 = TF_IDF, TF, IDF,
 *   BINARY; scoringType 0 = L1_NORM (BowVector.h:36-53).  A word record sets its node's word id; of two records that
 *   name one node the later stands (`m_nodes[nid].word_id = wid`).
 *   The reference trusts the file.  Here a file that would make it read out of bounds is refused by name
 *   (ESVIO_FE_EINVAL, before any device work): a byte count other than the header implies; nNodes < 1; a nodeId outside
 *   1..nNodes or duplicated; a parentId outside 0..nNodes or equal to its node; a node not reachable from the root; a
 *   root without children; a wordId outside 0..nWords-1 or duplicated; a word on a node that has children (or on a node
 *   outside 1..nNodes); a leaf without a word; a weighting outside 0..3.  Scoring other than L1_NORM: ESVIO_FE_ENOTIMPL.
 * W, the word of a descriptor — TemplatedVocabulary.h:1217-1258, FBrief.cpp:53-57: from the root, go to the child with
 *   the least popcount(d xor child); of equal distances the first in child order (`d < best_d` is strict); stop at a
 *   leaf: its word_id and weight.  The walk follows the tree, not L: leaves at any depth, any child count >= 1.
 * T, the BoW vector — TemplatedVocabulary.h:1065-1121, BowVector.cpp:34-84, ScoringObject.h:73 (L1 scoring normalises
 *   with L1): descriptors whose weight is not > 0 are skipped.  TF_IDF, TF: the value of a word hit c times is w added c
 *   times one after another, ((w + w) + w) + ..., not c * w.  IDF, BINARY: w.  norm = the sum of fabs(value) in ascending
 *   word id, one addition after another from 0.0; if norm > 0.0 every value is divided by it (IEEE division).  The vector
 *   is the list of (word, value) in ascending word id.
 * A, add — TemplatedDatabase.h:408-475: entry id = entries so far; its vector is T(desc); empty vectors make entries too.
 * Q, query — TemplatedDatabase.h:607-723: q = T(desc), N = entries now.  Entry e takes part iff e < max_id ||
 *   max_id == -1 || e == N - 1 (the last entry always does; max_id == -1 admits all; any other max_id <= 0 the last
 *   alone).  For an entry that takes part and shares a word with q, s_e = the sum over the shared words in ascending
 *   word id of fabs(qv - dv) - fabs(qv) - fabs(dv), each term left to right in double, the first term starting the sum;
 *   entries that share no word are absent.  Results by ascending s_e, cut at max_results, then Score = -s_e / 2.0.
 *   The reference orders with std::sort on the score alone, so the order of equal scores is its library's; HERE EQUAL
 *   SCORES ARE ORDERED BY ASCENDING ENTRY ID — this project's own rule (-0.0 and 0.0 are equal; a NaN, which only a
 *   file with non-finite weights produces, is ordered by its bits — the NaN 0x7fffffffffffffff has the largest key
 *   there is and comes last).  max_results is 1..ESVIO_FE_BOW_MAX_RESULTS; the
 *   reference's "all results" form (<= 0) has no caller in ESVIO: ESVIO_FE_EINVAL.
 * L, the loop decision — pose_graph.cpp:347-404: R = Q(desc, ESVIO_FE_BOW_LOOP_RESULTS, frame_index -
 *   ESVIO_FE_BOW_LOOP_GAP), then A(desc).  find = |R| >= 1 && R[0].Score > ESVIO_FE_BOW_LOOP_MIN_FIRST && (exists i >= 1:
 *   R[i].Score > ESVIO_FE_BOW_LOOP_MIN_OTHER).  If find && frame_index > ESVIO_FE_BOW_LOOP_GAP: m = -1; for i = 0..: if
 *   m == -1 || (R[i].Id < m && R[i].Score > ESVIO_FE_BOW_LOOP_MIN_OTHER) then m = R[i].Id; the answer is m.  Otherwise -1.
 *   So R[0] is taken whatever its score is to 0.015, and at frame_index 49 max_id is -1: everything takes part.
 *
 * Conventions: the keyframe group's.  desc: n x 8 words in `space` (ESVIO_FE_HOST: copied first; ESVIO_FE_DEVICE: read
 * in place, 16-byte aligned), 0 <= n <= 2^20.  Every argument error is ESVIO_FE_EINVAL with a message, before any device
 * work; a null handle: ESVIO_FE_EINVAL.  Every call orders itself on the main stream, waits for its own result and
 * touches nothing of the tracker: made between two track calls, batches announced or not, it changes no later result.
 * No track path launches anything of this group; the group's own sort passes are k_radix_pass launches and are counted
 * in that slot of the track path's kernel statistics (esvio_fe_get_kernel_stats) when profiling is on.
 * Every call but esvio_fe_bow_vocabulary_header, _set_vocabulary and _entries is ESVIO_FE_EINVAL before a vocabulary is
 * set.  The vocabulary is a setting and survives esvio_fe_reset; the database is pose-graph state: esvio_fe_reset does
 * not touch it, esvio_fe_bow_clear empties it.
 *
 * esvio_fe_bow_vocabulary_header: checks V on a file image in host memory and fills info; takes no handle and uses no
 *   device.  On a refusal info->message names the item.  max_children: the largest child count; depth: the deepest
 *   leaf's (the root's children are at depth 1); leaves: nodes without children.
 * esvio_fe_bow_set_vocabulary: checks V, lays the tree out for the device (every node's children contiguous in child
 *   order, descriptors apart from weights) and uploads it.  Refused while the database holds entries.
 * esvio_fe_bow_transform: W and T.  word / weight (host, n entries each, either may be NULL): W per descriptor.  bow_word /
 *   bow_value (host): the first min(*n_bow, bow_cap) pairs of T; *n_bow (may be NULL with bow_cap 0) is the full count.
 * esvio_fe_bow_add: A; *entry_id (may be NULL) is the new entry's id.
 * esvio_fe_bow_query: Q; results (host, room for max_results), *n_results how many.
 * esvio_fe_bow_detect_loop: L — the descriptors are transformed once for the query and the add; *loop_index the answer;
 *   results / n_results (both may be NULL): R, room for ESVIO_FE_BOW_LOOP_RESULTS.
 * esvio_fe_bow_entries: the entries now (0 before a vocabulary).  esvio_fe_bow_reserve(h, entries, words): room for that
 *   many entries and that many (word, value) pairs in all; adds and queries inside it allocate nothing beyond the scratch
 *   the first call of a descriptor count allocates.  Without a reserve the pools grow like the other buffers, a quarter
 *   to spare, earlier entries kept.  The binding in pose_graph.cpp: INTEGRATION.md. */
#define ESVIO_FE_BOW_MAX_RESULTS 64
#define ESVIO_FE_BOW_LOOP_RESULTS 4
#define ESVIO_FE_BOW_LOOP_GAP 50
#define ESVIO_FE_BOW_LOOP_MIN_FIRST 0.05
#define ESVIO_FE_BOW_LOOP_MIN_OTHER 0.015
typedef struct esvio_fe_bow_vocabulary_info {
  int32_t k, L;      /* as the header has them; the walk does not use them */
  int32_t scoring;   /* 0: L1_NORM */
  int32_t weighting; /* 0..3: TF_IDF, TF, IDF, BINARY */
  int32_t nodes;     /* nNodes: without the root */
  int32_t words;     /* nWords */
  int32_t leaves;
  int32_t max_children;
  int32_t depth;
  char message[188]; /* "" or what the file is refused for */
} esvio_fe_bow_vocabulary_info;
typedef struct esvio_fe_bow_result {
  int32_t id;
  double score;
} esvio_fe_bow_result;
int esvio_fe_bow_vocabulary_header(const void* bytes, size_t n_bytes, esvio_fe_bow_vocabulary_info* info);
int esvio_fe_bow_set_vocabulary(esvio_fe_handle h, const void* bytes, size_t n_bytes);
int esvio_fe_bow_transform(esvio_fe_handle h, const uint32_t* desc, int n, int space, int32_t* word, double* weight,
                           uint32_t* bow_word, double* bow_value, int32_t bow_cap, int32_t* n_bow);
int esvio_fe_bow_add(esvio_fe_handle h, const uint32_t* desc, int n, int space, int32_t* entry_id);
int esvio_fe_bow_query(esvio_fe_handle h, const uint32_t* desc, int n, int space, int max_results, int max_id,
                       esvio_fe_bow_result* results, int32_t* n_results);
int esvio_fe_bow_detect_loop(esvio_fe_handle h, const uint32_t* desc, int n, int space, int frame_index,
                             int32_t* loop_index, esvio_fe_bow_result* results, int32_t* n_results);
int esvio_fe_bow_clear(esvio_fe_handle h);
int esvio_fe_bow_entries(esvio_fe_handle h);
int esvio_fe_bow_reserve(esvio_fe_handle h, int64_t entries, int64_t words);

/* ---- C, creating a vocabulary: k-means++, the tree, the word weights (DBoW2) ------------------ */
/* The input every call above depends on: TemplatedVocabulary::create with HKmeansStep, initiateClustersKMpp,
 * createWords, setNodeWeights and FBrief::meanValue / distance, from training descriptors to a file image in format V.
 * Paths are under pose_graph/src/ThirdParty/.  Integer arithmetic on 256-bit descriptors throughout; doubles only in the
 * draws (C5) and the weights (C4).  CITED BY LINE AND RESTATED, unpinned, like W to L; this text is the specification.
 * The claim is "equal to create() given the draws of C5 in place of rand()" — not equal to any particular run of the
 * reference, which seeds rand() from the clock.
 *
 * Input: n descriptors of 8 words, grouped into n_docs documents (images) by doc_offsets[0..n_docs]: ascending,
 *   doc_offsets[0] = 0, doc_offsets[n_docs] = n.  Empty documents are allowed and count in NDocs.  The flat order is
 *   document order (getFeatures, DBoW/TemplatedVocabulary.h:618-634).  Parameters: k, L, weighting 0..3, scoring (0
 *   only), seed, max_passes.
 * C1, a node's step — HKmeansStep, TemplatedVocabulary.h:639-816, for a node with m features in order (m = 0 never
 *   occurs: :642 returns at once, and only nodes with features are made).  m <= k (:657-667): one cluster per feature, in
 *   order, the centre the feature itself; duplicates stay duplicates.  m > k: the centres are seeded by C2, then passes
 *   repeat.  A pass after the first recomputes every centre by C3 from the previous pass's groups; every pass assigns each
 *   feature to the centre with the least popcount(f xor c), of equal distances the lowest cluster index (`dist <
 *   best_dist` is strict, :731-742).  The loop ends after the first pass, the very first not counted, whose assignment
 *   equals the previous pass's (:753-769); the clusters are the centres that pass used, the groups its assignment, a
 *   group in the node's feature order.  Every cluster becomes a child of the node in cluster order, its id
 *   m_nodes.size() at the push (:783-790).  If current_level < L, each child whose group has more than one feature is
 *   split in turn, child 0's whole subtree first (:793-815).  So: ids are the depth-first creation order; a child with
 *   one feature, or with none, is a leaf at any depth; a node has 1..k children.
 * C2, k-means++ seeding — initiateClustersKMpp, :831-912.  The first centre is feature RandomInt(0, m - 1).
 *   min_dist[i] starts as the distance to it.  While fewer than k centres exist: every feature with min_dist > 0 takes
 *   the minimum with its distance to the newest centre (the first time round that is the first centre again and changes
 *   nothing — stated, not imitated); dist_sum = the sum, exact, the terms being integers; dist_sum == 0 ends the seeding
 *   with fewer than k centres (:907-908); else cut_d = RandomValue<double>(0, dist_sum), drawn again while cut_d == 0.0;
 *   the new centre is the first feature whose running sum of min_dist in feature order, as a double, is >= cut_d, or the
 *   last feature if none (:892-904).
 * C3, the mean — DBoW/FBrief.cpp:22-49: bit i of the centre is set iff more than floor(m_c / 2) of the group's m_c
 *   features have it set; an empty group gives the all-zero descriptor (:25-27).  Empty groups are common on clustered
 *   descriptors: centres that collapse onto one majority pattern lose every feature but the first's.
 * C4, words and weights — createWords :917-937, setNodeWeights :942-995, Node().  Word ids go to the leaves in ascending
 *   node id.  Nodes with children weigh 0.0.  TF and BINARY: every word weighs 1.0.  TF_IDF and IDF: Ni[w] = the documents
 *   with at least one feature whose walk W (above, on the finished tree) ends in word w; the weight is log((double)NDocs
 *   / (double)Ni) by the host's libm, or 0.0 where Ni == 0 (empty clusters; the later of two equal features of an m <= k
 *   node).
 * C5, the draws — the project's own rule: a draw is a function of (seed, node, index), so that any order of evaluating
 *   the nodes sees the same numbers.  mix(z) is splitmix64's step: z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 *   0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31, all modulo 2^64.  key(root) = mix(seed);
 *   key(child c of n) = mix(key(n) ^ (uint64)(c + 1)), c the cluster index.  Draw j = 0, 1, ... of node n in the order C2
 *   takes them: r = mix(key(n) ^ ((uint64)(j + 1) << 32)) >> 33, 31 bits, glibc's rand() range.  RandomInt(0, m - 1) =
 *   (int)(((double)r / 2147483648.0) * (double)m) (DUtils/Random.cpp:47-50); RandomValue<double>(0, s) = ((double)r /
 *   2147483647.0) * s (DUtils/Random.h:56-68), as IEEE double operations.
 * C6, the output: a file image in format V that loadBin reads and esvio_fe_bow_vocabulary_header accepts; node records
 *   in ascending nodeId (which is child order), word records in ascending wordId; k, L, scoring, weighting as given.
 * C7, refused with ESVIO_FE_EINVAL and a message, before any device work: n < 1 or n > 2^24; k outside 2..32; L outside
 *   1..10; a weighting outside 0..3; offsets that are not as stated; a misaligned device pointer; a negative max_passes.
 *   A scoring other than 0: ESVIO_FE_ENOTIMPL.
 * The project's own guard: the reference's loop has no bound.  If a node has not settled after max_passes assignment
 *   passes (0 means 100) the call fails with ESVIO_FE_EINVAL, the message naming how many nodes of the first level that
 *   has any; nothing is stored.
 *
 * esvio_fe_bow_create_vocabulary: desc in ESVIO_FE_HOST memory is copied first, in ESVIO_FE_DEVICE memory it is read in
 *   place (16-byte aligned); doc_offsets, params and info are host memory.  The call orders itself on the main stream and
 *   waits for its own result.  It touches neither the tracker nor the vocabulary that is set nor the database: made
 *   between two track calls, batches announced or not, it changes no later result.  On failure info holds the message
 *   and zeros.
 * esvio_fe_bow_get_created: the image of the last successful create, info.bytes bytes, into host memory of `cap` bytes
 *   (ESVIO_FE_EINVAL if there is none or cap is too small).  The image lives until the next successful create or
 *   esvio_fe_destroy; esvio_fe_reset keeps it.  Using it is the caller's esvio_fe_bow_set_vocabulary on the bytes.
 *   Where a maintainer calls this, offline: INTEGRATION.md. */
typedef struct esvio_fe_bow_create_params {
  int32_t k, L;
  int32_t weighting;  /* 0..3: TF_IDF, TF, IDF, BINARY */
  int32_t scoring;    /* 0: L1_NORM */
  int32_t max_passes; /* 0: 100 */
  int32_t reserved;
  uint64_t seed;
} esvio_fe_bow_create_params;
typedef struct esvio_fe_bow_create_info {
  int32_t nodes, words, depth, max_children; /* as esvio_fe_bow_vocabulary_info has them */
  int32_t kmeans_nodes;   /* nodes with more than k features */
  int32_t passes;         /* the most assignment passes any node needed under C1 (0 without a k-means node) */
  int32_t empty_clusters; /* final clusters of k-means nodes without a feature */
  int32_t short_seedings; /* nodes whose seeding stopped at dist_sum == 0 */
  uint64_t bytes;         /* size of the file image */
  char message[188];      /* "" or why the call failed */
} esvio_fe_bow_create_info;
int esvio_fe_bow_create_vocabulary(esvio_fe_handle h, const uint32_t* desc, int64_t n, int space, const int64_t* doc_offsets,
                                   int32_t n_docs, const esvio_fe_bow_create_params* params, esvio_fe_bow_create_info* info);
int esvio_fe_bow_get_created(esvio_fe_handle h, void* out, size_t cap);

/* ---- camera split across GPUs (BASELINE config C4) ----------------------- */
/* The left and right cameras have disjoint SAE state (sae_/sae_latest_ vs sae_right/
 * sae_latest_right, event_detector.h:74-79), so a second GPU can own the right camera: it runs
 * esvio_fe_create_sae(cam=1) + esvio_fe_sae_to_time_surface(cam=1, t_sync = LEFT batch end,
 * feature_tracker.cpp:367-368) and ships the 1-byte/pixel image.  export: copy the current image
 * of `cam` into a contiguous width*height buffer (host or device).  import: hand the left GPU's
 * handle the right image for the NEXT esvio_fe_track_event call (one shot), which then skips the
 * right camera's SAE update and rendering (pass nR = 0) and uses this image for stereo LK. */
int esvio_fe_export_image(esvio_fe_handle h, int cam, uint8_t* dst, int space);
int esvio_fe_import_image(esvio_fe_handle h, int cam, const uint8_t* src, int space);

/* ---- one stream time-sliced across GPUs (BASELINE config C5) ------------- */
/* createSAE_left/right (event_detector.cc:149-166) for ONE batch cut into N consecutive slices of the
 * stream, one per GPU.  Every rank holds the planes as they were before the batch.  Per batch:
 *   1. rank r: esvio_fe_sae_slice_last(its slice) -> last_r: per (camera, pixel, polarity) the time of
 *      the slice's last event, ESVIO_FE_SLICE_NONE where it has none (L[p] = t is unconditional,
 *      :158, so this does not depend on what came before);          all-gather last_0..last_{N-1}
 *   2. rank r: esvio_fe_sae_slice_apply(its slice, last_0..last_{r-1}) -> s_r: the time of the
 *      slice's last event that PASSES `t > L[p] + thr || L[!p] > L[p]` (:155), evaluated with the
 *      exact carried-in L (planes before the batch overlaid with the earlier slices), NONE where no
 *      event passes — the decisions are the sequential loop's for any timestamps; all-gather s_r
 *   3. every rank: esvio_fe_sae_slice_commit(all last, all s): planes after the batch = planes
 *      before it overlaid with the slices in order.  The next esvio_fe_track_event call on this
 *      handle then takes the batch's SAE update as done (it still needs the batch's left events
 *      for Arc*) — one shot, like esvio_fe_import_image.
 * A plane set is esvio_fe_sae_plane_doubles(h) = 2 cameras x width*height x 2 polarities doubles in
 * the handle's own order (opaque to the caller; it only travels between handles of the same size).
 * Not to be mixed with esvio_fe_set_next_batch. */
#define ESVIO_FE_SLICE_NONE (-1.0)
size_t esvio_fe_sae_plane_doubles(esvio_fe_handle h);
int esvio_fe_sae_slice_last(esvio_fe_handle h, const esvio_fe_event* left, size_t nL,
                            const esvio_fe_event* right, size_t nR, int space, double* last_out,
                            int out_space);
int esvio_fe_sae_slice_apply(esvio_fe_handle h, const esvio_fe_event* left, size_t nL,
                             const esvio_fe_event* right, size_t nR, int space,
                             const double* last_before /* [n_before] plane sets */, int n_before,
                             int in_space, double* s_out, int out_space);
int esvio_fe_sae_slice_commit(esvio_fe_handle h, const double* last_all, const double* s_all,
                              int n_slices, int space);

/* ---- event memory ------------------------------------------------------------------------- */
/* Memory for event batches from the HIP runtime the library itself is linked to (a process may hold a
 * second one, e.g. the copy PyTorch bundles).  ESVIO_FE_HOST: pinned host memory — a batch kept there
 * (a dvs_msgs::EventArray_<Allocator> whose allocator calls this, or a buffer the driver's callback
 * deserialises into) goes to the device as one DMA, without the staging copy pageable memory needs.
 * ESVIO_FE_DEVICE: device memory on the current device; esvio_fe_mem_upload fills it from host memory
 * (synchronous).  Freed with esvio_fe_mem_free(space, p). */
int esvio_fe_mem_alloc(int space, size_t bytes, void** out);
int esvio_fe_mem_free(int space, void* p);
int esvio_fe_mem_upload(void* dst_device, const void* src_host, size_t bytes);
/* ... or the caller's own storage, page-locked where it lies: esvio_fe_register_host_buffer(p, bytes) once for a
 * buffer that event batches are handed over from again and again (the deserialisation buffer of the driver callback,
 * a ring of EventArray storage, stereo_event_tracker_node.cpp:128-142,399) — every later batch inside [p, p + bytes)
 * then crosses PCIe straight from there: no staging copy by the CPU at all.  Registering costs a system call and
 * a page walk (~0.1 ms per MB): per buffer, not per batch.  esvio_fe_unregister_host_buffer(p) before the memory
 * is freed.  (hipHostRegister / hipHostUnregister through the library's own HIP runtime.) */
int esvio_fe_register_host_buffer(void* p, size_t bytes);
int esvio_fe_unregister_host_buffer(void* p);

/* ---- capacity ----------------------------------------------------------------------------- */
/* Every event-proportional device buffer (partition scratch, candidate sets, staging lanes) grows on
 * demand, by a hipFree + hipMalloc inside the call that first needs more — a stall of 0.1-2 ms in the
 * middle of a stream.  esvio_fe_reserve makes them all large enough for batches of up to
 * max_events_left + max_events_right events (and for max_events_left Arc* candidates in every candidate
 * set) now, so that no call below that size allocates (esvio_fe_latency.allocs counts the ones that
 * do); with host_batches != 0 also the staging slots of batches handed over in ESVIO_FE_HOST memory
 * (8 slots of 32 B per event, half of it pinned).  Not while batches are announced.  The reference has
 * no counterpart: its std::vectors grow inside the callbacks. */
int esvio_fe_reserve(esvio_fe_handle h, size_t max_events_left, size_t max_events_right, int host_batches);

#ifdef __cplusplus
}
#endif
#endif /* ESVIO_FE_H */
