// fe_kernels.h — internal launch API of the gfx950 kernels (fe_kernels.hip).
// Not part of the public boundary; the C ABI is include/esvio_fe.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace esvio {


// dvs_msgs::Event, 16 B AoS (reference: feature_tracker/src/dvs_msgs/Event.h:42-52)
struct __attribute__((aligned(16))) EventRec {
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t pol;
  uint8_t pad[3];
};
static_assert(sizeof(EventRec) == 16, "event record must be 16 B");

constexpr int kPad = 24;        // image border kept around every pyramid level (>= LK win 21)
constexpr int kMaxLevels = 4;   // LK maxLevel 3 -> 4 levels
constexpr int kLkWin = 21;      // cv::Size(21,21) at every call site (feature_tracker.cpp:410..495)
constexpr int kArcBlock = 256;  // events per block of the Arc* kernel
constexpr int kMaxDiscR = 63;   // max min_dist supported by the selection kernel

// One image pyramid resident in HBM.  Level l is stored padded by kPad on every side
// (BORDER_REFLECT_101 for the image, zeros for the Scharr derivatives), row stride
// w[l]+2*kPad; pointers address the padded buffer's origin.
struct PyrDesc {
  uint8_t* img[kMaxLevels];
  int16_t* deriv[kMaxLevels];  // interleaved (Ix,Iy), same stride (in pixels) as the image
  int w[kMaxLevels], h[kMaxLevels];
  int stride[kMaxLevels];  // row stride in pixels: (w + 2*kPad) rounded up to 16
  int levels;  // maxLevel (inclusive) actually built
};
inline int pyr_stride(int w) { return (w + 2 * kPad + 15) & ~15; }

// Slots of the per-kernel timers (esvio_fe_set_profiling): one per kernel FUNCTION, named as rocprofv3 names it
// (kKernelNames, fe_ctx.h), so that a bench line's `kernels` can be matched with a profile without a table.  A
// launch site that picks between forms (k_lk / k_lk_f32, k_time_surface4 / k_time_surface, the selection kernels)
// books the one it launched.  The few slots that cover more than one function say so in their name's comment.
enum KernelId {
  K_TILE_HIST = 0,   // (+ k_mc_warp in front of it for a motion-compensated batch)
  K_TILE_SCAN,
  K_TILE_SCATTER,
  K_TILE_APPLY,
  K_SAE_KEYS,        // the radix-sort form of the update: k_sae_keys, k_radix_pass, k_sae_apply (_ev, _ev_write)
  K_RADIX_PASS,
  K_SAE_APPLY,
  K_TIME_SURFACE4,
  K_TIME_SURFACE,
  K_MEDIAN,
  K_CLAHE,           // k_clahe_lut, k_clahe_interp (k_normalize in the unfused form)
  K_NORM_PYR,
  K_PYR3,
  K_PYR_DOWN,
  K_PYR_PAD,
  K_SCHARR,
  K_PAD_SCHARR,
  K_LK_F32,
  K_LK,
  K_ARC_MAP,         // (+ k_arc_mark where the SAE update has not left the touched flags)
  K_ARC_EV,
  K_DEDUP,
  K_COMPACT,
  K_SELECT_MW,
  K_SELECT,
  K_SELECT_GBM,
  K_FAST_SCORE,      // (appended: the ids above keep their meaning)
  K_FAST_COLLECT,
  K_EVENTS_FROM_FIELDS,
  // ---- from here on: kernels of stages that no track call launches (kTrackKernels below).  A kernel of a track path
  // is appended ABOVE this line — the ids below move up by one; nothing outside the library holds them as numbers
  K_BAF_HEADS,       // esvio_fe_filter_events (its key and sort launches are booked as K_SAE_KEYS / K_RADIX_PASS)
  K_BAF_FILTER,
  K_BAF_COUNT,
  K_BAF_SCAN,
  K_BAF_EMIT,
  K_BAF_KEYS_FIELDS, // esvio_fe_filter_batch on field arrays (its heads launch is booked as K_BAF_HEADS)
  K_BAF_EMIT_FIELDS,
  K_RAW_REDUCE,      // esvio_fe_decode_raw / esvio_fe_track_raw: the decode chain runs in front of the track call
  K_RAW_SCAN,
  K_RAW_EMIT,
  K_SLICE_REDUCE,    // esvio_fe_slice_events: cutting a record stream into fixed-rate windows
  K_SLICE_SCAN,
  K_SLICE_CUTS,
  K_BAF_KEYS_ADDR,   // the filter's record form with an address stage set (in k_sae_keys' place)
  K_HOT_COUNT,       // esvio_fe_hot_learn (records and fields)
  K_HOT_KEYS,        // esvio_fe_hot_select: keys of the count plane (its sort is booked as K_RADIX_PASS), then the pick
  K_HOT_PICK,
  K_TRIG_REDUCE,     // esvio_fe_decode_triggers (its scan launch is k_raw_scan, booked as K_RAW_SCAN)
  K_TRIG_EMIT,
  K_COUNT
};
// esvio_fe_kernel_count(): the kernels of the tracker's entry points, the table bench.py and the recorded launch traces
// list.  The ids from here on belong to stages off every track path and are listed by esvio_fe_stage_kernel_count().
constexpr int kTrackKernels = K_BAF_HEADS;
static_assert(K_EVENTS_FROM_FIELDS + 1 == kTrackKernels && K_TRIG_EMIT + 1 == K_COUNT,
              "a track-path kernel goes in front of K_BAF_HEADS (and into this assertion), a stage's kernel behind it");

// ---- SAE update -------------------------------------------------------------------------
// Bounds of the device-side waits (every one gives up instead of hanging the GPU; the host then fails
// the call or redoes the launch).  They are launch parameters so that a test can make a wait expire on
// demand (esvio_fe_debug_inject, fe_ctx.h: WaitLimits).
constexpr uint32_t kSpinLookback = 1u << 20;  // k_radix_pass: polls of an earlier tile's look-back word
constexpr uint32_t kSpinTicket = 1u << 21;    // k_tile_apply: polls of the block's turn ticket
constexpr unsigned long long kTicksPoll = 2000000ull;   // k_lk waiting for k_select's corner: 20 ms
constexpr unsigned long long kTicksChain = 4000000ull;  // k_lk waiting for the previous frame's k_lk: 40 ms

constexpr int kRadixTile = 2048;  // keys per block
constexpr int kRadixMaxBits = 8;
constexpr int kRadixMaxPasses = 4;
inline uint32_t radix_blocks(uint32_t n) { return (n + kRadixTile - 1) / kRadixTile; }
// sort scratch layout (uint32 words): [ghist: passes<<bits][tickets: passes] cleared by k_sae_apply,
// then [lookback: passes * radix_blocks(n) << bits] cleared by k_sae_keys.  The only place that computes an offset
// into it (host-only arithmetic, inline like make_tile_geom below).
constexpr uint32_t kSortTickets = (uint32_t)kRadixMaxPasses << kRadixMaxBits;  // behind the largest ghist
constexpr uint32_t kSortHeadWords = kSortTickets + 64;
static_assert(kSortTickets == 1024 && kSortHeadWords == 1088, "sort scratch layout moved");
struct SortScratch {
  uint32_t* ghist;      // [passes << bits]
  uint32_t* tickets;    // [passes]
  uint32_t* lookback;   // [passes][radix_blocks(n) << bits]
  uint32_t head_words;  // ghist + tickets: what k_sae_apply clears
};
inline size_t sort_scratch_words(size_t cap) {  // for sorts of up to cap pairs, whatever (passes, bits)
  return kSortHeadWords + (size_t)kRadixMaxPasses * ((size_t)radix_blocks((uint32_t)cap) << kRadixMaxBits);
}
inline SortScratch sort_scratch(uint32_t* base) {
  return SortScratch{base, base + kSortTickets, base + kSortHeadWords, kSortHeadWords};
}
// keys[i] = cam*P + y*W + x (or invalid_key for out-of-sensor events), vals[i] = i, for the
// virtual concatenation [left; right]; also fills the per-pass global digit histograms.
void launch_sae_keys(hipStream_t s, const EventRec* evL, uint32_t nL, const EventRec* evR,
                     uint32_t nR, int W, int H, uint32_t* keys, uint32_t* vals,
                     uint32_t invalid_key, unsigned long long* n_rejected, int passes, int bits,
                     uint32_t* ghist, uint32_t* lookback, uint32_t lookback_words,
                     const struct McParams* mc /* NULL: no motion compensation */);
// one stable LSD pass on digit (key >> shift) & ((1<<bits)-1) with decoupled look-back
// n_dev (optional): the number of pairs is *n_dev, known on the device only, and n its upper bound — the launch is
// sized for n, a block whose tile lies behind *n_dev ends at once
void launch_radix_pass(hipStream_t s, const uint32_t* keys_in, const uint32_t* vals_in, uint32_t n,
                       int shift, int bits, const uint32_t* ghist, uint32_t* lookback,
                       uint32_t* ticket, uint32_t* keys_out, uint32_t* vals_out, int* err,
                       uint32_t spin_limit = kSpinLookback, const uint32_t* n_dev = nullptr);
// walk every same-pixel segment of the sorted keys in stream order applying the SAE rule
// (event_detector.cc:149-166). L2/S2: double2 per (cam,pixel): {L[0],L[1]} and {S[0],S[1]}.
void launch_sae_apply(hipStream_t s, const uint32_t* keys, const uint32_t* vals, uint32_t n,
                      const EventRec* evL, uint32_t nL, const EventRec* evR, double2* L2,
                      double2* S2, double filter_threshold, uint32_t invalid_key,
                      uint32_t* sort_scratch, uint32_t sort_scratch_words);
// the same update with one lane per EVENT instead of one per pixel (see k_sae_apply_ev): for batches
// with many events per pixel, where the per-pixel walk leaves most lanes idle
void launch_sae_apply_ev(hipStream_t s, const uint32_t* keys, const uint32_t* vals, uint32_t n,
                         const EventRec* evL, uint32_t nL, const EventRec* evR, double2* L2,
                         double2* S2, double filter_threshold, uint32_t invalid_key,
                         uint32_t* sort_scratch, uint32_t sort_scratch_words, uint8_t* marks /* [n] */);

// ---- SAE update, tiled form (default) --------------------------------------------------------
// The sensor is cut into tiles of tw x th pixels; a tile of one camera is a bucket.  One stable
// partition of the event records by bucket (k_tile_hist + k_tile_scan + k_tile_scatter: one digit of
// <= 11 bits, no atomics or spins across blocks; the partitioned records are 8 bytes — tile-local
// pixel, polarity, seconds relative to the batch's smallest, nsec — whenever the batch's stamps allow
// it, else the raw 16), then one block per bucket applies its events in stream order with the tile's
// L planes in LDS (k_tile_apply).  Replaces key generation + 3 radix passes over (key, index) pairs +
// a gathering apply: per event 16 B are read twice, 8 written and 8 read.
// points (= waves) of an LK launch per workgroup; in the float-order mode a workgroup's 122 KB of LDS make it the only
// one on its CU (fe_kernels.hip kLkWaves; what the host needs it for: esvio_fe_ctx::waits_fit_*)
#ifndef ESVIO_LK_WAVES
#define ESVIO_LK_WAVES 4
#endif
constexpr int kLkPointsPerBlock = ESVIO_LK_WAVES;

struct TileGeom {
  int W, H;
  int tw, th;            // tile size in pixels (tw * th <= kTileMaxPx)
  int tiles_x, tiles_y;  // tiles per camera
  int nt_cam;            // tiles_x * tiles_y
  int nbins;             // 2 * nt_cam + 1 (last bin: out-of-sensor events)
  int bits;              // ceil(log2(nbins))
  int pix_bits;          // ceil(log2(tw * th))
};
constexpr int kTileMaxBins = 2048;
constexpr int kTileMaxPx = 2048;
constexpr int kTileScatterThreads = 256;
// smallest tile whose bucket count fits one digit; false: sensor too large for the tiled form
// (host-only arithmetic: inline here, so that a build without the kernels — tests/hipstub — has it too)
inline bool make_tile_geom(int W, int H, TileGeom* g) {
  // the smallest tile whose bucket count fits (a larger one was measured at C5: 64x32 takes 10 % off the
  // scatter and adds 50 % to the apply)
  static const int cand[][2] = {{32, 16}, {32, 32}, {64, 32}};
  for (const auto& c : cand) {
    const int tx = (W + c[0] - 1) / c[0], ty = (H + c[1] - 1) / c[1];
    const int nb = 2 * tx * ty + 1;
    if (nb > kTileMaxBins || c[0] * c[1] > kTileMaxPx) continue;
    g->W = W;
    g->H = H;
    g->tw = c[0];
    g->th = c[1];
    g->tiles_x = tx;
    g->tiles_y = ty;
    g->nt_cam = tx * ty;
    g->nbins = nb;
    g->bits = 1;
    while ((1 << g->bits) < nb) g->bits++;
    g->pix_bits = 1;
    while ((1 << g->pix_bits) < c[0] * c[1]) g->pix_bits++;
    return true;
  }
  return false;
}

// events per scatter block.  (Until round 6: 4096 from 2^20 events on, in 16 rounds per wave — 212 VGPRs, two resident
// blocks per CU; with one camera's buckets per table (below) the 8-round kernel's 33 KiB and 128 VGPRs let three run,
// and at 6.7 M events 2048 measured 59-66 us against 70 for 4096, profiles/r06_scatter_grid_and_nt_store_sweep.txt.)
constexpr uint32_t kTileScatterEvents = 2048;
// The batch is [left array; right array], and every bucket belongs to one camera: a scatter block never mixes the two.
// Scatter block b < nblkL owns the left events [b*TE, (b+1)*TE), block nblkL + b the right events [b*TE, (b+1)*TE) —
// so a block's bucket table (LDS in k_tile_scatter, a row of the count matrices) has one camera's nt_cam buckets + the
// out-of-sensor bin: half the columns the whole batch has (round 6; before, blocks were cut from the concatenated
// stream and every table had both cameras' buckets).  k_tile_hist block `seg` counts the buckets of `group`
// consecutive scatter blocks of ONE camera, so that the count matrices stay small: at most kTileMaxGroups groups.
constexpr uint32_t kTileMaxGroups = 512;
struct TileSplit {
  uint32_t te;            // events per scatter block
  uint32_t nblkL, nblkR;  // scatter blocks per camera
  uint32_t group;         // scatter blocks per k_tile_hist block
  uint32_t nsegL, nsegR;  // k_tile_hist blocks (= groups) per camera
  __host__ __device__ uint32_t nblk() const { return nblkL + nblkR; }
  __host__ __device__ uint32_t nseg() const { return nsegL + nsegR; }
};
inline TileSplit tile_split(uint32_t nL, uint32_t nR) {
  TileSplit t;
  t.te = kTileScatterEvents;
  t.nblkL = (nL + t.te - 1) / t.te;
  t.nblkR = (nR + t.te - 1) / t.te;
  t.group = (t.nblkL + t.nblkR + kTileMaxGroups - 3) / (kTileMaxGroups - 2);  // (each camera's last group may be short)
  if (!t.group) t.group = 1;
  t.nsegL = (t.nblkL + t.group - 1) / t.group;
  t.nsegR = (t.nblkR + t.group - 1) / t.group;
  return t;
}
// scratch (uint32 words).  Every k_tile_hist block leaves the range of seconds and the OR of the nsec words
// of its events in its own slot of `ranges` (three same-address global atomics per block — 410 blocks
// ending together — were 6 of the kernel's 32 us at 6.7 M events); k_tile_scan reduces the slots and
// writes the record format of the partition into `meta`
enum { kTileMetaCompact = 0, kTileMetaSecBase, kTileMetaWords = 8 };
constexpr int kTileRecSecBits = 20;
struct TileScratch {
  uint32_t* meta;      // [kTileMetaWords], written by k_tile_scan
  uint32_t* ranges;    // [kTileMaxGroups][4] {sec min, sec max, nsec OR, -} per k_tile_hist block
  uint32_t* totals;    // [nbins] events per bucket
  uint32_t* tile_off;  // [nbins + 1] exclusive bucket offsets into `part`, written by k_tile_scatter
  uint32_t* tile_order;  // [nbins - 1] buckets by descending size class, written by k_tile_scatter
  // the count matrices: one row per scatter block / group, one column per bucket of the row's camera (nt_cam + 1: the
  // last one is the out-of-sensor bin)
  uint32_t* P;         // [nblk][nt_cam + 1] bucket counts of the earlier scatter blocks of the same group
  uint32_t* T;         // [ngroups][nt_cam + 1] bucket counts per group
  uint32_t* C;         // [ngroups][nt_cam + 1] ... of all earlier groups of the camera (out-of-sensor bin: of all earlier groups)
};
// The layout of the scratch (d_tile), in words, for a partition buffer of part_cap events: the only place that
// computes an offset into it (host-only arithmetic, inline like make_tile_geom).  `meta` sits in the 32 spare words
// behind tile_order.
constexpr size_t kTileOffTotals = 0, kTileOffTileOff = kTileMaxBins, kTileOffOrder = 2 * (size_t)kTileMaxBins + 32,
                 kTileOffMeta = 3 * (size_t)kTileMaxBins + 32, kTileOffRanges = 3 * (size_t)kTileMaxBins + 64,
                 kTileOffP = kTileOffRanges + 4 * (size_t)kTileMaxGroups;
static_assert(kTileOffTotals == 0 && kTileOffTileOff == 2048 && kTileOffOrder == 4128 && kTileOffMeta == 6176 &&
                  kTileOffRanges == 6208 && kTileOffP == 8256,
              "tile scratch layout moved");
static_assert(kTileOffMeta + kTileMetaWords <= kTileOffRanges, "meta leaves the spare words behind tile_order");
// rows of P: 2048 events per scatter block at least; each camera's last block may be short
inline size_t tile_scratch_blocks(size_t part_cap) { return (part_cap + 2047) / 2048 + 2; }
inline size_t tile_scratch_words(size_t part_cap) {
  return kTileOffP + (tile_scratch_blocks(part_cap) + 2 * (size_t)kTileMaxGroups) * kTileMaxBins;
}
inline TileScratch tile_scratch(uint32_t* base, size_t part_cap) {
  TileScratch sc;
  sc.meta = base + kTileOffMeta;
  sc.ranges = base + kTileOffRanges;
  sc.totals = base + kTileOffTotals;
  sc.tile_off = base + kTileOffTileOff;
  sc.tile_order = base + kTileOffOrder;
  sc.P = base + kTileOffP;
  sc.T = sc.P + tile_scratch_blocks(part_cap) * kTileMaxBins;
  sc.C = sc.T + (size_t)kTileMaxGroups * kTileMaxBins;
  return sc;
}
// k_tile_hist: P, T and the blocks' ranges; launch_tile_scan: C, totals, the record format; out-of-sensor
// events added to *n_rejected
// mc (optional, enabled): the motion-compensated overload — buckets by the warped pixel, which is kept
// in warp_xy[nL + nR] for launch_tile_scatter
void launch_tile_hist(hipStream_t s, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
                      const TileGeom& g, const TileScratch& sc, unsigned long long* n_rejected,
                      const struct McParams* mc = nullptr, uint32_t* warp_xy = nullptr);
void launch_tile_scan(hipStream_t s, uint32_t nL, uint32_t nR, const TileGeom& g, const TileScratch& sc,
                      unsigned long long* n_rejected);
// stable partition of [left; right] into `part` by bucket (warp_xy non-null: the records get the
// warped pixels launch_tile_hist computed)
void launch_tile_scatter(hipStream_t s, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR,
                         const TileGeom& g, const TileScratch& sc, EventRec* part, const uint32_t* warp_xy = nullptr);
// createSAE_left/right (event_detector.cc:149-166, :212-228) per bucket, events in stream order.
// arc_touched (optional): ArcArgs::touched of the Arc* pass this batch will get — the left camera's
// touched (pixel, polarity) flags are written here, from the tiles' own bookkeeping, instead of by
// launch_arc_mark
void launch_tile_apply(hipStream_t s, const EventRec* part, uint32_t n, const TileGeom& g, const TileScratch& sc,
                       double2* L2, double2* S2, double filter_threshold, uint8_t* arc_touched, int* err,
                       uint32_t spin_limit = kSpinTicket);

// ---- time-slice composition (one stream cut into N slices, one per GPU) -------------------
constexpr double kSliceNone = -1.0;  // "this slice wrote nothing here" (event times are >= 0)
void launch_fill_f64(hipStream_t s, double* p, size_t n, double v);
void launch_spin(hipStream_t s, unsigned long long ticks);  // (100 MHz ticks)
void launch_set_u32(hipStream_t s, uint32_t* p, uint32_t v);  // *p = v, visible device-wide, behind everything enqueued on s so far
// dst[i] = src[i] unless src[i] == none
void launch_overlay_f64(hipStream_t s, double* dst, const double* src, size_t n, double none);

// ---- time surface -----------------------------------------------------------------------
// renders ncam cameras (S2 + cam*P) into level-0 interiors of dst[cam]
KernelId launch_time_surface(hipStream_t s, const double2* S2, int W, int H, double t_sync,
                         double decay_sec, int ignore_polarity, uint8_t* dst0, uint8_t* dst1,
                         int dst_stride, int ncam);

// ---- cv::medianBlur(ksize = 2k+1) of the rendered time surface (event_detector.cc:262-264) ----
// src/dst: pixel (0,0) pointers of nimg images with the given strides; BORDER_REPLICATE; k <= 7
constexpr int kMaxMedianK = 7;
void launch_median(hipStream_t s, const uint8_t* src0, const uint8_t* src1, int src_stride,
                   uint8_t* dst0, uint8_t* dst1, int dst_stride, int W, int H, int k, int nimg);

// ---- CLAHE + normalize (equalize: 1) ---------------------------------------------------------
// stage 0: per-tile LUTs, stage 1: LUT blending + min/max, stage 2: MINMAX normalisation in place
void launch_norm_pyr(hipStream_t s, const uint8_t* src0, const uint8_t* src1, int src_stride, const int* minmax,
                     const PyrDesc* p);
void launch_clahe(hipStream_t s, const uint8_t* raw0, const uint8_t* raw1, int raw_stride,
                  uint8_t* dst0, uint8_t* dst1, int dst_stride, int W, int H, uint8_t* lut,
                  int* minmax, int nimg, int stage);

// ---- pyramid ----------------------------------------------------------------------------
void launch_pyr_down(hipStream_t s, const PyrDesc* p, int nimg, int src_level);
// levels 1..3 of nimg images whose level 0 is in place, one launch (maxLevel 3)
void launch_pyr3(hipStream_t s, const PyrDesc* p, int nimg);
void launch_pyr_pad(hipStream_t s, const PyrDesc* p, int nimg);
void launch_pad_scharr(hipStream_t s, const PyrDesc* p, int nimg);  // k_pyr_pad + k_scharr, one launch
void launch_scharr(hipStream_t s, const PyrDesc* p, int nimg);

// ---- LK ---------------------------------------------------------------------------------
struct LkArgs {
  PyrDesc P;  // prev pyramid (+ derivatives)
  PyrDesc N;  // next pyramid (images only)
  const float2* prev_pts;
  const float2* init_pts;  // initial nextPts when flags has USE_INITIAL_FLOW (may alias next_pts)
  float2* next_pts;        // out
  uint8_t* status;
  const int* n_ptr;  // device count (may be NULL -> n_max)
  int n_max;
  // optional: points with index >= poll_from are not in prev_pts yet; their wave waits (bounded)
  // for k_select to publish them (SelectArgs::pub_*) or to announce a total below their index
  const unsigned long long* poll_slots = nullptr;
  const unsigned long long* poll_done = nullptr;
  uint32_t poll_seq = 0;
  int poll_from = 0;
  int* poll_err = nullptr;  // set to 1 if a wait expired (host-visible)
  // optional: two temporal launches chained point by point (frames g and g+1 when g publishes
  // nothing, so g+1 tracks exactly g's forward results).  The producer (chain_out) publishes each
  // point's forward result the moment it has it — two self-validating words per point,
  // (chain_seq << 2 | alive) << 32 | float bits of x resp. y; the consumer's wave of the same index
  // (chain_in) waits (bounded, poll_err) for them instead of reading prev_pts, and leaves
  // status 0 for a point whose forward status was 0 or that does not exist.
  unsigned long long* chain_out = nullptr;
  const unsigned long long* chain_in = nullptr;
  uint32_t chain_seq = 0;  // 30 bits, never 0
  unsigned long long poll_ticks = kTicksPoll, chain_ticks = kTicksChain;  // bounds of the two waits
  // gate: the kernel's waves go on only when *gate_ptr has reached gate_val (serial-number compare) — the `next`
  // pyramid of a chained launch is built by a prefetch sequence another thread is still issuing, so a stream wait
  // on that sequence's event cannot be enqueued yet; the sequence's last launch writes the word (launch_set_u32).
  // Bounded by chain_ticks, failure in *poll_err like the other waits.
  const uint32_t* gate_ptr = nullptr;
  uint32_t gate_val = 0;
  int max_level;
  int max_count;
  double eps2;
  int flags;
  int accum = 1;  // 1: exact integer sums (k_lk); 2: float sums in the reference build's order (k_lk_f32)
};
// one launch runs call `f`; if `b` != NULL the same wave then runs call `b` with prevPts = f's
// result and initial flow = f's prevPts (the forward/backward check of feature_tracker.cpp:410-418
// and :490-495); b->prev_pts/init_pts/next_pts/status are ignored.
void launch_lk(hipStream_t s, const LkArgs& f, const LkArgs* b, float2* back_pts,
               uint8_t* back_status);

// ---- Arc* + selection -------------------------------------------------------------------
struct ArcArgs {
  const EventRec* ev;
  uint32_t n;
  const double2* L2;  // left planes
  const double2* S2;
  int W, H;
  double filter_threshold;
  int border;                  // MIN_DIST + 1
  const uint8_t* ts;           // left level-0 padded image origin, or NULL (skip TS test)
  int ts_stride;
  double ts_lk_threshold;
  const uint32_t* mask_bits;   // H * wpr words, bit set = blocked; or NULL
  int wpr;
  uint8_t* flags;              // [n] or NULL
  uint32_t* cand_xy;           // [nblk*kArcBlock] per-block ordered candidates (x | y<<16), or NULL
  uint32_t* cand_idx;          // [nblk*kArcBlock]
  uint32_t* cand_cnt;          // [nblk]
  // per-pixel earliest candidate of this launch (optional): every candidate does
  // atomicMin(first_map[pixel], first_key | event index); keys of later launches are smaller
  // (first_key's top byte counts down), so the map is only cleared when that byte wraps
  uint32_t* first_map;
  uint32_t first_key;
  // touched: one flag byte per (pixel, polarity), index 2*pixel + polarity (arc_flag_bytes()), set by
  //          launch_arc_mark for every pair the batch has an event of, consumed (and cleared) by
  //          launch_arc_map; must start out zeroed
  // cmap:    bitmap, bit 2*pixel + polarity (arc_bitmap_words() words): result of the
  //          event-independent part of isCorner for the touched pairs, written by launch_arc_map
  //          from the planes as they are, read by launch_arc
  uint8_t* touched;
  uint32_t* cmap;
};
inline size_t arc_bitmap_words(int W, int H) { return ((size_t)2 * W * H + 31) / 32 + 64; }
inline size_t arc_flag_bytes(int W, int H) { return (size_t)2 * W * H + 1024; }
void launch_stage_pull(hipStream_t s, const void* pinned_src, void* dst, size_t bytes);
// ... of chunks of `epc` events each, packed to 8 bytes per event or raw as desc[chunk] = {base second, packed?} says
void launch_stage_pull_packed(hipStream_t s, const void* pinned_src, void* dst, size_t bytes, const void* desc, uint32_t epc);  // H2D of staged events by a kernel
void launch_arc_mark(hipStream_t s, const ArcArgs& a);  // per event: which (pixel, polarity) pairs occur
void launch_arc_map(hipStream_t s, const ArcArgs& a);   // per touched pair (rings, L[!p] > L[p], TS, border)
void launch_arc(hipStream_t s, const ArcArgs& a);       // per event, in stream order (needs the map)

// Only the earliest candidate of a pixel can ever be accepted by the greedy selection
// (feature_tracker.cpp:13-38: if it is accepted its disc blocks the pixel, if it is refused the
// pixel was blocked already, and blocked pixels stay blocked), so the later ones (more than half
// of the Arc* corners of a 5 Mev/s stream) are dropped from the per-block lists, in place and in
// order, before the ordered compaction; the sequential stage then has less than half the work.
void launch_dedup(hipStream_t s, uint32_t* cand_xy, uint32_t* cand_idx, uint32_t* cand_cnt,
                  uint32_t nblk, const uint32_t* first_map, uint32_t first_key, int W);

// ordered compaction of the per-block candidate lists (parallel; one block per Arc* block)
// grp_scratch (optional, [nblk / 64 + 1]): with more than 2048 blocks the counts are summed per 64
// blocks first (k_compact_groups)
void launch_compact(hipStream_t s, const uint32_t* cand_xy, const uint32_t* cand_idx,
                    const uint32_t* cand_cnt, uint32_t nblk, uint32_t* comp_xy, uint32_t* comp_idx,
                    uint32_t* total, uint32_t* grp_scratch = nullptr);

// ---- goodFeaturesToTrack (image front-end) ----------------------------------
// cv::goodFeaturesToTrack(img, n, quality, minDistance, mask) with blockSize 3 / gradientSize 3 /
// Shi-Tomasi, as FeatureTracker::trackImage calls it (feature_tracker.cpp:228) [OpenCV, restated]:
//   k_gftt_cov      Sobel (float, scale 1/3060) -> (Dx*Dx, Dx*Dy, Dy*Dy) per pixel
//   k_gftt_rowsum   box filter rows: (c[x-1] + c[x]) + c[x+1]
//   k_gftt_eig      box filter columns as OpenCV's running sum (one thread per column, rows in
//                   order: float addition order matters), min eigenvalue, masked maximum
//   k_gftt_collect  threshold at quality*max, 3x3 local maximum, mask -> per-block ordered lists
//   (k_compact), k_gftt_sortprep + 4 x k_radix_pass: by value then address, both descending
//   k_select with the open Euclidean disc: the minDistance greedy
struct GfttArgs {
  const uint8_t* img;  // level-0 pixel (0,0) inside its reflect-101 padded buffer
  int stride;
  int W, H;
  float4* cov;         // [W*H] scratch
  float4* rowsum;      // [W*H] scratch
  float* eig;          // [W*H] cornerMinEigenVal
  const uint32_t* mask_bits;  // blocked pixels (1 = not allowed), may be NULL
  int wpr;
  uint32_t* max_key;   // [1] order-preserving key of the masked maximum (cleared by k_gftt_cov)
  double quality;
  uint32_t* cand_xy;   // [nblk*kArcBlock] per-block ordered candidates: x | y<<16 ...
  uint32_t* cand_val;  // ... and the response bits
  uint32_t* cand_cnt;  // [nblk]
};
void launch_gftt_response(hipStream_t s, const GfttArgs& a);  // cov, rowsum, eig
void launch_gftt_collect(hipStream_t s, const GfttArgs& a);
// keys = ~value bits, vals = xy, read back to front (so that the stable sort leaves equal values
// in descending address order); accumulates the 4 x 8-bit digit histograms, clears the look-back
void launch_gftt_sortprep(hipStream_t s, const uint32_t* comp_xy, const uint32_t* comp_val, uint32_t n,
                          uint32_t* keys, uint32_t* vals, uint32_t* ghist, uint32_t* lookback,
                          uint32_t lookback_words);

// ---- FAST-9/10 on an 8-bit image (the time surface) -----------------------------------------
// fast::fast_corner_detect_9 / _10, fast_corner_score_10 and fast_nonmax_3x3 of the reference's vendored
// library (dependences/fast_neon-master/include/fast/fast.h:22-47), as closed forms:
//   ring p[0..15]: the radius-3 Bresenham circle from (0,3) through (3,0), (0,-3), (-3,0); c the centre
//   score_N = max over the 16 starts s of max(min_{k<N}(p[s+k] - c), min_{k<N}(c - p[s+k])) - 1
//   corner  <=> 3 <= x < W-3, 3 <= y < H-3 and score_N >= barrier; the list is in raster order
//   nonmax  keeps a corner iff none of its 8 neighbours is a corner with a score >= its own
// Integer-only: the results are exact, and pinned to vectors the reference's compiled code produced
// (tests/golden/fast_ref_*.npz).
//   k_fast_score<N>  byte map m = score_N + 1 where the pixel is a corner at `barrier`, else 0
//   k_fast_collect   (3x3 non-max on m) -> per-block ordered lists (x | y<<16, score); block b owns pixels
//                    [b*kArcBlock, (b+1)*kArcBlock) in row-major order, so k_compact's concatenation in
//                    block order is raster order; no atomics: k_fast_sum adds up the per-block counts before non-max
struct FastArgs {
  const uint8_t* img;   // pixel (0,0); rows `stride` bytes apart (a pyramid's padded level 0, or stride = W)
  int stride;
  int W, H;
  int arc;              // 9 or 10
  int barrier;          // 0..255
  int nonmax;
  uint8_t* m;           // [W*H]
  uint32_t* cand_xy;    // [nblk*kArcBlock]
  uint32_t* cand_score; // [nblk*kArcBlock]
  uint32_t* cand_cnt;   // [nblk]
  uint32_t* det_cnt;    // [nblk] corners before non-max
  uint32_t* n_detected; // [1] their sum (k_fast_sum), or NULL: not wanted
  // >= 0 (the candidate pass of ESVIO_FE_DETECT_FAST, nonmax only): a survivor of the non-max whose centre byte has
  // this value is left out of the lists (the TS_LK_threshold test of feature_tracker.cpp:26); det_cnt / n_detected
  // then count the survivors, the left-out ones included, instead of the corners before non-max.  -1: nobody is
  int skip_center;
};
void launch_fast_score(hipStream_t s, const FastArgs& a);
void launch_fast_collect(hipStream_t s, const FastArgs& a);
// The FAST candidate pass orders its corners by score, descending, equal scores in raster order: k_compact's raster-
// ordered list of *total (xy, score) entries -> the pairs of ONE stable 8-bit radix pass.  Scores are 0..254, so
// keys[i] = (254 - score) | score << 8 (the pass looks at the low byte, the score rides along), vals[i] = xy; the
// low bytes' histogram is added to ghist[256] (zeroed by the caller) and the look-back words of the tiles that pass
// will use are cleared.  *total is read on the device: the launch is sized for n_max.
void launch_fast_keys(hipStream_t s, const uint32_t* comp_xy, const uint32_t* comp_score, const uint32_t* total,
                      uint32_t n_max, uint32_t* keys, uint32_t* vals, uint32_t* ghist, uint32_t* lookback);

// ---- caller-layout event arrays -> event records (esvio_fe_convert_events) -------------------
// Where the four fields of event i lie: base + i * stride, any alignment (esvio_fe_event_fields with the pointers
// the DEVICE reads: device memory, or the device-side address of page-locked host memory).  Per event, in integers:
//   ticks = t + t_offset; bad (counted in *n_bad, record unspecified) if ticks < 0, ticks >= 2^32 * tps or a
//   64-bit t outside +-2^62;  sec = ticks / tps, nsec = (ticks % tps) * t_unit_ns with tps = 10^9 / t_unit_ns;
//   polarity = (signed p > 0);  x, y copied;  the record's padding bytes zero.
// k_events_from_fields: four consecutive events per lane.  A field whose four values lie side by side and aligned
// is read with one load (8 B of x or y, 16 / 2 x 16 B of t, 4 B of p); four fields that share aligned 16-byte
// records are read as those records; anything else element by element, byte by byte where the element itself is
// unaligned.  One 16-byte store per event.
struct FieldsArgs {
  const uint8_t *x, *y, *t, *p;
  int32_t x_stride, y_stride, t_stride, p_stride;
  int32_t t_bits;     // 32 (unsigned) or 64 (signed)
  int32_t t_unit_ns;  // 1 or 1000
  int32_t p_bits;     // 8 or 16 (signed)
  int64_t t_offset;
};
void launch_events_from_fields(hipStream_t s, const FieldsArgs& a, size_t n, EventRec* dst, unsigned long long* n_bad);

// ---- background-activity + refractory filter of an event batch (esvio_fe_filter_events, esvio_fe_filter_batch) ----
// include/esvio_fe.h holds the rule.  The chain: launch_sae_keys (keys = y*W + x, out-of-sensor events = P: they sort
// last; values = event index) -> launch_radix_pass x passes -> heads -> filter -> count -> scan -> emit, all on one
// stream, each launch reading what the launches before it wrote; no launch of these five waits on the device.
// On field arrays (esvio_fe_filter_batch with esvio_fe_event_fields) three launches differ: launch_baf_keys_fields
// in launch_sae_keys' place, the heads launch with BafArgs::tstream set, launch_baf_emit_fields in launch_baf_emit's.
// With an address stage set (esvio_fe_set_address_filter: step 1a of the rule) the record form launches
// launch_baf_keys_addr in launch_sae_keys' place and the fields form's keys kernel takes the stage too: an event the
// stage rejects gets key P, as an out-of-sensor one — it sorts last and nothing behind the keys looks at it.  The emits
// take the flatten value.  on == 0: no stage; the chain is then the launches it was without one.
struct AddrArgs {
  uint32_t x0, y0, x1, y1;  // the ROI, inclusive
  int32_t polarity;         // 0 both; 1 ON only; 2 OFF only
  int32_t on;               // != 0: a stage is set
  const uint32_t* mask;     // [(P + 31) / 32] bit (pixel & 31) of word (pixel >> 5): the pixel is silenced; NULL: no mask
};
struct BafResult {  // zeroed by the host in front of the chain; one per camera
  unsigned long long n_rejected;  // k_sae_keys / k_baf_keys_addr / k_baf_keys_fields
  uint32_t n_kept;                // k_baf_scan
  int err;                        // k_radix_pass: a look-back wait expired
  EventRec last;                  // k_baf_emit(_fields): the last kept record (untouched if none)
  unsigned long long n_bad;       // k_baf_keys_fields: BAD events by conversion's test; != 0: k_baf_count leaves B alone
  unsigned long long reserved;
};
static_assert(sizeof(BafResult) == 48 && offsetof(BafResult, last) == 16, "BafResult layout");
constexpr uint32_t kBafBlock = 1024;  // events per block of the ordered compaction (four flags per lane)
// lanes of k_baf_scan's one workgroup: each owns ceil(blocks / lanes) consecutive blocks' counts (esvio_fe_scan_lanes)
constexpr int kBafScanThreads = 1024;
inline uint32_t baf_blocks(uint32_t n) { return (n + kBafBlock - 1) / kBafBlock; }
struct BafArgs {
  const EventRec* ev;    // [n] the call's events, device memory (the fields form: not read)
  const long long* tstream;  // the fields form: [n] stamps (ns) in stream order; NULL: the stamps are read from ev
  uint32_t n;
  uint32_t P;            // W * H, also the key of an out-of-sensor event
  int W, H;
  const uint32_t* keys;  // [n] sorted ...
  const uint32_t* vals;  // ... with their event indices (ascending inside a key: the sort is stable)
  uint32_t* head;        // [P] position of a pixel's first pair; stale entries are recognised, never cleared
  long long* tsort;      // [n] stamps (ns) in sorted order
  long long* B;          // [P] the camera's plane: -1 = none, else the stamp in ns
  long long window_ns;
  int min_support;       // 0: no support test
  long long refractory_ns;  // 0: no refractory test
  uint8_t* flags;        // [n rounded up to 4] keep_i, by event index
  uint32_t* blk_cnt;     // [baf_blocks(n) + 1] kept per block, then their exclusive offsets and the total
  EventRec* dst;         // [n] the kept records in stream order; must not overlap ev
  BafResult* res;
  uint32_t* sort_scratch;  // the sort's ghist + tickets, cleared by launch_baf_filter (sort_head_words words)
  uint32_t sort_head_words;
  int flatten;           // the address stage's: 0 no; 1 / 2: a kept record's polarity byte becomes 1 / 0
};
void launch_baf_heads(hipStream_t s, const BafArgs& a);
void launch_baf_filter(hipStream_t s, const BafArgs& a);
void launch_baf_count(hipStream_t s, const BafArgs& a);   // + the plane update
void launch_baf_scan(hipStream_t s, const BafArgs& a);
void launch_baf_emit(hipStream_t s, const BafArgs& a);
// the fields form: per event of `fields` (FieldsArgs, above: pointers the device reads) the key, the index, the
// stream-order stamp, the digit histograms and the cleared look-back words as launch_sae_keys; res->n_rejected and
// res->n_bad are added to
void launch_baf_keys_fields(hipStream_t s, const FieldsArgs& fields, uint32_t n, int W, int H, uint32_t* keys, uint32_t* vals,
                            long long* tstream, BafResult* res, int passes, int bits, uint32_t* ghist, uint32_t* lookback,
                            uint32_t lookback_words, const AddrArgs& addr);
void launch_baf_emit_fields(hipStream_t s, const BafArgs& a, const FieldsArgs& fields);
// the record form with an address stage: launch_sae_keys' keys, indices, digit histograms and look-back clearing for
// one camera's n records; key P for an out-of-sensor or address-rejected event, both counted in res->n_rejected
void launch_baf_keys_addr(hipStream_t s, const EventRec* ev, uint32_t n, int W, int H, uint32_t* keys, uint32_t* vals,
                          BafResult* res, int passes, int bits, uint32_t* ghist, uint32_t* lookback, uint32_t lookback_words,
                          const AddrArgs& addr);

// ---- hot-pixel learning (esvio_fe_hot_learn, esvio_fe_hot_select) ----------------------------------------------------
// include/esvio_fe.h holds the rule.  Learn: one launch; C[pixel] += 1 per in-sensor event, equal pixels combined
// inside a wave (one add of the group's size per distinct pixel), per wave one add to n and one 64-bit max each to
// tmax and to ~tmin.  Select: keys of the count plane (0xFFFFFFFF - C for C >= T, else 0xFFFFFFFF; value = pixel) ->
// launch_radix_pass x 4 over 8 bits (stable: equal counts stay in pixel order) -> pick (one workgroup: the list, the
// counts, the result block and, installing, the mask words).  No launch of these waits on the device for another
// workgroup but the radix pass's bounded look-back.
struct HotState {  // per camera; all zero = nothing learned
  unsigned long long n;         // events counted
  unsigned long long not_tmin;  // ~t_min (so that the empty state is zero and the update is a max)
  unsigned long long tmax;
  unsigned long long n_bad;     // the running call's BAD events (zeroed by the host in front of the launch)
};
struct HotResult {  // zeroed by the host in front of a selection
  uint32_t above, selected;
  int err;          // k_radix_pass: a look-back wait expired
  int installed;
};
constexpr uint32_t kHotMaxPixels = 4096;
void launch_hot_count(hipStream_t s, const EventRec* ev, uint32_t n, int W, int H, uint32_t* C, HotState* st);
void launch_hot_count_fields(hipStream_t s, const FieldsArgs& fields, uint32_t n, int W, int H, uint32_t* C, HotState* st);
// keys / values of the P pixels, their four digit histograms added to ghist[4 << 8] (zeroed by the caller, as the
// look-back words are), res->above
void launch_hot_keys(hipStream_t s, const uint32_t* C, uint32_t P, uint32_t threshold, uint32_t* keys, uint32_t* vals,
                     uint32_t* ghist, HotResult* res);
// the first min(res->above, max_pixels) sorted pairs -> xy[2j], xy[2j+1], counts[j]; res->selected; with mask != NULL
// and selected <= cap: the mask_words words cleared and the selection's bits set (res->installed = 1)
void launch_hot_pick(hipStream_t s, const uint32_t* keys, const uint32_t* vals, int W, uint32_t P, uint32_t max_pixels,
                     uint32_t cap, uint16_t* xy, uint32_t* counts, uint32_t* mask, uint32_t mask_words, HotResult* res);

// ---- raw sensor streams: Prophesee EVT3 / EVT2 words -> event records (esvio_fe_decode_raw, esvio_fe_track_raw) ----
// include/esvio_fe.h holds the rule.  Everything a word needs from the words before it is a "last writer before me"
// or a prefix sum, so a run of words is summarised by a TRANSFORMER of the decoder state (RawXf) and transformers
// compose associatively (raw_combine: earlier, later).  The chain: reduce (one transformer per tile of kRawTileBytes
// bytes) -> scan (one workgroup per camera: the tiles' exclusive prefixes, seeded with the camera's carried state; the
// totals and the state after the call) -> emit (re-reads the tile, scans inside it from the tile's carry-in, builds the
// records at offset + rank).  Three launches for one camera or for both: both cameras' tiles share each grid.  No
// launch waits on the device for another workgroup.  EVT2 is the same chain with a smaller classifier; EVT2.1 is EVT2's
// with 64-bit words — two per lane — whose event count is the popcount of the word's 32-bit mask (a lane can stand for
// 64 records, a tile for 16 384).
// Triggers (esvio_fe_decode_triggers): the same chain with a classifier of its own — k_trig_reduce, k_raw_scan as it is,
// k_trig_emit — over the same RawXf: only the time base and the counts are used, a trigger word counts as one "event",
// and the records stored are esvio_fe_trigger's 16 bytes.
constexpr uint32_t kRawTileBytes = 4096;  // 256 lanes x 16 bytes: 2048 EVT3 words, 1024 EVT2 words, 512 EVT2.1 words
// lanes of k_raw_scan's workgroup (one per camera): each owns ceil(tiles / lanes) consecutive tiles' transformers
constexpr uint32_t kRawScanLanes = 256;
constexpr int kRawEvt2 = 2, kRawEvt3 = 3, kRawEvt21 = 21;
constexpr uint32_t kRawHasTh = 1u, kRawHasTl = 2u, kRawHasY = 4u, kRawHasBx = 8u, kRawBp = 16u;
constexpr int kRawTlShift = 8, kRawYShift = 20;  // flags: tl in bits 8..19, y in bits 20..30
struct RawXf {
  uint32_t th_first, th_last;  // kRawHasTh: the first and the last TIME_HIGH value of the run ...
  uint32_t wraps;              // ... and the wraps between its TIME_HIGH words
  uint32_t flags;              // which fields the run sets (kRawHas*), and bp, tl, y as it leaves them
  uint32_t bx;                 // kRawHasBx: bx as the run leaves it; else the sum of its increments (mod 2^16)
  uint32_t before;             // events in front of the run's first TIME_HIGH (all of them if it has none): emitted if
                               // the state in front of the run has seen a TIME_HIGH, else untimed
  uint32_t after;              // events behind it: emitted
  uint32_t other;
};
static_assert(sizeof(RawXf) == 32, "RawXf layout");
struct RawResult {  // written by k_raw_scan (bad: cleared there, added to by k_raw_emit); one per camera
  uint32_t events, untimed, other, wraps;  // wraps: inside this call
  RawXf state;                             // the carried state composed with the whole call: the state after it
  unsigned long long bad;
  long long first_t, last_t;               // ticks of the first / last emitted event (k_raw_emit; untouched if none)
};
static_assert(sizeof(RawResult) == 72, "RawResult layout");
struct RawCam {
  const uint8_t* words;   // the device reads them here, at any alignment (16-byte aligned: one load per lane)
  uint32_t n_bytes;       // a multiple of the word size
  uint32_t tiles;         // ceil(n_bytes / kRawTileBytes); 0: the camera takes no part
  RawXf seed;             // the carried state as a transformer (wraps 0, counts 0)
  unsigned long long wraps_base;  // the carried wrap count
  long long t_offset;     // microseconds
  RawXf* sums;            // [tiles] reduce: the tiles' transformers; scan: their exclusive prefixes, seed included
  EventRec* dst;          // [dst_cap]; nothing is stored when the call's events exceed dst_cap
  uint32_t dst_cap;
  RawResult* res;
};
struct RawArgs {
  int format;     // kRawEvt2 / kRawEvt3 / kRawEvt21
  RawCam cam[2];  // the grid's blocks: cam[0].tiles, then cam[1].tiles
};
void launch_raw_reduce(hipStream_t s, const RawArgs& a);
void launch_raw_scan(hipStream_t s, const RawArgs& a);
void launch_raw_emit(hipStream_t s, const RawArgs& a);
// the trigger chain's own two launches (RawCam::dst: [dst_cap] 16-byte esvio_fe_trigger records; RawResult::events,
// untimed, bad, first_t, last_t count triggers; `other` stays 0)
void launch_trig_reduce(hipStream_t s, const RawArgs& a);
void launch_trig_emit(hipStream_t s, const RawArgs& a);

// ---- libcaer / AEDAT 3.1 polarity records -> event records (esvio_fe_decode_aedat, esvio_fe_track_aedat) ----
// include/esvio_fe.h holds the rule.  The host has walked the packet chain (fe_aedat.h): what arrives here is the chunk's
// polarity records packed into one array and the table of its runs of equal eventTSOverflow.  A record needs nothing
// from the records before it but its rank among the kept ones, so the chain is count (kept records per tile of
// kAedatTile) -> scan (one workgroup per camera: the tiles' exclusive prefixes, the totals) -> emit (one record per
// lane: its run by a binary search of the table, the stamp, one 16-byte store at dst[rank]).  With keep_invalid the
// rank is the index: the host writes the result block's counts itself and launches the emit alone.  Both cameras'
// tiles share each grid, as in the raw chain; no launch waits on the device for another workgroup.
// The timer slots of these kernels are a range of their own behind K_COUNT (esvio_fe_ingest_kernel_count()): the stage
// table, whose end a test pins, stays as it is.
enum IngestKernelId { K_AEDAT_COUNT = K_COUNT, K_AEDAT_SCAN, K_AEDAT_EMIT, K_BAG_EMIT, K_IMAGE_EMIT, K_INGEST_COUNT };
constexpr uint32_t kAedatTile = 1024;  // records per workgroup: 1024 lanes, one record each
constexpr uint32_t kAedatScanLanes = 256;  // lanes of k_aedat_scan's workgroup: each owns ceil(tiles / lanes) consecutive tiles' counts
struct AedatRun {                      // (fe_aedat.h: esvio::aedat::Run)
  uint32_t first;
  int32_t overflow;
};
struct AedatResult {  // events, invalid: k_aedat_scan (keep_invalid: the host); bad, first_t, last_t: k_aedat_emit
  uint32_t events, invalid;
  unsigned long long bad;
  unsigned long long first_t, last_t;  // ticks_ns of the first / last emitted event (untouched if none)
};
static_assert(sizeof(AedatResult) == 32, "AedatResult layout");
struct AedatCam {
  const uint2* rec;      // [n] the packed polarity records, device memory
  uint32_t n;
  uint32_t tiles;        // ceil(n / kAedatTile); 0: the camera takes no part
  const AedatRun* runs;  // [n_runs] ascending in `first`, runs[0].first == 0
  uint32_t n_runs;
  uint32_t keep_invalid;
  long long t_offset;    // nanoseconds
  uint32_t* sums;        // [tiles] count: the tiles' kept records; scan: their exclusive prefixes
  EventRec* dst;         // [dst_cap]; nothing is stored when the kept records exceed dst_cap
  uint32_t dst_cap;
  AedatResult* res;
};
struct AedatArgs {
  AedatCam cam[2];  // the grid's blocks: cam[0].tiles, then cam[1].tiles
};
void launch_aedat_count(hipStream_t s, const AedatArgs& a);
void launch_aedat_scan(hipStream_t s, const AedatArgs& a);
void launch_aedat_emit(hipStream_t s, const AedatArgs& a);

// ---- rosbag v2.0: dvs_msgs/EventArray wire events -> event records (esvio_fe_decode_bag, esvio_fe_feed_push_bag) ----
// include/esvio_fe.h holds the rule.  The host has walked the records (fe_bag.h): what arrives here is each camera's wire
// events of the chunk, 13 packed bytes each (u16 x, u16 y, u32 sec, u32 nsec, u8 polarity), from a 16-byte aligned base.
// Every wire event is emitted and the host knows the count, so one launch does it all: k_bag_emit, both cameras' tiles in
// one grid, one event per lane, 13 bytes in and one 16-byte store out; no workgroup waits for another.  A wave's 64
// events are 832 bytes = 52 dwordx4, so every wave's span is 64-byte aligned.  Each lane assembles its own 13 bytes,
// the byte assembly of k_events_from_fields' element path (KERNELS.md "ROS bags" has the measurement behind it).
// K_BAG_EMIT is appended to the ingest range (IngestKernelId above).
constexpr uint32_t kBagTile = 1024;      // events per workgroup: 1024 lanes, one event each
constexpr uint32_t kBagEventBytes = 13;
struct BagResult {  // zeroed in front of the launch; k_bag_emit: the BAD events, the first / last event's stamp
  unsigned long long bad;
  uint32_t first_sec, first_nsec, last_sec, last_nsec;
  uint32_t pad[2];
};
static_assert(sizeof(BagResult) == 32, "BagResult layout");
struct BagCam {
  const uint8_t* src;  // [13 n] the packed wire events, device memory, 16-byte aligned; readable up to the next multiple of 16
  uint32_t n;
  uint32_t tiles;      // ceil(n / kBagTile); 0: the camera takes no part
  EventRec* dst;       // [dst_cap]; nothing is stored when n exceeds dst_cap
  uint32_t dst_cap;
  BagResult* res;
};
struct BagArgs {
  BagCam cam[2];       // the grid's blocks: cam[0].tiles, then cam[1].tiles
};
void launch_bag_emit(hipStream_t s, const BagArgs& a);

// ---- text event files: "t x y p" / "x y p t" lines -> event records (esvio_fe_decode_text, esvio_fe_track_text) ----
// include/esvio_fe.h "text event files" holds the rule, fe_text.h the line classifier both sides share.  The VIRTUAL
// STREAM of a camera is its carried tail (at most 65 bytes, a by-value argument) followed by the chunk; a line belongs
// to the tile of kTextTileBytes virtual bytes in which it STARTS, and a byte starts a line when the byte in front of it
// is '\n' (virtual byte 0: unless the carried state is "inside an overlong line").  The chain is the raw decoder's:
//   k_text_count  stages the tile, one byte in front of it and a halo of one maximal line (kTextHalo) in LDS with
//                 16-byte loads, compacts the tile's line starts with ballots, one lane classifies one line out of LDS;
//                 per tile the classes' counts, the least malformed line start and the tile's last '\n'
//   k_text_place  one workgroup per camera: the tiles' exclusive event prefixes, the totals, the corrections only the
//                 whole stream can decide (the line an earlier call left overlong; an overlong line no '\n' follows),
//                 the state behind the call
//   k_text_emit   the same staging and the same classifier; an event line's rank among the tile's event lines by
//                 ballots, one 16-byte store at dst[prefix + rank]
// Three launches for one camera or for both: both cameras' tiles share each grid.  No workgroup waits for another.
// Their timer slots lie behind every other table (fe_ctx.h).
constexpr uint32_t kTextTileBytes = 4096;  // 256 lanes x 16 bytes
constexpr uint32_t kTextScanLanes = 256;   // lanes of k_text_place's workgroup: each owns ceil(tiles / lanes) consecutive tiles' summaries
constexpr uint32_t kTextHalo = 66;         // a body of 64 bytes, '\r', '\n'
struct TextTile {      // k_text_count per tile; k_text_place turns `events` into the exclusive prefix
  uint32_t events;     // event lines, the BAD ones among them
  uint32_t comments, blank, malformed, bad;
  uint32_t last_nl;    // the virtual position behind the tile's last '\n'; 0: it holds none
  uint32_t first_mal;  // the virtual position of the tile's first malformed line; 0xffffffff: none
  uint32_t pad;
};
static_assert(sizeof(TextTile) == 32, "TextTile layout");
struct TextCarry {  // the state between two calls (fe_text.h: State) as the kernels take and leave it
  unsigned long long tail_w[9];  // the tail's bytes, little-endian in 64-bit words (72 >= 65)
  unsigned long long skip_len;
  uint32_t len, skip;
};
static_assert(sizeof(TextCarry) == 88, "TextCarry layout");
struct TextResult {  // k_text_place; first_t .. last_nsec: k_text_emit (untouched if no event or a BAD first / last one)
  unsigned long long events, comments, blank, malformed, bad;
  long long first_malformed;  // relative to the chunk's first byte; valid if malformed
  long long first_t, last_t;  // ticks, nanoseconds
  uint32_t last_sec, last_nsec;
  TextCarry state;            // behind the call
};
static_assert(sizeof(TextResult) == 160, "TextResult layout");
struct TextCam {
  const uint8_t* bytes;  // the chunk, device-readable, any alignment
  uint32_t n_bytes;
  uint32_t tiles;        // max(1, ceil((carry.len + n_bytes) / kTextTileBytes)); 0: the camera takes no part
  TextCarry carry;       // the state in front of the call
  uint32_t end;          // ESVIO_FE_TEXT_END: an unterminated last line is a line
  uint32_t dst_cap;
  long long t_offset;    // nanoseconds
  TextTile* sums;        // [tiles]
  EventRec* dst;         // [dst_cap]; nothing is stored when the call's events exceed dst_cap
  TextResult* res;
};
struct TextArgs {
  int order, time;  // esvio::text::kTxyp / kXypt, kSecDecimal / kIntUs / kIntNs
  TextCam cam[2];   // the grid's blocks: cam[0].tiles, then cam[1].tiles
};
void launch_text_count(hipStream_t s, const TextArgs& a);
void launch_text_place(hipStream_t s, const TextArgs& a);
void launch_text_emit(hipStream_t s, const TextArgs& a);

// ---- rosbag images: sensor_msgs/Image payloads -> dense 8-bit gray (esvio_fe_decode_bag_images, esvio_fe_convert_image) ----
// include/esvio_fe.h holds the rule.  The host has walked the records (fe_bag.h): what arrives here is a table of image
// descriptors — where the payload's first row lies, its row stride, its encoding class, where the dense width x height
// gray image goes — and one launch, k_image_emit, writes all of them: grid.y is the image, a lane writes ONE ALIGNED DWORD
// of the destination, four consecutive pixels of the dense image counted from the dword boundary at or below dst (dst may
// lie at any byte: 346 x 260 images side by side do not keep 16-byte boundaries, 5 x 1 ones not even dword boundaries);
// the dwords the image's ends share with its neighbours, and groups that span two rows, go pixel by pixel.  The source
// bytes of a group are 4 or 12 consecutive bytes at ANY alignment (step may be odd): each lane assembles its own with
// ld_any (KERNELS.md "ROS bag images" has the measurement behind it).  K_IMAGE_EMIT is appended to the ingest range.
constexpr uint32_t kImageTile = 1024;  // pixels per workgroup: 256 lanes, one destination dword each
constexpr uint32_t kImageMaxSide = 8192;
struct ImageDesc {
  const uint8_t* src;  // the payload's first byte, device memory, any alignment
  uint8_t* dst;        // [width * height], device memory, any alignment
  uint32_t step;       // bytes between rows, >= width * bpp
  uint32_t cls;        // 1: the byte; 2: (B, G, R) -> gray; 3: (R, G, B) -> gray
};
static_assert(sizeof(ImageDesc) == 24, "ImageDesc layout");
struct ImageArgs {
  const ImageDesc* desc;  // [n_images] device memory
  uint32_t n_images;
  uint32_t width, height;  // of every image of the launch; width * height <= 2^26
};
void launch_image_emit(hipStream_t s, const ImageArgs& a);

// ---- AEDAT 3.1 frames: 16-bit DAVIS frame pixels -> dense 8-bit gray (esvio_fe_decode_aedat_frames, esvio_fe_convert_frame16) ----
// include/esvio_fe.h "AEDAT 3.1 frames" holds the rule.  The host has walked the packets (fe_aedat.h): what arrives here
// is a table of frame descriptors — where the frame's uint16 values lie, dense and row-major with the channels
// interleaved, how many channels, where the dense width x height gray image goes — and one launch, k_frame16_emit,
// writes all of them: grid.y is the frame, a lane writes ONE ALIGNED DWORD of the destination as k_image_emit does, and
// the dwords the image's ends share with its neighbours go pixel by pixel with byte stores.  The source is dense, so a
// group never spans a row's padding: its 8 (mono) or 24 (colour) source bytes are consecutive, at any 2-BYTE alignment —
// the scratch is 16-byte aligned, but the group's phase follows dst's, and esvio_fe_convert_frame16 takes a device
// source wherever it lies.  Each lane assembles them with ld_pair16: a dword load where the address is dword aligned,
// else two 16-bit loads (KERNELS.md "AEDAT frames").  The kernel's timer slot, K_FRAME16_EMIT, lies behind every other
// table (fe_ctx.h).
constexpr uint32_t kFrame16Tile = 1024;  // pixels per workgroup: 256 lanes, one destination dword each
struct Frame16Desc {
  const uint8_t* src;  // channels * width * height uint16 values, device memory, 2-byte aligned
  uint8_t* dst;        // [width * height], device memory, any alignment
  uint32_t channels;   // 1: value >> 8; 3: (R, G, B) = values >> 8 -> gray
  uint32_t reserved;
};
static_assert(sizeof(Frame16Desc) == 24, "Frame16Desc layout");
struct Frame16Args {
  const Frame16Desc* desc;  // [n_frames] device memory
  uint32_t n_frames;
  uint32_t width, height;  // of every frame of the launch; width * height <= 2^26
};
void launch_frame16_emit(hipStream_t s, const Frame16Args& a);

// ---- event images: detector.cur_event_mat_left/right (esvio_fe_set_event_images) ----
// include/esvio_fe.h holds the rule: per camera the LAST event of the call at every pixel decides its colour.  Two
// launches behind the SAE update of the handle's own planes, on its stream:
//   k_evimg_mark  one lane per event, both cameras in one grid: atomicMax(marks[cam][pixel], ((k + 1) << 1) | polarity),
//                 k the event's index in its camera's array (< 2^31 - 1: every entry point refuses larger batches).  The
//                 maximum does not depend on the order in which the lanes arrive, so the word ends as the pixel's last
//                 event in stream order, exactly.  For a batch of more than one event per pixel the lanes walk the stream from its end and read the word first: an
//                 event that finds a later one's key there skips its atomic (each atomic is a 64-byte request at the
//                 memory side, whose rate bounds the kernel; KERNELS.md "Event images").  The pixel: the event's own (kEvimgPixOwn), or the one the
//                 motion-compensated update writes it at — k_mc_warp's warp_xy[i] where the tiled update has filled it
//                 (kEvimgPixWarp), mc_pixel as k_sae_keys<true> computes it in the sort form (kEvimgPixMc).  An
//                 out-of-sensor event is skipped as the update skips it; the warp drops none (mc_warp keeps the event's
//                 own pixel where the warped one leaves the sensor).
//   k_evimg_emit  one lane per FOUR pixels: four marks in, three dwords of (B, G, R) bytes out, the marks it found set
//                 back to zero — so the planes are zero between calls and no call clears them.  FRESH (track calls):
//                 every pixel is written, colour or zero.  Otherwise (stage calls): only marked pixels are merged into
//                 the bytes that are there.  marks and images are padded to a multiple of four pixels (`groups` of
//                 them); the caller sees the first width*height*3 bytes, dense.
//   k_evimg_canvas  hconcat(left, right) into a scratch of the getter's (esvio_fe_get_event_canvas), one lane per pixel.
// They are booked in two timer slots of their own (esvio_fe_ctx::evimg.stats), outside the stage and the ingest tables.
enum { kEvimgPixOwn = 0, kEvimgPixWarp = 1, kEvimgPixMc = 2 };
void launch_evimg_mark(hipStream_t s, const EventRec* evL, uint32_t nL, const EventRec* evR, uint32_t nR, int W, int H,
                       uint32_t* marksL, uint32_t* marksR, int pix, const uint32_t* warp_xy, const McParams* mc);
// marks1 == nullptr: one camera (marks0 / img0)
void launch_evimg_emit(hipStream_t s, uint32_t* marks0, uint32_t* img0, uint32_t* marks1, uint32_t* img1, uint32_t groups,
                       bool fresh);
void launch_evimg_canvas(hipStream_t s, const uint8_t* left, const uint8_t* right, int W, int H, uint8_t* canvas);

// ---- stream slicing: a record stream cut into fixed-rate windows (esvio_fe_slice_events) ----
// include/esvio_fe.h holds the rule.  An event's window is m_i = max(m_{i-1}, c_i), c_i = the boundaries at or below its
// stamp: a prefix MAXIMUM, associative and commutative, so a tile of events is summarised by one number and the chain
// is the raw chain's: reduce (the tile's maximum of c) -> scan (one workgroup per camera: the tiles' exclusive prefix
// maxima behind the carried count, the totals and the state after the call) -> cuts (re-reads the tile, scans inside it
// from the tile's prefix; the lane where m rises writes the cut entries it owns).  The kernels take two cameras' tiles
// in one grid, as the raw chain's do; the entry points there are so far run ONE camera per chain (a slice call and a
// feed push are per camera): cam[1].tiles is 0 and the scan is one workgroup.  No launch waits on the device for another workgroup.  Every count is RELATIVE to the windows closed before the call.
constexpr uint32_t kSliceTile = 1024;        // events per workgroup: 256 lanes x 4 consecutive records
constexpr uint32_t kSliceScanLanes = 256;    // lanes of k_slice_scan's workgroup: each owns ceil(tiles / lanes) consecutive tiles' maxima
constexpr uint32_t kSliceMaxWindows = 4096;  // ESVIO_FE_SLICE_MAX_WINDOWS
struct SliceResult {  // written by k_slice_scan (first_of_last: k_slice_cuts); one per camera, the cuts behind it
  uint32_t closed;         // windows the call closes (the maximum of c over its events)
  uint32_t overflow;       // an event lies at or beyond the last boundary of the call's range: nothing else is valid
  uint32_t first_of_last;  // index of the first event of the window left open (untouched when closed == 0)
  uint32_t reserved;
};
static_assert(sizeof(SliceResult) == 16, "SliceResult layout");
constexpr uint32_t kSliceResWords = sizeof(SliceResult) / 4 + kSliceMaxWindows;  // a camera's result block and its cuts
struct SliceCam {
  const EventRec* ev;   // [n] device memory
  uint32_t n;
  uint32_t tiles;       // ceil(n / kSliceTile); 0: the camera takes no part
  const double* bounds; // [n_bounds] toSec(E_k) of the windows open or ahead at the call's start, ascending (windows at
                        // given stamps: the caller's, non-decreasing, and one closing +inf that no stamp reaches)
  uint32_t n_bounds;    // <= kSliceMaxWindows + 1; c == n_bounds is the overflow
  uint32_t* tmax;       // [tiles] reduce: the tiles' maxima; scan: their exclusive prefix maxima
  SliceResult* res;
  uint32_t* cuts;       // [kSliceMaxWindows] entry j: the first event that does not belong to the j-th window closed
};
struct SliceArgs {
  SliceCam cam[2];  // the grid's blocks: cam[0].tiles, then cam[1].tiles
};
void launch_slice_reduce(hipStream_t s, const SliceArgs& a);
void launch_slice_scan(hipStream_t s, const SliceArgs& a);
void launch_slice_cuts(hipStream_t s, const SliceArgs& a);

struct SelectArgs {
  const uint32_t* comp_xy;   // compacted candidates in stream order
  const uint32_t* comp_idx;
  const uint32_t* total;     // number of candidates
  int W, H, wpr;
  int max_corners;
  int radius;
  int8_t hw[kMaxDiscR + 1];  // cv::circle half-widths per |dy|
  // >= 0: "|dx| <= hw[|dy|]" is the same set as "dx*dx + dy*dy <= disc_c" (true for cv::circle's
  // table at every radius 1..63 and for the open Euclidean disc; disc_threshold() checks it), so
  // disc membership is two multiply-adds instead of a table look-up; -1: use the table
  int disc_c;
  float2* out_pts;           // accepted corners are written at out_pts[out_base + k]
  int32_t* out_idx;          // may be NULL
  int out_base;
  int* n_out;                // number accepted
  int* n_total;              // out_base + accepted (feeds the LK kernels' n_ptr), may be NULL
  int* host_counts;          // optional host-mapped mirror: {accepted, out_base + accepted, total}
  // non-null: the disc bitmap lives here (H*wpr + 4 words of device memory) instead of in LDS — for
  // sensors whose bitmap does not fit the 160 KiB (k_select_gbm; LDS then holds the tables only)
  uint32_t* gbitmap;
  const uint32_t* init_bits; // optional H*wpr words the disc bitmap starts from (blocked pixels)
  // ... or, instead, the points whose discs ARE those blocked pixels (Event_setMask stamps
  // cv::circle(mask, cvRound(pt), MIN_DIST, 0, -1) for every point it keeps, feature_tracker.cpp
  // :77-86): the wave stamps them itself, so the host uploads n_stamp points, not a bitmap.
  // Needs n_stamp more LDS words behind the half-width table.
  const float2* stamp_pts;
  int n_stamp;
  // optional publication of each accepted corner the moment it is accepted, for an LK launch that
  // is already waiting (LkArgs::poll_*): slot[out_base + k] = seq<<32 | y<<16 | x, and at the end
  // *done = seq<<32 | (out_base + accepted).  Device memory, relaxed agent-scope atomics; the data
  // travels in the flag word itself, so no fence is needed.
  unsigned long long* pub_slots;
  unsigned long long* pub_done;
  uint32_t pub_seq;
  // != 0: the one-wave walk (k_select) even where the 16-wave kernel's queue fits LDS beside the bitmap
  // (sensors between ~1.2 and 1.3 M pixels take it for lack of LDS; ESVIO_FE_SELECT_SERIAL=1, test-only)
  int one_wave;
};
KernelId launch_select(hipStream_t s, const SelectArgs& a, size_t lds_bytes);  // (returns the form it launched)
// the threshold described at SelectArgs::disc_c for a half-width table, or -1 if there is none
inline int disc_threshold(const int8_t* hw, int radius) {
  long inside = -1, outside = (long)(radius + 1) * (radius + 1);
  for (int dy = 0; dy <= radius && dy <= kMaxDiscR; dy++) {
    const long h = hw[dy];
    if (h >= 0) inside = inside > h * h + (long)dy * dy ? inside : h * h + (long)dy * dy;
    const long o = (h + 1) * (h + 1) + (long)dy * dy;  // (h = -1: the row's centre pixel is outside)
    outside = outside < o ? outside : o;
  }
  return inside >= 0 && inside < outside ? (int)inside : -1;
}

// ---- loop-closure keyframes: blur, BRIEF, matching (esvio_fe_kf_*) ----
// include/esvio_fe.h "keyframes" holds the rules (B, F, D, M); all of it is integer arithmetic except D's one float
// addition.  F runs on k_fast_score<9> / k_fast_collect / k_compact above as they are.  Three kernels of their own,
// booked in timer slots of their own behind the event images' (esvio_fe_kf_kernel_*), outside the stage and ingest
// tables.  No kernel waits on another workgroup; every loop is bounded by its arguments.
//   k_kf_blur   cv::GaussianBlur(9 x 9, sigma 2) of an 8-bit image: a kKfBlurTileW x kKfBlurTileH tile per workgroup;
//               the tile and its 4-pixel halo go into LDS once, the reflect-101 indices resolved at the load; the row
//               pass leaves 16-bit sums in LDS (exact: at most 255 * 256), the column pass reads them, rounds once
//               ((sum + 2^15) >> 16) and stores 4 pixels per lane — as one word where the four lie in the row and their
//               address is a word's, byte by byte elsewhere (a width that is no multiple of 4).
//   k_kf_brief  one wave per point, 4 tests per lane; the pattern (4 x 256 int8: x1 | y1 | x2 | y2) is copied into LDS
//               by the workgroup; the gathers go to the blurred plane (dense, width bytes per row); a lane's 4 bits
//               are OR-ed over its group of 8 lanes by shuffles into one of the point's 8 words, which lanes 0 and 32
//               store as two 16-byte stores.
//   k_kf_match  one workgroup per query: its 8 words in registers, the lanes stride over the train set (8 x xor +
//               popcount); the reduction runs on the key dist << 20 | index, wave then block, so that the minimum key
//               is the FIRST index of the minimal distance whatever order the lanes finish in.  nt <= 2^20.
constexpr int kKfBlurTileW = 64, kKfBlurTileH = 16;
constexpr int kKfPatternTests = 256;
constexpr uint32_t kKfMatchMaxTrain = 1u << 20;
constexpr int kKfBestInit = 128, kKfMatchDist = 80;  // ESVIO_FE_KF_BEST_INIT, ESVIO_FE_KF_MATCH_DIST
// src: pixel (0,0), rows src_stride bytes apart; dst: dense width x height
void launch_kf_blur(hipStream_t s, const uint8_t* src, int src_stride, int W, int H, uint8_t* dst);
// pattern: [4][256] int8 (device); pts: [n] (x, y); desc: [n][8] words, 16-byte aligned
void launch_kf_brief(hipStream_t s, const uint8_t* blurred, int W, int H, const int8_t* pattern, const float2* pts,
                     uint32_t n, uint32_t* desc);
// query [nq][8], train [nt][8] words, both 16-byte aligned; idx / dist [nq] int32, status [nq] bytes.  nq >= 1
void launch_kf_match(hipStream_t s, const uint32_t* query, uint32_t nq, const uint32_t* train, uint32_t nt, int32_t* idx,
                     int32_t* dist, uint8_t* status);

// ---- loop detection: DBoW2 words, vectors, the database's L1 scores (esvio_fe_bow_*) ----
// include/esvio_fe.h "loop detection" holds the rules (V, W, T, A, Q, L): Hamming distances, integer sorting and IEEE
// double additions, subtractions and one division in a stated order; no product anywhere.  Four kernels of their own in
// timer slots behind the keyframes' (esvio_fe_bow_kernel_*); the sort between the first two is k_radix_pass as it is.
// No kernel of the four waits on another workgroup; every loop is bounded by its arguments and by the tree, which the
// host has checked (fe_bow.h: every child index lies inside the node arrays, every walk ends at a leaf).
// The tree on the device: node 0 is the root, every node's children are contiguous and in child order —
// kids[node] = {first child, child count}, count 0 at a leaf; node_desc[node] 8 words; node_word / node_weight at leaves.
//   k_bow_walk    W: kBowGroup lanes per descriptor, 4 descriptors per wave.  A lane takes one child per round (32 bytes
//                 as two 16-byte loads) and keeps its least distance with the lowest rank; the group reduces the distance,
//                 then the rank among the lanes that hold that distance: the first child of the least distance, whatever
//                 lane held it.  More children than lanes: more rounds.  Leaves word and weight per descriptor, and the
//                 sort's input: key = word (or invalid_key, above every word, where the weight is not > 0), value =
//                 index, the digit histograms of `passes` 8-bit passes.
//   k_bow_vector  T behind the sort, ONE workgroup: the heads of the runs of equal keys compacted in order (ballot
//                 ranks), run lengths as counts, per word the weight added count times one after another (repeat != 0)
//                 or the weight itself, then the norm — lane 0 adds 1024 staged values at a time in ascending word order,
//                 the chain the rule prescribes — and the division.  out[0] = words in the vector.
//   k_bow_score   Q's sums: one wave per database entry (grid-stride), the entry's words in chunks of 64, each lane
//                 looks its word up in the query's sorted words (binary search; in LDS up to kBowLdsWords words, in memory
//                 beyond), the matching lanes' terms are added in lane (= word) order.  score[e], present[e].
//   k_bow_select  one workgroup: max_results times the least (order-preserving bits of score, id) above the last one taken.
constexpr int kBowGroup = 16;
constexpr int kBowLdsWords = 4096;
constexpr int kBowMaxResults = 64;
constexpr int kBowVectorBlock = 1024;
// desc [n][8] words, 16-byte aligned; word / weight / keys / vals [n]; ghist: the sort scratch's, cleared.  n >= 1
void launch_bow_walk(hipStream_t s, const uint32_t* desc, uint32_t n, const uint4* node_desc, const uint2* kids,
                     const int32_t* node_word, const double* node_weight, uint32_t invalid_key, int passes, int32_t* word,
                     double* weight, uint32_t* keys, uint32_t* vals, uint32_t* ghist);
// keys [n] sorted; heads [n] scratch; vec_word / vec_val [n]; out [2]: words in the vector, keys below invalid_key.  n >= 1
void launch_bow_vector(hipStream_t s, const uint32_t* keys, uint32_t n, uint32_t invalid_key, const double* word_weight,
                       int repeat, uint32_t* heads, uint32_t* vec_word, double* vec_val, uint32_t* out);
// the query's m words; the database's pools and offsets [n_entries + 1]; score / present [n_entries].  n_entries >= 1
void launch_bow_score(hipStream_t s, const uint32_t* q_word, const double* q_val, uint32_t m, const uint32_t* db_word,
                      const double* db_val, const uint64_t* db_off, uint32_t n_entries, int max_id, double* score,
                      uint8_t* present);
// out_id / out_score / out_raw [max_results], *out_n: how many; out_score = -raw / 2.  n_entries >= 1
void launch_bow_select(hipStream_t s, const double* score, const uint8_t* present, uint32_t n_entries, int max_results,
                       int32_t* out_id, double* out_score, double* out_raw, uint32_t* out_n);

// ---- vocabulary creation: k-means++ seeding, k-means passes, regrouping, document counts (esvio_fe_bow_create_*) ----
// include/esvio_fe.h "C, creating a vocabulary" holds the rule: Hamming distances, integer sums and counts, and in C5 one
// double division and one product per draw (__ddiv_rn / __dmul_rn, nothing to contract).  The tree grows breadth first,
// one level's nodes together (fe_voc.h drives it).  A level's features are `na` POSITIONS: perm[i] the feature at position
// i, segof[i] its segment (= a node of the level that is split), ascending, a segment's positions in feature order.  A
// segment with more than k features is a K-MEANS NODE x (seg_km[s] = x, else -1) and owns ncent[x] <= k centres of 8
// words at centres[(x k + c) 8]; one with at most k features has one cluster per feature and needs no centre.  A k-means
// node with at least kVocBigNode features is BIG (km_big[x] = its index among them, else -1).
//   k_voc_first        C2's first centre: one lane per k-means node, draw 0, RandomInt.
//   k_voc_mindist      one lane per position: min_dist against the node's newest centre (first != 0: against the first,
//                      stored as it is); a min_dist of 0 stays (C2's `if(*dit > 0)`).
//   k_voc_scan_reduce, k_voc_scan_top, k_voc_scan_down: the inclusive u64 running sums run[] of min_dist over ALL
//                      positions, kVocScanTile per workgroup — a node's running sum at i is run[i] - run[start - 1], so no
//                      scan knows of segments.  Three launches, no workgroup waits for another.
//   k_voc_draw         one lane per k-means node: dist_sum = run[end - 1] - run[start - 1]; 0 stops the node's seeding
//                      (stopped[x] = 1, cut_d[x] = -1), else cut_d[x] by C5, drawn again while it is 0.0.
//   k_voc_pick         one lane per segment: the first position whose (double)(running sum) >= cut_d by bisection (run[]
//                      ascends), the last one if none; with take != 0 the feature there becomes the node's next centre.
//   k_voc_assign       one lane per position: the least distance's lowest cluster; centres from LDS where the workgroup's
//                      256 positions lie in one node, from memory otherwise.  changed[x] = 1 where a lane's cluster
//                      differs from the one it held.  m <= k segments: the cluster is the position's rank in its segment.
//   k_voc_count_big    C3's counts of the big nodes: 8 lanes per feature (one word each), kVocScanTile positions per
//                      workgroup, LDS counters [k][257] (256 bits and the group's size) flushed by integer atomics.  A big
//                      node holds more positions than a tile, so only a tile's first and last segment can be big: the
//                      tile counts its part of each, one after the other.
//   k_voc_mean_big     one lane per (big node, cluster, word): bit set iff its count > size / 2.
//   k_voc_mean_small   one workgroup per k-means node that is not big: counts in LDS, then the centres.
//   k_voc_child_count  slot_size[seg_slot[s] + cluster] += 1 per position: the sizes of the level's children (through
//                      <= 32 LDS counters where the workgroup's 256 positions lie in one k-means node).
//   k_voc_regroup_keys the stable sort's input for the next level: key = slot_map[child slot] (the child's segment on the
//                      next level, or the `dead` key of a child that is not split), value = the feature; digit histograms.
//   k_voc_doc_count    behind k_bow_walk and the stable sort by word: Ni[word] += 1 at every position where the word or
//                      the document (bisection in doc_offsets) differs from the position before.
constexpr uint32_t kVocBigNode = 4096;
constexpr int kVocScanTile = 2048;
constexpr uint32_t kVocScanLanes = 256;  // lanes of k_voc_scan_top's one workgroup: each owns ceil(tiles / lanes) consecutive tiles' sums
struct VocArgs {
  const uint32_t* desc;     // [n][8], 16-byte aligned
  uint32_t na, n_seg, n_km, n_big;
  int k;
  const uint32_t* perm;     // [na]
  const uint32_t* segof;    // [na]
  const uint32_t* seg_off;  // [n_seg + 1]
  const int32_t* seg_km;    // [n_seg]
  const uint32_t* seg_slot; // [n_seg] the segment's first child slot
  const uint32_t* km_start; // [n_km] first position, and one behind the last
  const uint32_t* km_end;
  const uint64_t* km_key;   // [n_km] C5's key of the node
  const int32_t* km_big;    // [n_km]
  const uint32_t* big_km;   // [n_big]
  uint32_t* ncent;          // [n_km] each: centres so far, draws taken, seeding stopped short, assignment changed
  uint32_t* draws;
  uint32_t* stopped;
  uint32_t* changed;
  uint32_t* centres;        // [n_km][k][8]
  double* cut_d;            // [n_km]
  uint32_t* pick;           // [n_km]
  uint32_t* min_dist;       // [na]
  uint64_t* run;            // [na]
  uint64_t* tile_sum;       // [tiles of na]
  uint32_t* assign;         // [na]
  uint32_t* counts;         // [n_big][k][257]
  uint32_t* slot_size;      // [slots]
};
// splitmix64 (C5)
inline __host__ __device__ uint64_t voc_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline __host__ __device__ uint32_t voc_draw(uint64_t key, uint32_t j) { return (uint32_t)(voc_mix(key ^ ((uint64_t)(j + 1u) << 32)) >> 33); }
inline uint32_t voc_tiles(uint32_t n) { return (n + kVocScanTile - 1) / kVocScanTile; }
void launch_voc_first(hipStream_t s, const VocArgs& a);
void launch_voc_mindist(hipStream_t s, const VocArgs& a, int first);
// run[i] = min_dist[0] + ... + min_dist[i] for i < n; tile_sum: voc_tiles(n) words.  n >= 1
void launch_voc_scan_reduce(hipStream_t s, const uint32_t* min_dist, uint32_t n, uint64_t* tile_sum);
void launch_voc_scan_top(hipStream_t s, uint64_t* tile_sum, uint32_t tiles);
void launch_voc_scan_down(hipStream_t s, const uint32_t* min_dist, uint32_t n, const uint64_t* tile_sum, uint64_t* run);
void launch_voc_draw(hipStream_t s, const VocArgs& a);
// start / end / cut_d / pick [n_seg]; a cut_d that is not >= 0 or an empty segment gives pick 0xffffffff; take: a's
// centres grow by the picked feature (n_seg = a.n_km then)
void launch_voc_pick(hipStream_t s, const uint64_t* run, const uint32_t* start, const uint32_t* end, const double* cut_d,
                     uint32_t n_seg, uint32_t* pick, const VocArgs& a, int take);
void launch_voc_assign(hipStream_t s, const VocArgs& a, int first);
void launch_voc_count_big(hipStream_t s, const VocArgs& a);
void launch_voc_mean_big(hipStream_t s, const VocArgs& a);
void launch_voc_mean_small(hipStream_t s, const VocArgs& a);
void launch_voc_child_count(hipStream_t s, const VocArgs& a);
// keys / vals [a.na]; ghist: the sort scratch's, cleared
void launch_voc_regroup_keys(hipStream_t s, const VocArgs& a, const uint32_t* slot_map, int passes, uint32_t* keys,
                             uint32_t* vals, uint32_t* ghist);
// keys (words) sorted stably, vals the features; doc_off [n_docs + 1] with doc_off[0] = 0 and doc_off[n_docs] > every
// feature; ni [n_words] cleared
void launch_voc_doc_count(hipStream_t s, const uint32_t* keys, const uint32_t* vals, uint32_t n, const int64_t* doc_off,
                          uint32_t n_docs, uint32_t n_words, uint32_t* ni);


}  // namespace esvio
