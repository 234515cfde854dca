// fe_kf.h — the host side of the keyframe stage (esvio_fe_kf_*): KeyFrame::KeyFrame's image passes
// (pose_graph/src/keyframe.cpp:34-63) and searchByBRIEFDes (:183-232).  include/esvio_fe.h "keyframes" holds the rules,
// fe_kernels.h the kernels, esvio_fe_ctx::Kf the scratch.  Included by fe_api.cpp alone, behind its last entry point.
#pragma once
#include "fe_internal.h"

namespace {
using Kf = esvio_fe_ctx::Kf;
constexpr int kKfMaxPoints = 1 << 20;

// a keyframe call's device allocations go into the latency record's counter (esvio_fe_latency::allocs), as a track
// call's do: the second call of a size adds none
struct KfAllocs {
  esvio_fe_ctx* c;
  uint64_t before;
  explicit KfAllocs(esvio_fe_ctx* ctx) : c(ctx), before(ctx->n_allocs) {}
  ~KfAllocs() { c->lat.allocs += c->n_allocs - before; }
};

bool kf_space_ok(int space) { return space == ESVIO_FE_HOST || space == ESVIO_FE_DEVICE; }
bool kf_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
// a device descriptor array: two 16-byte accesses per descriptor
bool kf_desc_aligned(const void* p, int space) { return space != ESVIO_FE_DEVICE || ((uintptr_t)p & 15u) == 0; }

// the checks of an image argument, before any device work
int kf_image_check(esvio_fe_ctx* c, const char* who, int cam, const uint8_t* img, int space) {
  if (cam != 0 && cam != 1) return fail(c, ESVIO_FE_EINVAL, "%s: cam must be 0 or 1 (got %d)", who, cam);
  if (img && !kf_space_ok(space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d", who, space);
  if (!img && c->cfg.equalize != 0)
    return fail(c, ESVIO_FE_EINVAL, "%s: img == NULL with equalize: the handle's plane is the CLAHE image, the pose graph takes the raw frame", who);
  return 0;
}
// ... and where the kernels read it, on the main stream: the handle's own plane where it lies (the main stream is
// behind whatever rendered it, as for esvio_fe_fast_corners), a device image in place, a host image's copy
int kf_image_source(esvio_fe_ctx* c, int cam, const uint8_t* img, int space, const uint8_t** src, int* stride) {
  *src = img;
  *stride = c->W;
  if (!img) {
    const PyrDesc& d = cam ? c->pyr[c->slot_curR].d : c->pyr[c->slot_curL].d;
    *src = px00(d);
    *stride = d.stride[0];
  } else if (space == ESVIO_FE_HOST) {
    Kf& K = c->kf;
    if (!K.img)
      if (int rc = K.img.alloc(c, c->P)) return rc;
    HIPCHK(c, hipMemcpyAsync(K.img, img, c->P, hipMemcpyHostToDevice, cur_stream(c)));
    *src = K.img;
  }
  return 0;
}

int kf_blur_enqueue(esvio_fe_ctx* c, const uint8_t* src, int stride, uint8_t* dst) {
  ScopedKernel k(c, K_KF_BLUR, 2 * (uint64_t)c->P);  // the image read once, the blurred plane written
  launch_kf_blur(cur_stream(c), src, stride, c->W, c->H, dst);
  return 0;
}
int kf_blur_plane(esvio_fe_ctx* c) { return c->kf.blur ? 0 : c->kf.blur.alloc(c, c->P); }

// D at n points that lie in K.pts from `first` on, on the blurred plane at `blurred` (device, dense): the descriptors go
// to desc where that is device memory, through K.desc (from `first` on as well) where it is the host's.  Nothing is
// waited for.
int kf_brief_enqueue(esvio_fe_ctx* c, const uint8_t* blurred, size_t first, uint32_t n, uint32_t* desc, int desc_space) {
  if (!n) return 0;
  Kf& K = c->kf;
  hipStream_t s = cur_stream(c);
  uint32_t* d = desc_space == ESVIO_FE_DEVICE ? desc : K.desc.p + first * 8;
  {
    ScopedKernel k(c, K_KF_BRIEF, (uint64_t)n * (8 + 32 + 2 * kKfPatternTests));  // the point, the words, two gathered bytes per test
    launch_kf_brief(s, blurred, c->W, c->H, K.d_pat, K.pts.p + first, n, d);
  }
  if (desc_space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(desc, d, (size_t)n * 32, hipMemcpyDeviceToHost, s));
  return 0;
}
// room for n points (and their descriptors behind a host destination), the points themselves uploaded
int kf_points_upload(esvio_fe_ctx* c, const float* pts, size_t n, bool host_desc) {
  Kf& K = c->kf;
  if (!n) return 0;
  if (int rc = K.pts.grow(c, n)) return rc;
  if (host_desc)
    if (int rc = K.desc.grow(c, n * 8)) return rc;
  HIPCHK(c, hipMemcpyAsync(K.pts, pts, n * 8, hipMemcpyHostToDevice, cur_stream(c)));
  return 0;
}
}  // namespace

extern "C" {

int esvio_fe_kf_kernel_count(void) { return kKfKernels; }
const char* esvio_fe_kf_kernel_name(int which) { return which >= 0 && which < kKfKernels ? kKfKernelNames[which] : ""; }
int esvio_fe_kf_kernel_stats(esvio_fe_handle c, int which, double* total_ms, uint64_t* launches, uint64_t* alg_bytes) {
  if (!c || which < 0 || which >= kKfKernels) return ESVIO_FE_EINVAL;
  HIPCHK(c, hipSetDevice(c->dev));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  resolve_profile(c);
  const KStat& s = c->stats[K_KF_BLUR + which];
  if (total_ms) *total_ms = s.ms;
  if (launches) *launches = s.launches;
  if (alg_bytes) *alg_bytes = s.bytes;
  return 0;
}
int esvio_fe_kf_blur_tile(int32_t* tile_w, int32_t* tile_h) {
  if (!tile_w || !tile_h) return ESVIO_FE_EINVAL;
  *tile_w = kKfBlurTileW, *tile_h = kKfBlurTileH;
  return 0;
}

int esvio_fe_kf_set_pattern(esvio_fe_handle c, const int32_t* x1, const int32_t* y1, const int32_t* x2, const int32_t* y2, int n) {
  if (!c) return ESVIO_FE_EINVAL;
  KfAllocs allocs(c);
  if (!x1 || !y1 || !x2 || !y2) return fail(c, ESVIO_FE_EINVAL, "kf_set_pattern: a null array");
  if (n != kKfPatternTests) return fail(c, ESVIO_FE_EINVAL, "kf_set_pattern: the pattern has %d tests (got %d)", kKfPatternTests, n);
  const int32_t* src[4] = {x1, y1, x2, y2};
  for (int a = 0; a < 4; a++)
    for (int i = 0; i < n; i++)
      if (src[a][i] < -127 || src[a][i] > 127)
        return fail(c, ESVIO_FE_EINVAL, "kf_set_pattern: |offset| must be <= 127 (array %d, entry %d: %d)", a, i, src[a][i]);
  Kf& K = c->kf;
  HIPCHK(c, hipSetDevice(c->dev));
  if (!K.d_pat)
    if (int rc = K.d_pat.alloc(c, sizeof K.pat)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));  // (a descriptor call never returns with its launch in flight; the copy below reads K.pat)
  for (int a = 0; a < 4; a++)
    for (int i = 0; i < n; i++) K.pat[a * kKfPatternTests + i] = (int8_t)src[a][i];
  HIPCHK(c, hipMemcpyAsync(K.d_pat, K.pat, sizeof K.pat, hipMemcpyHostToDevice, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  K.has_pattern = true;
  return 0;
}

int esvio_fe_kf_blur(esvio_fe_handle c, const uint8_t* img, int space, uint8_t* dst, int dst_space) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "kf_blur";
  KfAllocs allocs(c);
  if (int rc = kf_image_check(c, who, 0, img, space)) return rc;
  if (!dst) return fail(c, ESVIO_FE_EINVAL, "%s: dst is null", who);
  if (!kf_space_ok(dst_space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d of dst", who, dst_space);
  if (img && space == dst_space && kf_overlap(img, c->P, dst, c->P)) return fail(c, ESVIO_FE_EINVAL, "%s: dst overlaps img", who);
  HIPCHK(c, hipSetDevice(c->dev));
  const uint8_t* src;
  int stride;
  if (int rc = kf_image_source(c, 0, img, space, &src, &stride)) return rc;
  uint8_t* out = dst;
  if (dst_space == ESVIO_FE_HOST) {
    if (int rc = kf_blur_plane(c)) return rc;
    out = c->kf.blur;
  }
  if (int rc = kf_blur_enqueue(c, src, stride, out)) return rc;
  if (dst_space == ESVIO_FE_HOST) HIPCHK(c, hipMemcpyAsync(dst, out, c->P, hipMemcpyDeviceToHost, cur_stream(c)));
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_kf_fast(esvio_fe_handle c, const uint8_t* img, int space, int threshold, float* out_xy, int32_t* out_score,
                     int32_t capacity, int32_t* n_out, int32_t* n_detected) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "kf_fast";
  KfAllocs allocs(c);
  if (n_out) *n_out = 0;
  if (n_detected) *n_detected = 0;
  if (!n_out) return fail(c, ESVIO_FE_EINVAL, "%s: n_out is null", who);
  if (int rc = kf_image_check(c, who, 0, img, space)) return rc;
  if (threshold < 0 || threshold > 255) return fail(c, ESVIO_FE_EINVAL, "%s: threshold must be in 0..255 (got %d)", who, threshold);
  if (capacity < 0 || (capacity > 0 && !out_xy)) return fail(c, ESVIO_FE_EINVAL, "%s: capacity %d without out_xy", who, capacity);
  HIPCHK(c, hipSetDevice(c->dev));
  const uint8_t* src;
  int stride;
  if (int rc = kf_image_source(c, 0, img, space, &src, &stride)) return rc;
  Kf& K = c->kf;
  if (int rc = fast_keyframe_run(c, src, stride, threshold, K.h_xy, K.h_score, n_detected)) return rc;
  const size_t k = std::min<size_t>(K.h_xy.size(), (size_t)capacity);
  for (size_t i = 0; i < k; i++) {
    out_xy[2 * i] = (float)(K.h_xy[i] & 0xffffu), out_xy[2 * i + 1] = (float)(K.h_xy[i] >> 16);
    if (out_score) out_score[i] = (int32_t)K.h_score[i];
  }
  *n_out = (int32_t)K.h_xy.size();
  return 0;
}

int esvio_fe_kf_brief(esvio_fe_handle c, const uint8_t* blurred, int space, const float* pts, int n, uint32_t* desc, int desc_space) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "kf_brief";
  KfAllocs allocs(c);
  if (!blurred) return fail(c, ESVIO_FE_EINVAL, "%s: the blurred image is null", who);
  if (!kf_space_ok(space) || !kf_space_ok(desc_space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space", who);
  if (n < 0 || n > kKfMaxPoints) return fail(c, ESVIO_FE_EINVAL, "%s: n must be in 0..2^20 (got %d)", who, n);
  if (n && (!pts || !desc)) return fail(c, ESVIO_FE_EINVAL, "%s: pts or desc is null with n = %d", who, n);
  if (n && !kf_desc_aligned(desc, desc_space)) return fail(c, ESVIO_FE_EINVAL, "%s: device descriptors must be 16-byte aligned", who);
  if (!c->kf.has_pattern) return fail(c, ESVIO_FE_EINVAL, "%s: no pattern is set (esvio_fe_kf_set_pattern)", who);
  if (!n) return 0;
  HIPCHK(c, hipSetDevice(c->dev));
  const uint8_t* src;
  int stride;
  if (int rc = kf_image_source(c, 0, blurred, space, &src, &stride)) return rc;
  if (int rc = kf_points_upload(c, pts, (size_t)n, desc_space == ESVIO_FE_HOST)) return rc;
  if (int rc = kf_brief_enqueue(c, src, 0, (uint32_t)n, desc, desc_space)) return rc;
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_kf_match(esvio_fe_handle c, const uint32_t* query, int nq, const uint32_t* train, int nt, int space, int32_t* idx,
                      int32_t* dist, uint8_t* status) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "kf_match";
  KfAllocs allocs(c);
  if (!kf_space_ok(space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d", who, space);
  if (nq < 0 || nq > kKfMaxPoints) return fail(c, ESVIO_FE_EINVAL, "%s: nq must be in 0..2^20 (got %d)", who, nq);
  if (nt < 0 || (uint32_t)nt > kKfMatchMaxTrain) return fail(c, ESVIO_FE_EINVAL, "%s: nt must be in 0..2^20 (got %d)", who, nt);
  if (nq && (!idx || !dist || !status)) return fail(c, ESVIO_FE_EINVAL, "%s: a null result array with nq = %d", who, nq);
  if (nq && nt && (!query || !train)) return fail(c, ESVIO_FE_EINVAL, "%s: null descriptors", who);
  if (nq && nt && (!kf_desc_aligned(query, space) || !kf_desc_aligned(train, space)))
    return fail(c, ESVIO_FE_EINVAL, "%s: device descriptors must be 16-byte aligned", who);
  if (!nq) return 0;
  if (!nt) {  // `bestIndex = -1, bestDist = 128` and an empty loop
    for (int i = 0; i < nq; i++) idx[i] = -1, dist[i] = ESVIO_FE_KF_BEST_INIT, status[i] = 0;
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->dev));
  Kf& K = c->kf;
  hipStream_t s = cur_stream(c);
  const uint32_t *dq = query, *dt = train;
  if (space == ESVIO_FE_HOST) {
    if (int rc = K.q.grow(c, (size_t)nq * 8)) return rc;
    if (int rc = K.t.grow(c, (size_t)nt * 8)) return rc;
    HIPCHK(c, hipMemcpyAsync(K.q, query, (size_t)nq * 32, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(K.t, train, (size_t)nt * 32, hipMemcpyHostToDevice, s));
    dq = K.q, dt = K.t;
  }
  // idx | dist | status
  if (int rc = K.res.grow(c, (size_t)nq * 2 + ((size_t)nq + 3) / 4)) return rc;
  int32_t *d_idx = K.res, *d_dist = K.res.p + nq;
  uint8_t* d_status = (uint8_t*)(K.res.p + 2 * (size_t)nq);
  {
    ScopedKernel k(c, K_KF_MATCH, ((uint64_t)nq + (uint64_t)nt) * 32 + (uint64_t)nq * 9);  // every descriptor once, the results
    launch_kf_match(s, dq, (uint32_t)nq, dt, (uint32_t)nt, d_idx, d_dist, d_status);
  }
  HIPCHK(c, hipMemcpyAsync(idx, d_idx, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(dist, d_dist, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(status, d_status, (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

int esvio_fe_kf_describe(esvio_fe_handle c, int cam, const uint8_t* img, int space, const float* window_pts, int n_window,
                         int fast_threshold, esvio_fe_kf_out* out) {
  if (!c) return ESVIO_FE_EINVAL;
  const char* who = "kf_describe";
  KfAllocs allocs(c);
  if (!out) return fail(c, ESVIO_FE_EINVAL, "%s: out is null", who);
  out->n_kp = out->n_detected = 0;
  if (int rc = kf_image_check(c, who, cam, img, space)) return rc;
  if (fast_threshold < 0 || fast_threshold > 255) return fail(c, ESVIO_FE_EINVAL, "%s: fast_threshold must be in 0..255 (got %d)", who, fast_threshold);
  if (n_window < 0 || n_window > kKfMaxPoints) return fail(c, ESVIO_FE_EINVAL, "%s: n_window must be in 0..2^20 (got %d)", who, n_window);
  if (n_window && (!window_pts || !out->window_desc)) return fail(c, ESVIO_FE_EINVAL, "%s: window_pts or window_desc is null with n_window = %d", who, n_window);
  if (out->kp_capacity < 0 || out->kp_capacity > kKfMaxPoints) return fail(c, ESVIO_FE_EINVAL, "%s: kp_capacity must be in 0..2^20 (got %d)", who, out->kp_capacity);
  if (!kf_space_ok(out->desc_space)) return fail(c, ESVIO_FE_EINVAL, "%s: bad memory space %d of the descriptors", who, out->desc_space);
  if ((n_window && !kf_desc_aligned(out->window_desc, out->desc_space)) || (out->kp_desc && !kf_desc_aligned(out->kp_desc, out->desc_space)))
    return fail(c, ESVIO_FE_EINVAL, "%s: device descriptors must be 16-byte aligned", who);
  if (!c->kf.has_pattern) return fail(c, ESVIO_FE_EINVAL, "%s: no pattern is set (esvio_fe_kf_set_pattern)", who);
  HIPCHK(c, hipSetDevice(c->dev));
  Kf& K = c->kf;
  const uint8_t* src;
  int stride;
  if (int rc = kf_image_source(c, cam, img, space, &src, &stride)) return rc;
  if (int rc = kf_blur_plane(c)) return rc;
  if (int rc = kf_blur_enqueue(c, src, stride, K.blur)) return rc;  // ONE blur: both compute*BRIEFPoint calls see this plane
  // cv::FAST on the image itself (keyframe.cpp:138); the call waits for the list, the blur has run by then
  if (int rc = fast_keyframe_run(c, src, stride, fast_threshold, K.h_xy, K.h_score, &out->n_detected)) return rc;
  const size_t k = std::min<size_t>(K.h_xy.size(), (size_t)out->kp_capacity), nw = (size_t)n_window;
  out->n_kp = (int32_t)K.h_xy.size();
  // the window points, then the kept corners as cv::KeyPoint::pt has them
  K.h_pts.resize((nw + k) * 2);
  if (nw) memcpy(K.h_pts.data(), window_pts, nw * 8);
  float* kp = K.h_pts.data() + nw * 2;
  for (size_t i = 0; i < k; i++) kp[2 * i] = (float)(K.h_xy[i] & 0xffffu), kp[2 * i + 1] = (float)(K.h_xy[i] >> 16);
  const bool host_desc = out->desc_space == ESVIO_FE_HOST;
  const size_t nd = nw + (out->kp_desc ? k : 0);
  if (int rc = kf_points_upload(c, K.h_pts.data(), nd, host_desc)) return rc;
  if (int rc = kf_brief_enqueue(c, K.blur, 0, (uint32_t)nw, out->window_desc, out->desc_space)) return rc;
  if (out->kp_desc)
    if (int rc = kf_brief_enqueue(c, K.blur, nw, (uint32_t)k, out->kp_desc, out->desc_space)) return rc;
  // under the descriptor launches: the host's part (keyframe.cpp:153-160; z = 1)
  if (k && out->kp_xy) memcpy(out->kp_xy, kp, k * 8);
  if (out->kp_score)
    for (size_t i = 0; i < k; i++) out->kp_score[i] = (int32_t)K.h_score[i];
  if (k && out->kp_norm) {
    K.lift_x.resize(k), K.lift_y.resize(k);
    host::lift_projective_batch(c->cfg.cam[cam], kp, (int)k, K.lift_x.data(), K.lift_y.data());
    for (size_t i = 0; i < k; i++) out->kp_norm[2 * i] = (float)(K.lift_x[i] / 1.0), out->kp_norm[2 * i + 1] = (float)(K.lift_y[i] / 1.0);
  }
  HIPCHK(c, hipStreamSynchronize(cur_stream(c)));
  HIPCHK(c, hipGetLastError());
  if (c->prof_on) resolve_profile(c);
  return 0;
}

}  // extern "C"
