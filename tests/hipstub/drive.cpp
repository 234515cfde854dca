// Driver of the ThreadSanitizer build of the library's host side (tests/hipstub, tests/test_host_tsan.py): the soak's
// toggling pattern over the C ABI — replay mode with batches announced up to four ahead from pageable memory (the
// staging helpers), the launch thread switched on and off mid-stream, 0..7 RANSAC helpers, lazy mode on and off,
// plain calls in between, calls that must fail (a published frame announced as unpublished), esvio_fe_reset with
// batches announced and in flight, handles created and destroyed.  The device is fake (fake_device.cpp): what is
// under test is every thread the library starts and every hand-over between them.  Before that, handles of a few
// configurations pass once through every entry point that allocates on first use (first_use_pass); after the last
// esvio_fe_destroy the stub's count of live device blocks, pinned blocks, events and streams is printed.
// The last line is a digest of what every successful track call and esvio_fe_finish returned (n_left, n_right, ids,
// cur_pts, ids_right, cur_right_pts, both velocity arrays): two builds of the library that compute the same print the same.
//   drive <seed> <frames>      exit 0: done; the sanitizer reports on stderr
//   drive trace                with HIPSTUB_TRACE=<file>: one thread, a fixed matrix of handles and calls (trace_matrix
//                              below); the file then holds every launch and stream call in order, with its stream, and
//                              per handle what the profiling API counted (tests/test_launch_trace.py)
//   drive trace_cand           the same for the paths that leave per-block candidate lists and the matrix above never
//                              reaches (trace_cand_matrix below; tests/test_launch_trace_cand.py)
//   drive trace_ingest         the same for the ingest entry points — decode, decode-and-track and the feed over raw words,
//                              AEDAT packets and bag chunks —, with every call's return code, error text and info struct
//                              (trace_ingest_matrix below; tests/test_launch_trace_ingest.py)
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "esvio_fe.h"
#if __has_include("esvio_fe_test.h")  // (trees from before the header was split have the taps in esvio_fe.h)
#include "esvio_fe_test.h"
extern "C" void hipstub_arm_faults(int on);  // tests/hipstub/hip_stub.cpp
extern "C" void hipstub_live(long out[4]);
extern "C" void hipstub_trace_on(int on);
extern "C" void hipstub_trace_note(const char* text);
extern "C" void hipstub_set_compact_total(uint32_t n);
extern "C" void hipstub_set_ingest(int k, uint32_t events, uint32_t untimed, unsigned long long bad, long long first_t, long long last_t,
                                   uint32_t st_th, uint32_t st_flags, uint32_t st_bx, uint32_t st_wraps);  // tests/hipstub/fake_device.cpp
extern "C" void hipstub_set_baf(int on, uint32_t kept, int err);
extern "C" void hipstub_set_baf_err_at(int nth);
#endif

static uint32_t rs;
static uint32_t rnd() { return rs = rs * 1664525u + 1013904223u; }

static uint64_t digest = 1469598103934665603ull;  // FNV-1a
static void fold(const void* p, size_t bytes) {
  for (size_t i = 0; i < bytes; i++) digest = (digest ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
}
static void fold_tracks(const esvio_fe_tracks& t) {
  const size_t nl = (size_t)t.n_left, nr = (size_t)t.n_right;
  fold(&t.n_left, 4);
  fold(&t.n_right, 4);
  fold(t.ids, nl * 4);
  fold(t.cur_pts, nl * 8);
  fold(t.ids_right, nr * 4);
  fold(t.cur_right_pts, nr * 8);
  fold(t.pts_velocity, nl * 8);
  fold(t.right_pts_velocity, nr * 8);
}

struct Batch {
  std::vector<esvio_fe_event> L, R;
  double t;
};

// The latest call's latency record: identities of the bookkeeping, whatever the clock read (1e-6 ms: the rounding of
// summed clock differences).  Phases 8..13 are parts of phase 5 and of published calls only, 15 is part of 0, and
// 0..7 with 14 lie end to end inside the call.
static bool latency_record_ok(esvio_fe_handle h, int pub) {
  esvio_fe_latency_call r;
  if (esvio_fe_latency_recent(h, 0, &r) != ESVIO_FE_OK) return false;
  double main_sum = r.phase_ms[14], pub_sum = 0;
  bool ok = r.published == (pub != 0);
  for (int i = 0; i < ESVIO_FE_LATENCY_PHASES; i++) {
    ok = ok && r.phase_ms[i] >= 0;
    if (i < 8) main_sum += r.phase_ms[i];
    else if (i < 14) pub_sum += r.phase_ms[i];
    const char* name = esvio_fe_latency_phase_name(i);
    ok = ok && name[0] != 0;
    for (int k = 0; k < i; k++) ok = ok && strcmp(name, esvio_fe_latency_phase_name(k)) != 0;
  }
  ok = ok && (pub ? pub_sum <= r.phase_ms[5] + 1e-6 : pub_sum == 0) && r.phase_ms[15] <= r.phase_ms[0] + 1e-6 &&
       main_sum <= r.ms + 1e-6;
  if (!ok) {
    fprintf(stderr, "latency record of call %llu (%s, %.6f ms):", (unsigned long long)r.call, pub ? "published" : "unpublished", r.ms);
    for (int i = 0; i < ESVIO_FE_LATENCY_PHASES; i++) fprintf(stderr, " %d=%.6f", i, r.phase_ms[i]);
    fprintf(stderr, "\n");
  }
  return ok;
}
static void make_batch(Batch& b, int W, int H, int frame, int n) {
  b.L.resize((size_t)n);
  b.R.resize((size_t)n * 3 / 4);
  const uint32_t sec = 1700000000u + (uint32_t)frame / 30u;
  for (auto* v : {&b.L, &b.R}) {
    uint32_t ns = (uint32_t)(frame % 30) * 33000000u;
    for (auto& e : *v) {
      std::memset(&e, 0, sizeof(e));
      e.x = (uint16_t)(rnd() % (uint32_t)W);
      e.y = (uint16_t)(rnd() % (uint32_t)H);
      ns += rnd() % 2000u;
      e.sec = sec;
      e.nsec = ns;
      e.polarity = (uint8_t)(rnd() & 1u);
    }
  }
  b.t = (double)sec + 1e-9 * (double)b.L.back().nsec;
}

// One handle through the entry points that allocate on first use (the stub kernels do nothing: the point is the
// allocations and the teardown).  Returns the number of calls that failed.
static int first_use_pass(esvio_fe_config c, int W, int H, bool images) {
  c.width = W; c.height = H;
  for (int k = 0; k < 2; k++) { c.cam[k].fx = c.cam[k].fy = 0.9 * W; c.cam[k].cx = W / 2.0; c.cam[k].cy = H / 2.0; }
  const int M = c.max_cnt;
  const size_t P = (size_t)W * H;
  esvio_fe_handle h = nullptr;
  if (esvio_fe_create(&c, &h) != ESVIO_FE_OK) return 1;
  int bad = 0;
#define OK(call)                                                                                \
  do {                                                                                          \
    if ((call) != ESVIO_FE_OK) {                                                                \
      bad++;                                                                                    \
      fprintf(stderr, "first_use_pass %dx%d: %s: %s\n", W, H, #call, esvio_fe_last_error(h));   \
    }                                                                                           \
  } while (0)
  std::vector<int32_t> ids((size_t)M), cnt((size_t)M), idr((size_t)M);
  std::vector<float> f2[6];
  for (auto& v : f2) v.resize(2 * (size_t)M);
  esvio_fe_tracks t;
  std::memset(&t, 0, sizeof(t));
  t.ids = ids.data(); t.track_cnt = cnt.data(); t.cur_pts = f2[0].data(); t.cur_un_pts = f2[1].data();
  t.pts_velocity = f2[2].data(); t.ids_right = idr.data(); t.cur_right_pts = f2[3].data();
  t.cur_un_right_pts = f2[4].data(); t.right_pts_velocity = f2[5].data();
  std::vector<uint8_t> img(P, 7), img2(P, 9), st((size_t)M);
  std::vector<float> xy(2 * (size_t)M, 40.f), xy2(2 * (size_t)M);
  int32_t n = 0, n_det = 0, lw = 0, lh = 0, nl = 0;
  OK(esvio_fe_set_profiling(h, 1));  // (the profiling event pool and its pending records)
  if (images) {
    std::vector<int16_t> fxy(2 * 64);
    std::vector<int32_t> fsc(64);
    OK(esvio_fe_fast_corners(h, 0, nullptr, ESVIO_FE_HOST, 10, 20, 1, fxy.data(), fsc.data(), 64, &n, &n_det));
    OK(esvio_fe_fast_corners(h, 0, img.data(), ESVIO_FE_HOST, 9, 20, 0, fxy.data(), nullptr, 64, &n, &n_det));
    OK(esvio_fe_good_features_to_track(h, img.data(), M, 0.01, 10.0, nullptr, xy2.data(), &n, nullptr));
    OK(esvio_fe_calc_optical_flow_pyr_lk(h, img.data(), img2.data(), W, H, xy.data(), xy2.data(), st.data(), M, 3, 30, 0.01, 0));
    OK(esvio_fe_calc_optical_flow_pyr_lk(h, img.data(), img2.data(), W / 2, H / 2, xy.data(), xy2.data(), st.data(), M, 3, 30, 0.01, 0));
    std::vector<uint8_t> lvl(P);
    std::vector<int16_t> der(2 * P);
    OK(esvio_fe_build_pyramid(h, img.data(), W, H, 3, 1, lvl.data(), der.data(), &lw, &lh, &nl));
    OK(esvio_fe_track_image(h, 1.0, img.data(), img2.data(), 1, &t));
    OK(esvio_fe_track_image(h, 1.03, img2.data(), img.data(), 1, &t));
    OK(esvio_fe_reset(h));
  }
  Batch b[3];
  for (int i = 0; i < 3; i++) make_batch(b[i], W, H, i, 9000);
  uint64_t rej = 0;
  {  // the time-sliced update: scratch planes, the staging of host-side slice planes
    const size_t nd = esvio_fe_sae_plane_doubles(h);
    std::vector<double> last(nd), s_out(nd);
    OK(esvio_fe_sae_slice_last(h, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, last.data(), ESVIO_FE_HOST));
    OK(esvio_fe_sae_slice_apply(h, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, last.data(), 1,
                                ESVIO_FE_HOST, s_out.data(), ESVIO_FE_HOST));
    OK(esvio_fe_sae_slice_commit(h, last.data(), s_out.data(), 1, ESVIO_FE_HOST));
    OK(esvio_fe_reset(h));
  }
  OK(esvio_fe_create_sae_stereo(h, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, &rej));
  {
    std::vector<uint8_t> flags(b[0].L.size());
    OK(esvio_fe_is_corner(h, b[0].L.data(), b[0].L.size(), ESVIO_FE_HOST, flags.data()));
    OK(esvio_fe_features_to_track(h, b[0].L.data(), b[0].L.size(), ESVIO_FE_HOST, M, nullptr, xy2.data(), nullptr, &n));
  }
  esvio_fe_motion mo;
  std::memset(&mo, 0, sizeof(mo));
  mo.t1 = b[0].t; mo.accel[0] = 9.f; mo.fx = mo.fy = 0.9 * W; mo.cx = W / 2.0; mo.cy = H / 2.0;
  OK(esvio_fe_create_sae_stereo_mc(h, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, &mo, &rej));
  // a plain call, a motion-compensated one, then an announced batch: all from pageable memory
  OK(esvio_fe_track_event(h, b[0].t, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, 1, &t));
  mo.t1 = b[1].t;
  OK(esvio_fe_set_next_batch(h, b[2].t, b[2].L.data(), b[2].L.size(), b[2].R.data(), b[2].R.size(), ESVIO_FE_HOST, 1));
  OK(esvio_fe_track_event_mc(h, b[1].t, b[1].L.data(), b[1].L.size(), b[1].R.data(), b[1].R.size(), ESVIO_FE_HOST, 1, &mo, &t));
  OK(esvio_fe_track_event(h, b[2].t, b[2].L.data(), b[2].L.size(), b[2].R.data(), b[2].R.size(), ESVIO_FE_HOST, 1, &t));
  OK(esvio_fe_finish(h, &t));
  OK(esvio_fe_reserve(h, 1u << 17, 1u << 17, 1));  // (every buffer grows once more)
#undef OK
  esvio_fe_destroy(h);
  return bad;
}

// ---- drive trace.  No launch thread, no RANSAC helpers, no staging threads: every HIP call is made by this thread,
// so the order of the lines is the order of the code.  The handles' creation is left out of the trace (its warm-up
// alone is 1200 lines); everything from there to the profile counters is in.
static int trace_bad = 0;
static void note(const char* fmt, const char* a, int b = 0, int c2 = 0) {
  char buf[256];
  snprintf(buf, sizeof(buf), fmt, a, b, c2);
  hipstub_trace_note(buf);
}
#define TR(call)                                                                  \
  do {                                                                            \
    note("-- %s", #call);                                                         \
    if ((call) != ESVIO_FE_OK) {                                                  \
      trace_bad++;                                                                \
      fprintf(stderr, "drive trace: %s: %s\n", #call, esvio_fe_last_error(h));    \
    }                                                                             \
  } while (0)

static esvio_fe_handle trace_create(const char* label, esvio_fe_config c, int W, int H) {
  c.width = W; c.height = H;
  for (int k = 0; k < 2; k++) { c.cam[k].fx = c.cam[k].fy = 0.9 * W; c.cam[k].cx = W / 2.0; c.cam[k].cy = H / 2.0; }
  note("== %s %d x %d", label, W, H);
  esvio_fe_handle h = nullptr;
  hipstub_trace_on(0);
  const int rc = esvio_fe_create(&c, &h);
  if (rc == ESVIO_FE_OK) esvio_fe_set_profiling(h, 1);
  hipstub_trace_on(1);
  if (rc != ESVIO_FE_OK) { trace_bad++; return nullptr; }
  rs = 1;
  return h;
}

static void trace_destroy(esvio_fe_handle h, int kernels = esvio_fe_kernel_count()) {
  for (int id = 0; id < kernels; id++) {
    uint64_t launches = 0, bytes = 0;
    hipstub_trace_on(0);
    esvio_fe_get_kernel_stats(h, id, nullptr, &launches, &bytes);
    hipstub_trace_on(1);
    char buf[128];
    snprintf(buf, sizeof(buf), "profile %s launches %llu bytes %llu", esvio_fe_kernel_name(id), (unsigned long long)launches,
             (unsigned long long)bytes);
    hipstub_trace_note(buf);
  }
  esvio_fe_destroy(h);
}

struct TraceOut {
  std::vector<int32_t> ids, cnt, idr;
  std::vector<float> f2[6];
  esvio_fe_tracks t;
  explicit TraceOut(int M) : ids((size_t)M), cnt((size_t)M), idr((size_t)M) {
    for (auto& v : f2) v.resize(2 * (size_t)M);
    std::memset(&t, 0, sizeof(t));
    t.ids = ids.data(); t.track_cnt = cnt.data(); t.cur_pts = f2[0].data(); t.cur_un_pts = f2[1].data();
    t.pts_velocity = f2[2].data(); t.ids_right = idr.data(); t.cur_right_pts = f2[3].data();
    t.cur_un_right_pts = f2[4].data(); t.right_pts_velocity = f2[5].data();
  }
};

static void trace_event_handle(const char* label, const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create(label, c, W, H);
  if (!h) return;
  const int M = c.max_cnt;
  TraceOut o(M);
  esvio_fe_tracks& t = o.t;
  Batch b[9];
  for (int i = 0; i < 9; i++) make_batch(b[i], W, H, i, 3000 + 100 * i);
#define EV(i) b[i].t, b[i].L.data(), b[i].L.size(), b[i].R.data(), b[i].R.size()
  // plain calls: batches in "device" memory (the stub's device memory is the host's), then in pageable memory
  TR(esvio_fe_track_event(h, EV(0), ESVIO_FE_DEVICE, 1, &t));
  TR(esvio_fe_track_event(h, EV(1), ESVIO_FE_DEVICE, 0, &t));
  TR(esvio_fe_track_event(h, EV(2), ESVIO_FE_DEVICE, 1, &t));
  TR(esvio_fe_track_event(h, EV(3), ESVIO_FE_HOST, 1, &t));
  TR(esvio_fe_track_event(h, EV(4), ESVIO_FE_HOST, 0, &t));
  TR(esvio_fe_track_event(h, EV(5), ESVIO_FE_HOST, 1, &t));
  // two batches announced ahead
  TR(esvio_fe_set_next_batch(h, EV(6), ESVIO_FE_HOST, 1));
  TR(esvio_fe_set_next_batch(h, EV(7), ESVIO_FE_HOST, 0));
  TR(esvio_fe_track_event(h, EV(6), ESVIO_FE_HOST, 1, &t));
  TR(esvio_fe_track_event(h, EV(7), ESVIO_FE_HOST, 0, &t));
  TR(esvio_fe_finish(h, &t));
  // the right camera's image brought in from outside, then the frame it belongs to
  std::vector<uint8_t> img((size_t)W * H, 7);
  TR(esvio_fe_import_image(h, 1, img.data(), ESVIO_FE_HOST));
  TR(esvio_fe_track_event(h, EV(8), ESVIO_FE_DEVICE, 1, &t));
  TR(esvio_fe_sae_to_time_surface(h, 0, b[8].t, img.data()));
  TR(esvio_fe_sae_to_time_surface(h, 1, b[8].t, img.data()));
  std::vector<float> xy(2 * (size_t)M);
  int32_t n = 0;
  TR(esvio_fe_features_to_track(h, b[8].L.data(), b[8].L.size(), ESVIO_FE_HOST, M, nullptr, xy.data(), nullptr, &n));
#undef EV
  trace_destroy(h);
}

static void trace_image_handle(const char* label, const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create(label, c, W, H);
  if (!h) return;
  const int M = c.max_cnt;
  TraceOut o(M);
  const size_t P = (size_t)W * H;
  std::vector<uint8_t> img(P, 7), img2(P, 9);
  std::vector<float> xy(2 * (size_t)M);
  int32_t n = 0;
  TR(esvio_fe_track_image(h, 1.0, img.data(), img2.data(), 1, &o.t));
  TR(esvio_fe_track_image(h, 1.03, img2.data(), img.data(), 0, &o.t));
  TR(esvio_fe_track_image(h, 1.06, img.data(), nullptr, 1, &o.t));
  TR(esvio_fe_good_features_to_track(h, img.data(), M, 0.01, 10.0, nullptr, xy.data(), &n, nullptr));
  trace_destroy(h);
}

static int trace_finish(const char* mode) {
  long live[4];
  hipstub_live(live);
  char buf[128];
  snprintf(buf, sizeof(buf), "live: device %ld pinned %ld events %ld streams %ld", live[0], live[1], live[2], live[3]);
  hipstub_trace_note(buf);
  if (trace_bad) fprintf(stderr, "drive %s: %d calls failed\n", mode, trace_bad);
  return trace_bad ? 6 : 0;
}

static int trace_matrix(esvio_fe_config c) {
  setenv("ESVIO_FE_STAGE_THREADS", "0", 1);
  hipstub_arm_faults(0);
  hipstub_set_compact_total(1000);
  const int W = 346, H = 260;
  esvio_fe_config eq = c, med = c;
  eq.equalize = 1;
  med.median_blur_kernel_size = 1;
  trace_event_handle("default", c, W, H);
  trace_event_handle("equalize", eq, W, H);
  trace_event_handle("median_blur_kernel_size=1", med, W, H);
  setenv("ESVIO_FE_NO_FUSE", "1", 1);
  trace_event_handle("ESVIO_FE_NO_FUSE", c, W, H);
  trace_event_handle("equalize ESVIO_FE_NO_FUSE", eq, W, H);
  unsetenv("ESVIO_FE_NO_FUSE");
  setenv("ESVIO_FE_SAE_SORT", "1", 1);
  trace_event_handle("ESVIO_FE_SAE_SORT", c, W, H);
  unsetenv("ESVIO_FE_SAE_SORT");
  setenv("ESVIO_FE_NO_CAMSPLIT", "1", 1);
  trace_event_handle("ESVIO_FE_NO_CAMSPLIT", c, W, H);
  unsetenv("ESVIO_FE_NO_CAMSPLIT");
  trace_event_handle("pyramid of fewer than three levels", c, 160, 120);
  trace_event_handle("selection bitmap in device memory", c, 1920, 1080);
  trace_image_handle("images", c, W, H);
  trace_image_handle("images equalize", eq, W, H);
  return trace_finish("trace");
}

// ---- drive trace_cand: every path that fills per-block candidate lists and has them compacted — esvio_fe_fast_corners,
// FAST as trackEvent's detector and its stage tap, the Arc* pass with k_dedup, goodFeaturesToTrack
static void trace_fast_corners(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_fast_corners", c, W, H);
  if (!h) return;
  std::vector<uint8_t> img((size_t)W * H, 7);
  std::vector<int16_t> fxy(2 * 64);
  std::vector<int32_t> fsc(64);
  int32_t n = 0, n_det = 0;
  // the handle's time surface, then a host image (the fake compaction reports 1000 corners: 64 are copied out)
  TR(esvio_fe_fast_corners(h, 0, nullptr, ESVIO_FE_HOST, 10, 20, 1, fxy.data(), fsc.data(), 64, &n, &n_det));
  TR(esvio_fe_fast_corners(h, 0, nullptr, ESVIO_FE_HOST, 10, 20, 0, fxy.data(), fsc.data(), 64, &n, &n_det));
  TR(esvio_fe_fast_corners(h, 1, nullptr, ESVIO_FE_HOST, 9, 20, 0, fxy.data(), nullptr, 64, &n, &n_det));
  TR(esvio_fe_fast_corners(h, 0, img.data(), ESVIO_FE_HOST, 10, 20, 1, fxy.data(), fsc.data(), 64, &n, &n_det));
  TR(esvio_fe_fast_corners(h, 0, img.data(), ESVIO_FE_HOST, 10, 20, 0, fxy.data(), nullptr, 64, &n, nullptr));
  TR(esvio_fe_fast_corners(h, 0, img.data(), ESVIO_FE_HOST, 9, 20, 0, fxy.data(), nullptr, 0, &n, &n_det));
  trace_destroy(h);
}

static void trace_fast_detector(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("ESVIO_FE_DETECT_FAST", c, W, H);
  if (!h) return;
  const int M = c.max_cnt;
  TraceOut o(M);
  esvio_fe_tracks& t = o.t;
  Batch b[4];
  for (int i = 0; i < 4; i++) make_batch(b[i], W, H, i, 3000 + 100 * i);
#define EV(i) b[i].t, b[i].L.data(), b[i].L.size(), b[i].R.data(), b[i].R.size()
  TR(esvio_fe_set_detector(h, ESVIO_FE_DETECT_FAST, 20));
  TR(esvio_fe_track_event(h, EV(0), ESVIO_FE_HOST, 1, &t));
  TR(esvio_fe_set_next_batch(h, EV(1), ESVIO_FE_HOST, 1));
  TR(esvio_fe_track_event(h, EV(1), ESVIO_FE_HOST, 1, &t));
  TR(esvio_fe_finish(h, &t));
  std::vector<uint8_t> img((size_t)W * H, 7), mask((size_t)W * H, 0);
  std::vector<float> xy(2 * (size_t)M);
  std::vector<int32_t> sc((size_t)M);
  int32_t n = 0, n_cand = 0;
  TR(esvio_fe_features_to_track_fast(h, nullptr, ESVIO_FE_HOST, 20, M, nullptr, xy.data(), sc.data(), &n, &n_cand));
  TR(esvio_fe_features_to_track_fast(h, img.data(), ESVIO_FE_HOST, 20, M, mask.data(), xy.data(), nullptr, &n, nullptr));
  TR(esvio_fe_set_next_batch(h, EV(2), ESVIO_FE_HOST, 1));
  TR(esvio_fe_reset(h));
  TR(esvio_fe_track_event(h, EV(3), ESVIO_FE_HOST, 1, &t));
#undef EV
  trace_destroy(h);
}

static void trace_dedup_handle(const char* label, const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create(label, c, W, H);
  if (!h) return;
  const int M = c.max_cnt;
  TraceOut o(M);
  Batch b[2];
  for (int i = 0; i < 2; i++) make_batch(b[i], W, H, i, 3000 + 100 * i);
  TR(esvio_fe_track_event(h, b[0].t, b[0].L.data(), b[0].L.size(), b[0].R.data(), b[0].R.size(), ESVIO_FE_HOST, 1, &o.t));
  TR(esvio_fe_set_next_batch(h, b[1].t, b[1].L.data(), b[1].L.size(), b[1].R.data(), b[1].R.size(), ESVIO_FE_HOST, 1));
  TR(esvio_fe_track_event(h, b[1].t, b[1].L.data(), b[1].L.size(), b[1].R.data(), b[1].R.size(), ESVIO_FE_HOST, 1, &o.t));
  TR(esvio_fe_finish(h, &o.t));
  std::vector<float> xy(2 * (size_t)M);
  int32_t n = 0;
  TR(esvio_fe_features_to_track(h, b[1].L.data(), b[1].L.size(), ESVIO_FE_HOST, M, nullptr, xy.data(), nullptr, &n));
  trace_destroy(h);
}

static void trace_gftt_handle(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_good_features_to_track", c, W, H);
  if (!h) return;
  const int M = c.max_cnt;
  std::vector<uint8_t> img((size_t)W * H, 7), mask((size_t)W * H, 0);
  std::vector<float> xy(2 * (size_t)M);
  int32_t n = 0;
  TR(esvio_fe_good_features_to_track(h, img.data(), M, 0.01, 10.0, nullptr, xy.data(), &n, nullptr));
  TR(esvio_fe_good_features_to_track(h, img.data(), M, 0.01, 10.0, mask.data(), xy.data(), &n, nullptr));
  trace_destroy(h);
}

static int trace_cand_matrix(esvio_fe_config c) {
  setenv("ESVIO_FE_STAGE_THREADS", "0", 1);
  hipstub_arm_faults(0);
  hipstub_set_compact_total(1000);
  const int W = 346, H = 260;
  trace_fast_corners(c, W, H);
  trace_fast_detector(c, W, H);
  esvio_fe_config big = c;
  big.max_cnt = 600;
  trace_dedup_handle("k_dedup: max_cnt 600", big, W, H);
  setenv("ESVIO_FE_DEDUP", "1", 1);
  trace_dedup_handle("k_dedup: ESVIO_FE_DEDUP", c, W, H);
  unsetenv("ESVIO_FE_DEDUP");
  trace_gftt_handle(c, W, H);
  return trace_finish("trace_cand");
}

// ---- drive trace_ingest: the ingest entry points.  The fake emit launchers report what the driver sets beforehand
// (hipstub_set_ingest: the result block of job slot 0 / 1), so refusals and the repeated emit are walked; calls may fail
// here, and behind every call the trace holds its return code, the error text of a failed one and the info struct.
// slot k reports `events` records, `bad` of them BAD; th: the TIME_HIGH the raw state is left with (every call another one)
static void ingest_set(int k, uint32_t events, unsigned long long bad, uint32_t th, uint32_t untimed = 0) {
  const long long t0 = 1700000000ll * 1000000 + th;  // (microsecond ticks; AEDAT reads them as ns, the bag as ns too)
  hipstub_set_ingest(k, events, untimed, bad, t0, t0 + 900, th, 1u | 16u | (th & 0xfffu) << 8 | 7u << 20, 3 + th, 1);
}
static void notef(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void notef(const char* fmt, ...) {
  char buf[700];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  hipstub_trace_note(buf);
}
// a call that may fail: its text, its return code, the error text of a failed one
#define TI(call)                                                   \
  do {                                                             \
    note("-- %s", #call);                                          \
    const int rc_ = (call);                                        \
    if (rc_) notef("   rc %d: %s", rc_, esvio_fe_last_error(h));   \
    else notef("   rc 0");                                         \
  } while (0)
#define U(x) (unsigned long long)(x)
// both slots of a two-camera call (th: the function's running TIME_HIGH)
#define BOTH(eL, eR, badL, badR) do { ingest_set(0, eL, badL, ++th); ingest_set(1, eR, badR, ++th); } while (0)
static void show(const esvio_fe_raw_info& i) {
  notef("   raw_info events %llu untimed %llu other %llu bad %llu wraps %llu first_t_us %lld last_t_us %lld", U(i.events), U(i.untimed),
        U(i.other), U(i.bad), U(i.wraps), (long long)i.first_t_us, (long long)i.last_t_us);
}
static void show(const esvio_fe_trigger_info& i) {
  notef("   trigger_info triggers %llu untimed %llu bad %llu wraps %llu first_t_us %lld last_t_us %lld", U(i.triggers), U(i.untimed), U(i.bad),
        U(i.wraps), (long long)i.first_t_us, (long long)i.last_t_us);
}
static void show(const esvio_fe_aedat_info& i) {
  notef("   aedat_info events %llu invalid %llu bad %llu polarity_packets %llu other_packets %llu first_t_us %lld last_t_us %lld", U(i.events),
        U(i.invalid), U(i.bad), U(i.polarity_packets), U(i.other_packets), (long long)i.first_t_us, (long long)i.last_t_us);
}
static void show(const esvio_fe_bag_info& i) {
  for (int cam = 0; cam < 2; cam++)
    notef("   bag_info cam %d events %llu bad %llu messages %llu first %u.%09u last %u.%09u", cam, U(i.cam[cam].events), U(i.cam[cam].bad),
          U(i.cam[cam].messages), i.cam[cam].first_sec, i.cam[cam].first_nsec, i.cam[cam].last_sec, i.cam[cam].last_nsec);
  notef("   bag_info other_messages %llu other_records %llu chunks %llu connections %llu", U(i.other_messages), U(i.other_records), U(i.chunks),
        U(i.connections));
}
static void show(const esvio_fe_batch_info& i) {
  notef("   batch_info kept %llu %llu rejected %llu %llu bad %llu %llu cur_time %.9f tracked %d reserved %d", U(i.kept[0]), U(i.kept[1]),
        U(i.rejected[0]), U(i.rejected[1]), U(i.bad[0]), U(i.bad[1]), i.cur_time, i.tracked, i.reserved);
}
static void show(const esvio_fe_feed_info& i) {
  notef("   feed_info appended %llu rejected %llu bad %llu closed %llu queued %llu", U(i.appended), U(i.rejected), U(i.bad), U(i.closed), U(i.queued));
}
template <class T>
static T stale() {  // an info struct a call has to overwrite: what stays 0x55 was left alone
  T v;
  memset(&v, 0x55, sizeof v);
  return v;
}

// AEDAT 3.1: `packets` packets of `events` 8-byte records each, of the given type (1: polarity); ts in microseconds
static std::vector<uint8_t> aedat_chunk(int packets, int events, int type = 1, int32_t size = 8) {
  std::vector<uint8_t> v;
  auto i32 = [&](int32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)((uint32_t)x >> 8 * k)); };
  for (int p = 0; p < packets; p++) {
    v.push_back((uint8_t)type), v.push_back(0), v.push_back(0), v.push_back(0);  // eventType, eventSource
    i32(size), i32(4), i32(0), i32(events), i32(events), i32(events);            // size, tsOffset, tsOverflow, capacity, number, valid
    for (int e = 0; e < events; e++) i32(1 | 10 << 2 | 20 << 17), i32(1000 * p + e);
  }
  return v;
}
// rosbag v2.0 behind the magic: the two event connections, then a message of nL events on /l and one of nR on /r
static std::vector<uint8_t> bag_chunk(uint32_t nL, uint32_t nR, uint32_t seq) {
  std::vector<uint8_t> v;
  auto u32 = [](std::vector<uint8_t>& o, uint32_t x) { for (int k = 0; k < 4; k++) o.push_back((uint8_t)(x >> 8 * k)); };
  auto field = [&](std::vector<uint8_t>& o, const char* name, const void* val, size_t n) {
    u32(o, (uint32_t)(strlen(name) + 1 + n));
    o.insert(o.end(), name, name + strlen(name));
    o.push_back('=');
    o.insert(o.end(), (const uint8_t*)val, (const uint8_t*)val + n);
  };
  auto record = [&](const std::vector<uint8_t>& hdr, const std::vector<uint8_t>& data) {
    u32(v, (uint32_t)hdr.size()), v.insert(v.end(), hdr.begin(), hdr.end());
    u32(v, (uint32_t)data.size()), v.insert(v.end(), data.begin(), data.end());
  };
  const char* topic[2] = {"/l", "/r"};
  const uint32_t n[2] = {nL, nR};
  for (uint32_t cam = 0; cam < 2; cam++) {
    std::vector<uint8_t> hdr, data;
    const uint8_t op = 7;
    field(hdr, "op", &op, 1), field(hdr, "conn", &cam, 4), field(hdr, "topic", topic[cam], 2);
    field(data, "type", "dvs_msgs/EventArray", 19), field(data, "md5sum", "5e8beee5a6c107e504c2e78903c224b8", 32);
    record(hdr, data);
  }
  for (uint32_t cam = 0; cam < 2; cam++) {
    if (!n[cam]) continue;
    std::vector<uint8_t> hdr, data;
    const uint8_t op = 2;
    const uint32_t time[2] = {1700000000u, seq};
    field(hdr, "op", &op, 1), field(hdr, "conn", &cam, 4), field(hdr, "time", time, 8);
    u32(data, seq), u32(data, 1700000000u), u32(data, seq * 1000u), u32(data, 0);  // seq, stamp, frame_id ""
    u32(data, 260), u32(data, 346), u32(data, n[cam]);
    for (uint32_t e = 0; e < n[cam]; e++) {
      data.push_back((uint8_t)e), data.push_back(0), data.push_back(9), data.push_back(0);  // x, y
      u32(data, 1700000000u), u32(data, seq * 1000u + e), data.push_back(1);
    }
    record(hdr, data);
  }
  return v;
}

static esvio_fe_motion ingest_motion(int W, int H) {
  esvio_fe_motion mo;
  std::memset(&mo, 0, sizeof(mo));
  mo.t1 = 1700000000.0, mo.accel[0] = 9.f, mo.fx = mo.fy = 0.9 * W, mo.cx = W / 2.0, mo.cy = H / 2.0;
  return mo;
}

static void ingest_decode_raw(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_decode_raw, esvio_fe_decode_triggers", c, W, H);
  if (!h) return;
  const size_t nb = (size_t)esvio_fe_raw_tile_bytes() + 8;  // two tiles, a whole number of words of every format
  std::vector<uint8_t> words(nb), pinned(nb);
  std::vector<esvio_fe_event> dst(40000);
  std::vector<esvio_fe_trigger> tdst(8000);
  esvio_fe_register_host_buffer(pinned.data(), pinned.size());
  uint32_t th = 100;
  const int formats[3] = {ESVIO_FE_RAW_EVT2, ESVIO_FE_RAW_EVT3, ESVIO_FE_RAW_EVT21};
  for (int f = 0; f < 3; f++)
    for (int src = 0; src < 3; src++)
      for (int ds = 0; ds < 2; ds++) {
        const void* w = src == 1 ? pinned.data() : words.data();
        const int space = src == 2 ? ESVIO_FE_DEVICE : ESVIO_FE_HOST, dspace = ds ? ESVIO_FE_DEVICE : ESVIO_FE_HOST;
        notef(".. format %d, source %s, dst %s", formats[f], src == 0 ? "host pageable" : src == 1 ? "host registered" : "device", ds ? "device" : "host");
        ingest_set(0, 700 + th, 0, th);
        esvio_fe_raw_info info = stale<esvio_fe_raw_info>();
        TI(esvio_fe_decode_raw(h, f & 1, formats[f], w, nb, space, 5, dst.data(), dst.size(), dspace, &info));
        show(info);
        th++;
      }
  const int F = ESVIO_FE_RAW_EVT3;
  esvio_fe_raw_info info;
#define RAW(cap_dst, cap) do { info = stale<esvio_fe_raw_info>(); TI(esvio_fe_decode_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, cap_dst, cap, ESVIO_FE_HOST, &info)); show(info); } while (0)
#define RAW_OK() do { ingest_set(0, 300, 0, ++th); RAW(dst.data(), dst.size()); } while (0)
  notef(".. ahead of the argument checks");
  info = stale<esvio_fe_raw_info>();
  TI(esvio_fe_decode_raw(h, 0, F, words.data(), 0, ESVIO_FE_HOST, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &info));
  show(info);
  info = stale<esvio_fe_raw_info>();
  TI(esvio_fe_decode_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, (esvio_fe_event*)((char*)dst.data() + 8), 100, ESVIO_FE_DEVICE, &info));
  show(info);
  RAW(nullptr, 100);
  info = stale<esvio_fe_raw_info>();
  TI(esvio_fe_decode_raw(h, 2, F, words.data(), nb, ESVIO_FE_HOST, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &info));
  TI(esvio_fe_decode_raw(h, 0, 4, words.data(), nb, ESVIO_FE_HOST, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &info));
  TI(esvio_fe_decode_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, dst.data(), dst.size(), 7, &info));
  RAW_OK();
  notef(".. behind the device work: bad stamps, no room, the emit again");
  ingest_set(0, 300, 2, ++th);
  RAW(dst.data(), dst.size());
  RAW_OK();
  ingest_set(0, 3000, 0, ++th);
  RAW(dst.data(), 2999);
  RAW_OK();
  ingest_set(0, 30000, 0, ++th);  // above one record per word, within dst_cap
  RAW(dst.data(), dst.size());
  RAW_OK();
  ingest_set(0, 0, 0, ++th, 12);  // no event at all: untimed ones
  RAW(dst.data(), dst.size());
#undef RAW
#undef RAW_OK
  notef(".. esvio_fe_decode_triggers");
  esvio_fe_trigger_info ti;
#define TRG(cap) do { ti = stale<esvio_fe_trigger_info>(); TI(esvio_fe_decode_triggers(h, 1, F, words.data(), nb, ESVIO_FE_HOST, 0, tdst.data(), cap, &ti)); show(ti); } while (0)
#define TRG_OK() do { ingest_set(0, 9, 0, ++th); TRG(tdst.size()); } while (0)
  TRG_OK();
  ingest_set(0, 9, 1, ++th);
  TRG(tdst.size());
  TRG_OK();
  ingest_set(0, 9, 0, ++th);
  TRG(8);
  TRG_OK();
  ingest_set(0, 5000, 0, ++th);  // above the 4096 the call starts with, within dst_cap
  TRG(tdst.size());
  TRG_OK();
  ti = stale<esvio_fe_trigger_info>();
  TI(esvio_fe_decode_triggers(h, 1, F, words.data(), nb, ESVIO_FE_HOST, 0, nullptr, 4, &ti));
  show(ti);
  TI(esvio_fe_decode_triggers(h, 1, F, words.data(), 0, ESVIO_FE_HOST, 0, tdst.data(), 4, &ti));
  show(ti);
#undef TRG
#undef TRG_OK
  notef(".. the event decoder again: its state is its own");
  ingest_set(0, 300, 0, ++th);
  info = stale<esvio_fe_raw_info>();
  TI(esvio_fe_decode_raw(h, 1, F, words.data(), nb, ESVIO_FE_HOST, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &info));
  show(info);
  TI(esvio_fe_decode_reset(h));
  info = stale<esvio_fe_raw_info>();
  TI(esvio_fe_decode_raw(h, 1, F, words.data(), nb, ESVIO_FE_HOST, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &info));
  show(info);
  TI(esvio_fe_reserve(h, 1u << 16, 1u << 16, 1));
  esvio_fe_unregister_host_buffer(pinned.data());
  trace_destroy(h, esvio_fe_ingest_kernel_count());
}

static void ingest_track_raw(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_track_raw", c, W, H);
  if (!h) return;
  TraceOut o(c.max_cnt);
  const size_t nb = (size_t)esvio_fe_raw_tile_bytes() + 8;
  std::vector<uint8_t> words(nb);
  const int F = ESVIO_FE_RAW_EVT3;
  const esvio_fe_filter_params flt{1000000, 1, 0, 0};
  const esvio_fe_motion mo = ingest_motion(W, H);
  uint32_t th = 200;
  esvio_fe_batch_info bi;
  esvio_fe_raw_info ri[2];
#define TRK(lb, rb, pub, filter, motion)                                                                                           \
  do {                                                                                                                             \
    bi = stale<esvio_fe_batch_info>(), ri[0] = ri[1] = stale<esvio_fe_raw_info>();                                                 \
    TI(esvio_fe_track_raw(h, F, words.data(), lb, words.data(), rb, ESVIO_FE_HOST, 0, pub, filter, motion, &o.t, &bi, ri));        \
    show(bi), show(ri[0]), show(ri[1]);                                                                                            \
  } while (0)
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  BOTH(900, 700, 0, 0);
  TRK(nb, (size_t)0, 0, nullptr, nullptr);
  BOTH(900, 700, 0, 0);
  TRK((size_t)0, nb, 1, nullptr, nullptr);
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, &mo);
  notef(".. with a filter");
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, &flt, nullptr);
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 0, &flt, &mo);
  notef(".. bad stamps on the right camera only; the next call's seeds are the ones before it");
  BOTH(900, 700, 0, 3);
  TRK(nb, nb, 1, nullptr, nullptr);
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  notef(".. the emit again: the right camera's events exceed the pair's room");
  BOTH(900, 100000, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  BOTH(100000, 900, 0, 0);
  TRK(nb, nb, 1, &flt, nullptr);
  notef(".. no left event: not tracked, the states move");
  BOTH(0, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  notef(".. the filter's body fails: the states stay");
  hipstub_set_baf(1, 0, 1);
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, &flt, nullptr);
  hipstub_set_baf(0, 0, 0);
  TI(esvio_fe_filter_reset(h));
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, &flt, nullptr);
  notef(".. refused: a bad filter, nothing to decode, a batch announced");
  const esvio_fe_filter_params bad_flt{1000000, 9, 0, 0};
  TRK(nb, nb, 1, &bad_flt, nullptr);
  TRK((size_t)0, (size_t)0, 1, nullptr, nullptr);
  Batch b;
  make_batch(b, W, H, 0, 3000);
  TI(esvio_fe_set_next_batch(h, b.t, b.L.data(), b.L.size(), b.R.data(), b.R.size(), ESVIO_FE_HOST, 1));
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  TI(esvio_fe_track_event(h, b.t, b.L.data(), b.L.size(), b.R.data(), b.R.size(), ESVIO_FE_HOST, 1, &o.t));
  TI(esvio_fe_finish(h, &o.t));
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  TI(esvio_fe_reset(h));
  BOTH(900, 700, 0, 0);
  TRK(nb, nb, 1, nullptr, nullptr);
  TI(esvio_fe_reserve(h, 1u << 16, 1u << 16, 1));
#undef TRK
  trace_destroy(h, esvio_fe_ingest_kernel_count());
}

static void ingest_aedat(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_decode_aedat, esvio_fe_track_aedat", c, W, H);
  if (!h) return;
  TraceOut o(c.max_cnt);
  const std::vector<uint8_t> ch = aedat_chunk(2, 5), big = aedat_chunk(2, 1500), other = aedat_chunk(1, 4, 7);
  std::vector<uint8_t> malformed = aedat_chunk(1, 5);
  malformed[4] = 9;  // a polarity packet whose eventSize is not 8
  std::vector<uint8_t> cut(ch.begin(), ch.begin() + 28 + 4);  // a header and half a record
  std::vector<esvio_fe_event> dst(4000);
  const esvio_fe_filter_params flt{1000000, 1, 0, 0};
  const esvio_fe_motion mo = ingest_motion(W, H);
  uint32_t th = 300;
  esvio_fe_aedat_info ai;
#define DEC(cam, chunk, flags, d, cap, dspace)                                                                         \
  do {                                                                                                                 \
    ai = stale<esvio_fe_aedat_info>();                                                                                 \
    TI(esvio_fe_decode_aedat(h, cam, chunk.data(), chunk.size(), 7, flags, d, cap, dspace, &ai));                      \
    show(ai);                                                                                                          \
  } while (0)
#define DEC_OK() do { ingest_set(0, 10, 0, ++th); DEC(0, ch, 0, dst.data(), dst.size(), ESVIO_FE_HOST); } while (0)
  for (int ds = 0; ds < 2; ds++)
    for (uint32_t flags = 0; flags < 2; flags++) {
      ingest_set(0, 8, 0, ++th, 2);
      DEC(0, ch, flags, dst.data(), dst.size(), ds ? ESVIO_FE_DEVICE : ESVIO_FE_HOST);
    }
  ingest_set(0, 2800, 0, ++th, 200);
  DEC(1, big, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  notef(".. ahead of the argument checks");
  ai = stale<esvio_fe_aedat_info>();
  TI(esvio_fe_decode_aedat(h, 0, ch.data(), 0, 0, 0, dst.data(), dst.size(), ESVIO_FE_HOST, &ai));
  show(ai);
  DEC(0, ch, 0, (esvio_fe_event*)((char*)dst.data() + 8), 100, ESVIO_FE_DEVICE);
  DEC(0, ch, 0, (esvio_fe_event*)nullptr, 100, ESVIO_FE_HOST);
  DEC(0, ch, 2u, dst.data(), dst.size(), ESVIO_FE_HOST);
  DEC(3, ch, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  DEC(0, ch, 0, dst.data(), dst.size(), 7);
  DEC(0, malformed, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  DEC_OK();
  notef(".. a chunk that completes no polarity record, then the rest of the record");
  DEC(0, cut, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  DEC(0, other, 0, dst.data(), dst.size(), ESVIO_FE_HOST);  // (inside the cut packet: its bytes are payload)
  TI(esvio_fe_decode_reset(h));
  DEC(0, other, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  notef(".. behind the device work: bad stamps, no room");
  ingest_set(0, 10, 1, ++th);
  DEC(0, ch, 0, dst.data(), dst.size(), ESVIO_FE_HOST);
  DEC_OK();
  ingest_set(0, 10, 0, ++th);
  DEC(0, ch, 0, dst.data(), (size_t)9, ESVIO_FE_HOST);
  ingest_set(0, 10, 0, ++th);
  DEC(0, ch, 1u, dst.data(), (size_t)9, ESVIO_FE_DEVICE);
  DEC_OK();
#undef DEC
#undef DEC_OK
  notef(".. esvio_fe_track_aedat");
  esvio_fe_batch_info bi;
  esvio_fe_aedat_info ri[2];
#define TRK(L, R, flags, pub, filter, motion)                                                                                         \
  do {                                                                                                                                \
    bi = stale<esvio_fe_batch_info>(), ri[0] = ri[1] = stale<esvio_fe_aedat_info>();                                                  \
    TI(esvio_fe_track_aedat(h, L.data(), L.size(), R.data(), R.size(), 0, flags, pub, filter, motion, &o.t, &bi, ri));                \
    show(bi), show(ri[0]), show(ri[1]);                                                                                               \
  } while (0)
  const std::vector<uint8_t> none;
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 0, 1, nullptr, nullptr);
  BOTH(10, 9, 0, 0);
  TRK(ch, none, 0, 0, nullptr, nullptr);
  BOTH(10, 9, 0, 0);
  TRK(none, ch, 0, 1, nullptr, nullptr);
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 1u, 1, nullptr, &mo);
  notef(".. with a filter");
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 0, 1, &flt, nullptr);
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 1u, 0, &flt, &mo);
  notef(".. bad stamps on the right camera only; a malformed right chunk; no left event");
  BOTH(2900, 9, 0, 3);
  TRK(big, ch, 0, 1, nullptr, nullptr);
  TRK(big, malformed, 0, 1, nullptr, nullptr);
  BOTH(0, 9, 0, 0);
  TRK(ch, ch, 0, 1, nullptr, nullptr);
  TRK(other, other, 0, 1, nullptr, nullptr);
  TRK(cut, ch, 0, 1, nullptr, nullptr);
  notef(".. the filter's body fails: the walkers stay (the next call completes the cut record once more)");
  hipstub_set_baf(1, 0, 1);
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 0, 1, &flt, nullptr);
  hipstub_set_baf(0, 0, 0);
  TI(esvio_fe_filter_reset(h));
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 0, 1, &flt, nullptr);
  notef(".. refused: nothing to decode, a batch announced");
  TRK(none, none, 0, 1, nullptr, nullptr);
  Batch b;
  make_batch(b, W, H, 0, 3000);
  TI(esvio_fe_set_next_batch(h, b.t, b.L.data(), b.L.size(), b.R.data(), b.R.size(), ESVIO_FE_HOST, 1));
  TRK(big, ch, 0, 1, nullptr, nullptr);
  TI(esvio_fe_reset(h));
  BOTH(2900, 9, 0, 0);
  TRK(big, ch, 0, 1, nullptr, nullptr);
  TI(esvio_fe_reserve(h, 1u << 16, 1u << 16, 1));
#undef TRK
  trace_destroy(h, esvio_fe_ingest_kernel_count());
}

static void ingest_bag(const esvio_fe_config& c, int W, int H) {
  esvio_fe_handle h = trace_create("esvio_fe_decode_bag", c, W, H);
  if (!h) return;
  const esvio_fe_bag_topics topics{"/l", "/r", nullptr};
  TI(esvio_fe_bag_set_topics(h, &topics));
  std::vector<esvio_fe_event> dl(4000), dr(4000);
  std::vector<esvio_fe_bag_message> msgs(8);
  esvio_fe_event* dst[2] = {dl.data(), dr.data()};
  uint32_t seq = 0, th = 400;
  esvio_fe_bag_info bi;
#define BAG(nL, nR, capL, capR, dspace, mcap)                                                                                 \
  do {                                                                                                                        \
    const std::vector<uint8_t> ch = bag_chunk(nL, nR, ++seq);                                                                 \
    const size_t cap[2] = {capL, capR};                                                                                       \
    bi = stale<esvio_fe_bag_info>();                                                                                          \
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 0, dst, cap, dspace, msgs.data(), mcap, &bi));                            \
    show(bi);                                                                                                                 \
  } while (0)
  BOTH(0, 0, 0, 0);
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  BOTH(0, 0, 0, 0);
  BAG(1500, 5, dl.size(), dr.size(), ESVIO_FE_DEVICE, msgs.size());
  BOTH(0, 0, 0, 0);
  BAG(6, 0, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  BOTH(0, 0, 0, 0);
  BAG(0, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  notef(".. refused: no room, no room for the messages, bad stamps; a success behind each");
  BOTH(0, 0, 0, 0);
  BAG(6, 5, dl.size(), (size_t)4, ESVIO_FE_HOST, msgs.size());
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, (size_t)1);
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  BOTH(0, 0, 2, 0);
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  BOTH(0, 0, 0, 0);
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  notef(".. ahead of the argument checks");
  {
    const std::vector<uint8_t> ch = bag_chunk(6, 5, ++seq);
    const size_t cap[2] = {dl.size(), dr.size()};
    esvio_fe_event* odd[2] = {dl.data(), (esvio_fe_event*)((char*)dr.data() + 8)};
    esvio_fe_event* null_right[2] = {dl.data(), nullptr};
    bi = stale<esvio_fe_bag_info>();
    TI(esvio_fe_decode_bag(h, ch.data(), 0, 0, dst, cap, ESVIO_FE_HOST, msgs.data(), msgs.size(), &bi));
    show(bi);
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 0, odd, cap, ESVIO_FE_DEVICE, msgs.data(), msgs.size(), &bi));
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 0, null_right, cap, ESVIO_FE_HOST, msgs.data(), msgs.size(), &bi));
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 1, dst, cap, ESVIO_FE_HOST, msgs.data(), msgs.size(), &bi));
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 0, dst, cap, 7, msgs.data(), msgs.size(), &bi));
    TI(esvio_fe_decode_bag(h, ch.data(), ch.size(), 0, dst, cap, ESVIO_FE_HOST, nullptr, 2, &bi));
    std::vector<uint8_t> broken = ch;
    broken[0] = 0xff, broken[1] = 0xff;  // header_len > 4096
    bi = stale<esvio_fe_bag_info>();
    TI(esvio_fe_decode_bag(h, broken.data(), broken.size(), 0, dst, cap, ESVIO_FE_HOST, msgs.data(), msgs.size(), &bi));
    show(bi);
  }
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  TI(esvio_fe_decode_reset(h));
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  TI(esvio_fe_reset(h));
  BAG(6, 5, dl.size(), dr.size(), ESVIO_FE_HOST, msgs.size());
  TI(esvio_fe_reserve(h, 1u << 16, 1u << 16, 1));
#undef BAG
  trace_destroy(h, esvio_fe_ingest_kernel_count());
}

static void ingest_feed(const char* label, const esvio_fe_config& c, int W, int H, const esvio_fe_filter_params* filter) {
  esvio_fe_handle h = trace_create(label, c, W, H);
  if (!h) return;
  TraceOut o(c.max_cnt);
  const esvio_fe_bag_topics topics{"/l", "/r", nullptr};
  TI(esvio_fe_bag_set_topics(h, &topics));
  esvio_fe_slice_params prm;
  std::memset(&prm, 0, sizeof prm);
  prm.frequency = 1000.0;
  const size_t nb = (size_t)esvio_fe_raw_tile_bytes() + 8;
  std::vector<uint8_t> words(nb);
  const std::vector<uint8_t> ch = aedat_chunk(2, 5);
  std::vector<uint8_t> malformed = aedat_chunk(1, 5);
  malformed[4] = 9;
  Batch b;
  make_batch(b, W, H, 0, 600);
  const int F = ESVIO_FE_RAW_EVT3;
  uint32_t th = 500, seq = 0;
  esvio_fe_feed_info fi, fi2[2];
#define PUSH(call) do { fi = stale<esvio_fe_feed_info>(); TI(call); show(fi); } while (0)
#define PUSH_BAG(nL, nR)                                                                  \
  do {                                                                                    \
    const std::vector<uint8_t> bc = bag_chunk(nL, nR, ++seq);                             \
    fi2[0] = fi2[1] = stale<esvio_fe_feed_info>();                                        \
    TI(esvio_fe_feed_push_bag(h, bc.data(), bc.size(), 0, fi2));                          \
    show(fi2[0]), show(fi2[1]);                                                           \
  } while (0)
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));  // no feed is open
  TI(esvio_fe_feed_open(h, &prm, filter));
  ingest_set(0, 500, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 1, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));  // no left record yet
  BOTH(0, 0, 0, 0);
  PUSH_BAG(0, 5);                                                                  // ... for the bag as well
  ingest_set(0, 500, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  ingest_set(0, 400, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 1, F, words.data(), nb, ESVIO_FE_DEVICE, 0, &fi));
  notef(".. raw: bad stamps, then the emit again");
  ingest_set(0, 500, 4, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  ingest_set(0, 100000, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  PUSH(esvio_fe_feed_push_raw(h, 0, 4, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), 0, ESVIO_FE_HOST, 0, &fi));
  notef(".. AEDAT");
  ingest_set(0, 10, 0, ++th);
  PUSH(esvio_fe_feed_push_aedat(h, 0, ch.data(), ch.size(), 0, 0, &fi));
  ingest_set(0, 10, 0, ++th);
  PUSH(esvio_fe_feed_push_aedat(h, 1, ch.data(), ch.size(), 0, 1u, &fi));
  ingest_set(0, 10, 1, ++th);
  PUSH(esvio_fe_feed_push_aedat(h, 0, ch.data(), ch.size(), 0, 0, &fi));
  PUSH(esvio_fe_feed_push_aedat(h, 0, malformed.data(), malformed.size(), 0, 0, &fi));
  PUSH(esvio_fe_feed_push_aedat(h, 0, ch.data(), ch.size(), 0, 2u, &fi));
  ingest_set(0, 10, 0, ++th);
  PUSH(esvio_fe_feed_push_aedat(h, 0, ch.data(), ch.size(), 0, 0, &fi));
  notef(".. bag chunks");
  BOTH(0, 0, 0, 0);
  PUSH_BAG(6, 5);
  BOTH(0, 0, 0, 1);
  PUSH_BAG(6, 5);
  BOTH(0, 0, 0, 0);
  PUSH_BAG(1500, 0);
  notef(".. records");
  PUSH(esvio_fe_feed_push_events(h, 0, b.L.data(), b.L.size(), ESVIO_FE_HOST, &fi));
  PUSH(esvio_fe_feed_push_events(h, 1, b.R.data(), b.R.size(), ESVIO_FE_DEVICE, &fi));
  PUSH(esvio_fe_feed_push_events(h, 1, (const esvio_fe_event*)((const char*)b.R.data() + 8), 4, ESVIO_FE_DEVICE, &fi));
  PUSH(esvio_fe_feed_push_events(h, 2, b.R.data(), b.R.size(), ESVIO_FE_HOST, &fi));
  esvio_fe_feed_window win;
  TI(esvio_fe_feed_peek(h, &win));
  notef("   feed_window ready %d index %llu end %u.%09u count %llu %llu", win.ready, U(win.index), win.end_sec, win.end_nsec, U(win.count[0]), U(win.count[1]));
  if (filter) {
    notef(".. a bag chunk whose right camera's filter fails behind the left camera's append: the append is undone, the walker stays");
    const std::vector<uint8_t> bc = bag_chunk(6, 5, ++seq);
    const size_t cut = bag_chunk(6, 0, seq).size() - 3 * 13;  // inside the left message: three of its events wait for the next call
    BOTH(0, 0, 0, 0);
    fi2[0] = fi2[1] = stale<esvio_fe_feed_info>();
    TI(esvio_fe_feed_push_bag(h, bc.data(), cut, 0, fi2));
    show(fi2[0]), show(fi2[1]);
    for (int again = 0; again < 2; again++) {
      // first with the second filter launch of the call, the right camera's, reporting its error; then as it is: a walker
      // that had moved would stand behind the chunk, where these bytes begin in the middle of an event
      BOTH(0, 0, 0, 0);
      if (!again) hipstub_set_baf_err_at(2);
      fi2[0] = fi2[1] = stale<esvio_fe_feed_info>();
      TI(esvio_fe_feed_push_bag(h, bc.data() + cut, bc.size() - cut, 0, fi2));
      show(fi2[0]), show(fi2[1]);
      if (!again) TI(esvio_fe_filter_reset(h));
    }
    // the left camera's length: a chunk that does not fit moves its records to the other buffer, one copy of 16 bytes each
    const std::vector<esvio_fe_event> big(200000);
    PUSH(esvio_fe_feed_push_events(h, 0, big.data(), big.size(), ESVIO_FE_HOST, &fi));
  }
  notef(".. the decoders' states over esvio_fe_decode_reset, esvio_fe_reset and esvio_fe_reserve");
  TI(esvio_fe_decode_reset(h));
  ingest_set(0, 500, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  TI(esvio_fe_reset(h));
  ingest_set(0, 500, 0, ++th);
  PUSH(esvio_fe_feed_push_raw(h, 0, F, words.data(), nb, ESVIO_FE_HOST, 0, &fi));
  TI(esvio_fe_reserve(h, 1u << 16, 1u << 16, 1));
  BOTH(0, 0, 0, 0);
  PUSH_BAG(6, 5);
  TI(esvio_fe_feed_close(h));
#undef PUSH
#undef PUSH_BAG
  trace_destroy(h, esvio_fe_ingest_kernel_count());
}

static int trace_ingest_matrix(esvio_fe_config c) {
  setenv("ESVIO_FE_STAGE_THREADS", "0", 1);
  hipstub_arm_faults(0);
  hipstub_set_compact_total(1000);
  const int W = 346, H = 260;
  ingest_decode_raw(c, W, H);
  ingest_track_raw(c, W, H);
  ingest_aedat(c, W, H);
  ingest_bag(c, W, H);
  ingest_feed("the feed", c, W, H, nullptr);
  const esvio_fe_filter_params flt{1000000, 1, 0, 0};
  ingest_feed("the feed with a filter", c, W, H, &flt);
  return trace_finish("trace_ingest");
}
#undef BOTH
#undef U
#undef TI


int main(int argc, char** argv) {
  const bool trace_mode = argc > 1 && !strcmp(argv[1], "trace");
  const bool trace_cand_mode = argc > 1 && !strcmp(argv[1], "trace_cand");
  rs = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
  const int frames = argc > 2 ? atoi(argv[2]) : 200;
  const int W = 640, H = 480, M = 120;
  esvio_fe_config c;
  std::memset(&c, 0, sizeof(c));
  c.width = W; c.height = H; c.decay_ms = 20; c.feature_filter_threshold = 0.01; c.ts_lk_threshold = 128;
  c.max_cnt = M; c.min_dist = 10; c.flow_back = 1; c.f_threshold = 1.0; c.f_ransac = 1; c.lk_accum = 1;
  c.focal_length = 460; c.device = -1;
  for (int k = 0; k < 2; k++) { c.cam[k].fx = c.cam[k].fy = 0.9 * W; c.cam[k].cx = W / 2.0; c.cam[k].cy = H / 2.0; }
  if (trace_mode) return trace_matrix(c);
  if (trace_cand_mode) return trace_cand_matrix(c);
  if (argc > 1 && !strcmp(argv[1], "trace_ingest")) return trace_ingest_matrix(c);
  std::vector<int32_t> ids(M), cnt(M), idr(M);
  std::vector<float> f2[6];
  for (auto& v : f2) v.resize(2 * M);
  esvio_fe_tracks t;
  std::memset(&t, 0, sizeof(t));
  t.ids = ids.data(); t.track_cnt = cnt.data(); t.cur_pts = f2[0].data(); t.cur_un_pts = f2[1].data();
  t.pts_velocity = f2[2].data(); t.ids_right = idr.data(); t.cur_right_pts = f2[3].data();
  t.cur_un_right_pts = f2[4].data(); t.right_pts_velocity = f2[5].data();
  long calls = 0, failed = 0, resets = 0, handles = 0;
  uint64_t staged[4] = {0, 0, 0, 0};  // esvio_fe_staging_counters, summed over the handles
  int f = 0;
  {  // (the injected failures are for the calls of the loop below)
    hipstub_arm_faults(0);
    int bad = 0;
    esvio_fe_config e = c;
    e.equalize = 1;
    e.median_blur_kernel_size = 1;
    bad += first_use_pass(e, W, H, true);
    setenv("ESVIO_FE_SAE_SORT", "1", 1);       // the radix-sort form of the SAE update ...
    setenv("ESVIO_FE_STAGE_THREADS", "0", 1);  // ... and host batches without the staging slots (the lanes' own buffers)
    bad += first_use_pass(c, W, H, false);
    unsetenv("ESVIO_FE_SAE_SORT");
    unsetenv("ESVIO_FE_STAGE_THREADS");
    bad += first_use_pass(c, 1920, 1200, true);  // a sensor whose selection bitmap does not fit LDS: the one in device memory
    hipstub_arm_faults(1);
    if (bad) { fprintf(stderr, "first_use_pass: %d calls failed\n", bad); return 5; }
  }
  while (f < frames) {
    esvio_fe_handle h = nullptr;
    // (both LK modes, and the batches handed over as host or as "device" memory — the stub's device memory is the
    // host's: with the launch thread on, the float-order mode and device batches the handle takes its second stereo
    // stream and the chained launch's device-side gate, fe_track.cpp)
    const bool split_case = handles == 0;  // (the first handle of a run: exactly that configuration, from its first frame)
    c.lk_accum = split_case ? 2 : 1 + (int)(rnd() & 1u);
    const int space = split_case ? ESVIO_FE_DEVICE : (rnd() & 1u) ? ESVIO_FE_HOST : ESVIO_FE_DEVICE;
    // (HIPSTUB_FAIL_EVERY: the injected failures are for the calls; a creation — whose warm-up alone records 384
    // events and checks every return code — is let through)
    hipstub_arm_faults(0);
    const int crc = esvio_fe_create(&c, &h);
    hipstub_arm_faults(1);
    if (crc != ESVIO_FE_OK) { fprintf(stderr, "create failed\n"); return 3; }
    handles++;
    esvio_fe_reserve(h, 1u << 16, 1u << 16, 1);
    const int stretch = 20 + (int)(rnd() % 40u);  // frames on this handle
    std::vector<Batch> bs((size_t)stretch);
    for (int i = 0; i < stretch; i++) {
      Batch& b = bs[(size_t)i];
      make_batch(b, W, H, f + i, 9000 + (int)(rnd() % 6000u));
      // about one batch in four: the second half of the left array one second earlier — a plain call's staging then meets
      // a chunk whose stamps step back over a second, which it must send raw and never write packed (fe_evstage.cpp)
      if (rnd() % 4u == 0)
        for (size_t j = b.L.size() / 2; j < b.L.size(); j++) b.L[j].sec -= 1;
    }
    std::vector<int> pub((size_t)stretch);
    for (int i = 0; i < stretch; i++) pub[(size_t)i] = (rnd() % 3u) != 0;
    int announced = 0;                                 // batches [i + 1, announced] are announced
    bool replay = split_case || (rnd() & 1u) != 0;
    if (split_case) {
      esvio_fe_set_launch_thread(h, 1);
      esvio_fe_set_lazy_new_stereo(h, 1);
    }
    for (int i = 0; i < stretch; i++) {
      if (rnd() % 7u == 0) esvio_fe_set_launch_thread(h, (int)(rnd() & 1u));
      if (rnd() % 9u == 0) esvio_fe_set_host_threads(h, (int)(rnd() % 8u));
      if (rnd() % 11u == 0) esvio_fe_set_lazy_new_stereo(h, (int)(rnd() & 1u));
      if (rnd() % 13u == 0) replay = !replay;
      if (rnd() % 29u == 0) {  // a clean slate in the middle of the stream, whatever is announced or in flight
        esvio_fe_reset(h);
        resets++;
        announced = i;
      }
      if (announced < i) announced = i;
      if (replay) {
        const int ahead = 1 + (int)(rnd() % 4u);
        while (announced < i + ahead && announced + 1 < stretch) {
          announced++;
          const Batch& n = bs[(size_t)announced];
          int hint = pub[(size_t)announced];
          if (rnd() % 41u == 0) hint = 0;  // (a wrong hint: with more than one batch ahead the call for it is refused)
          esvio_fe_set_next_batch(h, n.t, n.L.data(), n.L.size(), n.R.data(), n.R.size(), space, hint);
        }
      }
      const Batch& b = bs[(size_t)i];
      const int rc = esvio_fe_track_event(h, b.t, b.L.data(), b.L.size(), b.R.data(), b.R.size(), space,
                                          pub[(size_t)i], &t);
      calls++;
      if (rc != ESVIO_FE_OK) {  // refused (wrong hint) or failed: the handle must be usable after a reset
        failed++;
        esvio_fe_reset(h);
        announced = i;
      } else {
        fold_tracks(t);
        if (!latency_record_ok(h, pub[(size_t)i])) return 4;
      }
      if (rnd() % 17u == 0 && esvio_fe_finish(h, &t) == ESVIO_FE_OK) fold_tracks(t);
    }
    if (esvio_fe_finish(h, &t) == ESVIO_FE_OK) fold_tracks(t);
    {
      esvio_fe_latency_call lc;
      if (esvio_fe_latency_recent(h, 0, &lc) == ESVIO_FE_OK && lc.ms < 0) { fprintf(stderr, "latency record\n"); return 4; }
      uint64_t sc[4];
      if (esvio_fe_staging_counters(h, sc) == ESVIO_FE_OK)
        for (int k = 0; k < 4; k++) staged[k] += sc[k];
    }
    esvio_fe_destroy(h);
    f += stretch;
  }
  uint64_t tail[6];
  esvio_fe_ransac_tail(tail, 0);
  printf("drive ok: %ld calls on %ld handles, %ld refused/failed, %ld resets, tracks last %d / %d, ransac redone %llu\n", calls,
         handles, failed, resets, t.n_left, t.n_right, (unsigned long long)tail[2]);
  printf("staging: %llu batches, %llu chunks packed, %llu raw\n", (unsigned long long)staged[0], (unsigned long long)staged[2],
         (unsigned long long)staged[3]);
  long live[4];
  hipstub_live(live);
  printf("live: device %ld pinned %ld events %ld streams %ld\n", live[0], live[1], live[2], live[3]);
  printf("digest: %016llx\n", (unsigned long long)digest);
  return 0;
}
