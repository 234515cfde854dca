// The few "kernels" of the ThreadSanitizer build that do something (tests/hipstub): enough for the host side to have
// real work — corners appear, LK moves them a little, so tracks live on and rejectWithF_event runs its RANSAC on
// the helper pool every published frame — and the staged events are really read where the device would read them.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "fe_kernels.h"

namespace esvio {
namespace {
uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
}  // namespace

// H2D of staged events by a kernel: the pinned buffer the staging threads filled is READ here
void launch_stage_pull(hipStream_t s, const void* pinned_src, void* dst, size_t bytes) {
  hipstub_trace("launch_stage_pull", s);
  hipstub_stream_begin(s);
  std::memcpy(dst, pinned_src, bytes);
  hipstub_stream_end(s);
}

// ... of packed chunks (fe_evstage.cpp stage_pack): unpacked here as k_stage_pull_packed does
void launch_stage_pull_packed(hipStream_t s, const void* pinned_src, void* dst, size_t bytes, const void* desc, uint32_t epc) {
  hipstub_trace("launch_stage_pull_packed", s);
  hipstub_stream_begin(s);
  const uint32_t* d = (const uint32_t*)desc;
  const uint8_t* src = (const uint8_t*)pinned_src;
  uint32_t* out = (uint32_t*)dst;
  for (size_t i = 0; i < bytes / 16; i++) {
    const size_t c = i / epc, j = i - c * epc;
    const uint8_t* base = src + c * (size_t)epc * 16;
    if (d[2 * c + 1]) {
      uint32_t v[2];
      std::memcpy(v, base + 8 * j, 8);
      out[4 * i] = v[0];
      out[4 * i + 1] = d[2 * c] + (v[1] >> 31);
      out[4 * i + 2] = v[1] & 0x3fffffffu;
      out[4 * i + 3] = (v[1] >> 30) & 1u;
    } else {
      std::memcpy(out + 4 * i, base + 16 * j, 16);
    }
  }
  hipstub_stream_end(s);
}

// (drive trace: goodFeaturesToTrack sorts its candidates only if there are at least two)
static uint32_t g_compact_total = 0;
extern "C" void hipstub_set_compact_total(uint32_t n) { g_compact_total = n; }

void launch_compact(hipStream_t s, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*,
                    uint32_t* total, uint32_t*) {
  hipstub_trace("launch_compact", s);
  hipstub_stream_begin(s);
  if (total) *total = g_compact_total;
  hipstub_stream_end(s);
}

// Event_FeaturesToTrack: fills the free places with corners on a jittered grid (deterministic)
KernelId launch_select(hipStream_t s, const SelectArgs& a, size_t) {
  hipstub_trace("launch_select", s);
  hipstub_stream_begin(s);
  static uint32_t seed = 12345;
  const int want = a.max_corners > 0 ? a.max_corners : 0;
  int k = 0;
  for (; k < want; k++) {
    const float x = 8.f + (float)(lcg(seed) % (uint32_t)(a.W - 16)), y = 8.f + (float)(lcg(seed) % (uint32_t)(a.H - 16));
    a.out_pts[a.out_base + k] = make_float2(x, y);
    if (a.out_idx) a.out_idx[a.out_base + k] = k;
    if (a.pub_slots)
      a.pub_slots[a.out_base + k] = ((unsigned long long)a.pub_seq << 32) | ((unsigned long long)(uint32_t)y << 16) | (uint32_t)x;
  }
  if (a.n_out) *a.n_out = k;
  if (a.n_total) *a.n_total = a.out_base + k;
  if (a.host_counts) {
    a.host_counts[0] = k;
    a.host_counts[1] = a.out_base + k;
    a.host_counts[2] = k;
  }
  if (a.pub_done) *a.pub_done = ((unsigned long long)a.pub_seq << 32) | (uint32_t)(a.out_base + k);
  hipstub_stream_end(s);
  return K_SELECT_MW;
}

// calcOpticalFlowPyrLK forward (+ backward): every point found, moved by a fraction of a pixel that depends on the
// point (so that the epipolar geometry is not degenerate), the backward pass lands on the start
void launch_lk(hipStream_t s, const LkArgs& f, const LkArgs* b, float2* back_pts, uint8_t* back_status) {
  hipstub_trace("launch_lk", s);
  hipstub_stream_begin(s);
  const int n = f.n_ptr ? *f.n_ptr : f.n_max;
  for (int i = 0; i < n && i < f.n_max; i++) {
    float2 p = f.prev_pts ? f.prev_pts[i] : make_float2(0.f, 0.f);
    if (f.chain_in) {  // the previous launch's forward result
      const unsigned long long vx = f.chain_in[2 * i], vy = f.chain_in[2 * i + 1];
      uint32_t ux = (uint32_t)vx, uy = (uint32_t)vy;
      std::memcpy(&p.x, &ux, 4);
      std::memcpy(&p.y, &uy, 4);
    } else if (f.poll_slots && i >= f.poll_from) {
      const unsigned long long v = f.poll_slots[i];
      p = make_float2((float)(uint32_t)(v & 0xffffu), (float)(uint32_t)((v >> 16) & 0xffffu));
    }
    const float2 q = make_float2(p.x + 0.25f + 0.001f * (float)(i % 37), p.y - 0.125f + 0.002f * (float)(i % 11));
    f.next_pts[i] = q;
    f.status[i] = 1;
    if (f.chain_out) {
      uint32_t ux, uy;
      std::memcpy(&ux, &q.x, 4);
      std::memcpy(&uy, &q.y, 4);
      const unsigned long long hi = (unsigned long long)((f.chain_seq << 2) | 1u) << 32;
      f.chain_out[2 * i] = hi | ux;
      f.chain_out[2 * i + 1] = hi | uy;
    }
    if (b && back_pts) {
      back_pts[i] = p;
      back_status[i] = 1;
    }
  }
  hipstub_stream_end(s);
}

// ---- drive trace_ingest: the decode chains' result blocks.  The stub launchers leave a result block as the host zeroed
// it, so no refusal and no repeated emit would ever be walked: the driver sets, per job slot k of a call (0: the call's
// only or left camera, 1: its right one), what the next emit launches report (hipstub_set_ingest), and every launcher
// here writes what it was handed into the trace — the carried decoder state as the seed, the chunk, the room — so that a
// state that moved when it should not have, or did not when it should have, shows in the next call's lines.
namespace {
struct IngestPreset {
  uint32_t events, untimed;
  unsigned long long bad;
  long long first_t, last_t;
  uint32_t st_th, st_flags, st_bx, st_wraps;  // the raw chain's state behind the call
};
IngestPreset g_ingest[2];
struct BafPreset {
  int on, err;
  uint32_t kept;
  int err_at;  // > 0: the err_at-th launch from now reports err, whatever `on` says (the ones in front of it are as they were)
} g_baf;
void note(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void note(const char* fmt, ...) {
  char buf[320];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  hipstub_trace_note(buf);
}
void raw_note(const char* what, const RawArgs& a) {
  for (int k = 0; k < 2; k++) {
    const RawCam& c = a.cam[k];
    if (!c.tiles) continue;
    note("  %s[%d] format %d n_bytes %u tiles %u seed th %u flags 0x%x bx %u wraps_base %llu t_offset %lld dst %s dst_cap %u res %s", what, k,
         a.format, c.n_bytes, c.tiles, c.seed.th_last, c.seed.flags, c.seed.bx, c.wraps_base, c.t_offset, c.dst ? "set" : "null", c.dst_cap,
         c.res == a.cam[0].res ? "0" : "+");
  }
}
void raw_emit(const char* what, hipStream_t s, const RawArgs& a) {
  hipstub_trace(what, s);
  hipstub_stream_begin(s);
  raw_note(what, a);
  for (int k = 0; k < 2; k++) {
    if (!a.cam[k].tiles) continue;
    const IngestPreset& p = g_ingest[k];
    RawResult r{};
    r.events = p.events, r.untimed = p.untimed, r.wraps = p.st_wraps, r.bad = p.bad, r.first_t = p.first_t, r.last_t = p.last_t;
    r.state = RawXf{p.st_th, p.st_th, p.st_wraps, p.st_flags, p.st_bx, 0, 0, 0};
    *a.cam[k].res = r;
  }
  hipstub_stream_end(s);
}
}  // namespace
extern "C" void hipstub_set_ingest(int k, uint32_t events, uint32_t untimed, unsigned long long bad, long long first_t, long long last_t,
                                   uint32_t st_th, uint32_t st_flags, uint32_t st_bx, uint32_t st_wraps) {
  g_ingest[k & 1] = IngestPreset{events, untimed, bad, first_t, last_t, st_th, st_flags, st_bx, st_wraps};
}
// the filter's last launch: on = 0 keeps every record (what the launch does until the driver says otherwise)
extern "C" void hipstub_set_baf(int on, uint32_t kept, int err) { g_baf = BafPreset{on, err, kept, 0}; }
// ... or only its nth launch from now: one camera's chain of a call that runs both
extern "C" void hipstub_set_baf_err_at(int nth) { g_baf.err_at = nth; }

void launch_raw_reduce(hipStream_t s, const RawArgs& a) {
  hipstub_trace("launch_raw_reduce", s);
  hipstub_stream_begin(s);
  raw_note("launch_raw_reduce", a);
  hipstub_stream_end(s);
}
void launch_raw_emit(hipStream_t s, const RawArgs& a) { raw_emit("launch_raw_emit", s, a); }
void launch_trig_emit(hipStream_t s, const RawArgs& a) { raw_emit("launch_trig_emit", s, a); }

void launch_aedat_emit(hipStream_t s, const AedatArgs& a) {
  hipstub_trace("launch_aedat_emit", s);
  hipstub_stream_begin(s);
  for (int k = 0; k < 2; k++) {
    const AedatCam& c = a.cam[k];
    if (!c.tiles) continue;
    note("  launch_aedat_emit[%d] n %u tiles %u n_runs %u keep_invalid %u t_offset %lld dst %s dst_cap %u", k, c.n, c.tiles, c.n_runs,
         c.keep_invalid, c.t_offset, c.dst ? "set" : "null", c.dst_cap);
    const IngestPreset& p = g_ingest[k];
    AedatResult r{};
    r.events = p.events, r.invalid = p.untimed, r.bad = p.bad, r.first_t = (unsigned long long)p.first_t, r.last_t = (unsigned long long)p.last_t;
    *c.res = r;
  }
  hipstub_stream_end(s);
}

void launch_bag_emit(hipStream_t s, const BagArgs& a) {
  hipstub_trace("launch_bag_emit", s);
  hipstub_stream_begin(s);
  for (int k = 0; k < 2; k++) {
    const BagCam& c = a.cam[k];
    if (!c.tiles) continue;
    note("  launch_bag_emit[%d] n %u tiles %u dst %s dst_cap %u", k, c.n, c.tiles, c.dst ? "set" : "null", c.dst_cap);
    const IngestPreset& p = g_ingest[k];
    BagResult r{};
    r.bad = p.bad;
    r.first_sec = (uint32_t)(p.first_t / 1000000000), r.first_nsec = (uint32_t)(p.first_t % 1000000000);
    r.last_sec = (uint32_t)(p.last_t / 1000000000), r.last_nsec = (uint32_t)(p.last_t % 1000000000);
    *c.res = r;
  }
  hipstub_stream_end(s);
}

void launch_baf_emit(hipStream_t s, const BafArgs& a) {
  hipstub_trace("launch_baf_emit", s);
  hipstub_stream_begin(s);
  const bool hit = g_baf.err_at > 0 && --g_baf.err_at == 0;
  a.res->n_kept = hit ? 0 : g_baf.on ? g_baf.kept : a.n;
  a.res->err = hit ? 1 : g_baf.on ? g_baf.err : 0;
  a.res->last = EventRec{};
  a.res->last.sec = 1700000000u, a.res->last.nsec = 5000u;
  hipstub_stream_end(s);
}

}  // namespace esvio
