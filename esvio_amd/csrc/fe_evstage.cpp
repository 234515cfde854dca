// fe_evstage.cpp — host-resident event batches (ESVIO_FE_HOST, what the reference's
// `const dvs_msgs::EventArray&` interface hands over: feature_tracker/src/feature_tracker.h:51-52)
// on their way to the device.
//
// A hipMemcpyAsync from pageable memory is not asynchronous: the runtime stages it through its own
// bounce buffers on the calling thread (measured: 15 GB/s, 0.35 ms for the 5.3 MB of a C3 batch —
// almost three times the rest of the frame).  Here the batch is cut into chunks of 256 KiB (64 KiB when
// the calling thread waits for it); helper threads copy them into pinned memory with streaming stores and,
// when the last chunk of a group is in, send the group to the device on a copy stream of its own: an
// announced batch (esvio_fe_set_next_batch: all of it happens while the previous frames are tracked) as ONE
// DMA; a plain call's batch in a few groups, each pulled out of the pinned buffer by a small kernel
// (k_stage_pull) under the memcpy of the next one — lower latency than a copy engine at these sizes, and
// several DMAs in flight at once make the runtime bring up further copy engines in the middle of a stream
// (7-9 ms inside whichever hipMemcpyAsync does it, measured round 4; with more engines up the same calls
// then run 0.08 ms slower).  The compute streams only wait for an event.
// A source that already is pinned (hipHostMalloc / hipHostRegister) skips the memcpy: one DMA.
//
// Slots: one pinned + one device buffer per batch the handle knows about (announced, prefetched or
// being tracked).  A slot's device buffer is overwritten only after the kernels that read its
// previous batch (SAE update / Arc* on the prefetch stream, Arc* on the main stream) are done: the
// copy stream waits for the events recorded behind them.
#include "fe_internal.h"

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
#include <emmintrin.h>
#define ESVIO_STAGE_NT 1
#endif

namespace esvio {
namespace fe {

namespace {
// pageable source -> pinned chunk.  The destination is read next by the DMA engine, never by this core: streaming
// stores (no read-for-ownership of the destination lines, no cache filled with them); dst is 16-byte aligned (the
// slot is page-aligned, offsets are multiples of the 16-byte event record)
inline void stage_copy(uint8_t* dst, const uint8_t* src, size_t len) {
#ifdef ESVIO_STAGE_NT
  if (((uintptr_t)dst & 15u) == 0) {
    size_t i = 0;
    for (; i + 64 <= len; i += 64) {
      const __m128i a = _mm_loadu_si128((const __m128i*)(src + i)), b = _mm_loadu_si128((const __m128i*)(src + i + 16)),
                    c = _mm_loadu_si128((const __m128i*)(src + i + 32)), d = _mm_loadu_si128((const __m128i*)(src + i + 48));
      _mm_stream_si128((__m128i*)(dst + i), a);
      _mm_stream_si128((__m128i*)(dst + i + 16), b);
      _mm_stream_si128((__m128i*)(dst + i + 32), c);
      _mm_stream_si128((__m128i*)(dst + i + 48), d);
    }
    if (i < len) std::memcpy(dst + i, src + i, len - i);
    _mm_sfence();  // (before the chunk is marked done and its group's DMA enqueued)
    return;
  }
#endif
  std::memcpy(dst, src, len);
}

// nanoseconds since t0, as the stager's counters keep them; NsScope adds a scope's to one (cf. PhaseClock, fe_ctx.h)
using Clock = std::chrono::steady_clock;
inline uint64_t ns_since(Clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count(); }
struct NsScope {
  uint64_t& sum;
  Clock::time_point t0 = Clock::now();
  ~NsScope() { sum += ns_since(t0); }
};

// The same chunk as 8 bytes per event, when its events allow it: x | y << 16 as they are, nsec (30 bits) | polarity
// (!= 0, as every kernel reads it) << 30 | (sec - base) << 31 with base = the chunk's first event's second — so a
// chunk may cross ONE second boundary forwards; anything else (stamps going backwards across a second, nsec >= 2^30)
// and the caller copies the chunk raw instead.
// Whether the n events at src allow it.  Reads only: the OR over the records of their 32-bit lanes — x | y << 16,
// sec - base, nsec, polarity byte | padding — says it all
inline bool stage_packable(const uint8_t* src, size_t n, uint32_t base) {
  uint32_t acc[4] = {0, 0, 0, 0};
#ifdef ESVIO_STAGE_NT
  const __m128i b = _mm_set_epi32(0, 0, (int)base, 0);
  __m128i v = _mm_setzero_si128();
  for (size_t i = 0; i < n; i++) v = _mm_or_si128(v, _mm_sub_epi32(_mm_loadu_si128((const __m128i*)(src + 16 * i)), b));
  _mm_storeu_si128((__m128i*)acc, v);
#else
  for (size_t i = 0; i < n; i++) {
    uint32_t r[4];
    std::memcpy(r, src + 16 * i, 16);
    acc[1] |= r[1] - base;
    acc[2] |= r[2];
  }
#endif
  return ((acc[1] >> 1) | (acc[2] >> 30)) == 0;
}
// Decides first, writes afterwards: returns whether the packed form was written (dst: the first len / 2 bytes of the
// chunk's place in the pinned buffer) — a refused chunk leaves dst as it was.  *base_sec: the second the offsets count from.
inline bool stage_pack(uint8_t* dst, const uint8_t* src, size_t len, uint32_t* base_sec) {
  const size_t n = len / 16;
  if (!n || (len & 15u) || ((uintptr_t)dst & 15u)) return false;
  uint32_t base;
  std::memcpy(&base, src + 4, 4);
  *base_sec = base;
  if (!stage_packable(src, n, base)) return false;
  size_t i = 0;
  auto pack1 = [&](const uint8_t* p) -> uint64_t {
    uint64_t a, b;  // a = x | y << 16 | sec << 32;  b = nsec | polarity byte << 32 | padding
    std::memcpy(&a, p, 8);
    std::memcpy(&b, p + 8, 8);
    const uint32_t hi = (uint32_t)b | (((b >> 32) & 0xffu) ? 1u << 30 : 0u) | (((uint32_t)(a >> 32) - base) << 31);
    return (a & 0xffffffffull) | ((uint64_t)hi << 32);
  };
#ifdef ESVIO_STAGE_NT
  for (; i + 2 <= n; i += 2) {
    const uint64_t lo = pack1(src + 16 * i), hi = pack1(src + 16 * i + 16);
    _mm_stream_si128((__m128i*)(dst + 8 * i), _mm_set_epi64x((long long)hi, (long long)lo));
  }
  _mm_sfence();
#endif
  for (; i < n; i++) {
    const uint64_t v = pack1(src + 16 * i);
    std::memcpy(dst + 8 * i, &v, 8);
  }
  return true;
}
constexpr size_t kChunkBytes = 256 * 1024;
constexpr int kMaxGroups = 8;
// (by camera the calling thread waits for the left array: smaller pieces, more threads on it at once)
inline size_t chunk_bytes(bool by_camera) { return by_camera ? kChunkBytes / 4 : kChunkBytes; }

struct Group {
  size_t off = 0, len = 0;  // byte range of the slot's buffers that one DMA moves
  uint32_t first_chunk = 0; // its first chunk (Slot::chunk / Slot::desc index)
  std::atomic<uint32_t> chunks_left{0};
  std::atomic<bool> dma_enq{false};  // the group's DMA has been enqueued (at least once)
};

// one memcpy into a slot's pinned buffer.  Whoever moves it from TAKEN to DONE accounts for the chunk (a helper, or
// the calling thread redoing the copy of a helper that went away)
enum ChunkState : uint8_t { CH_FREE, CH_TAKEN, CH_DONE };
struct Chunk {
  int group = 0;
  const uint8_t* src = nullptr;
  size_t off = 0, len = 0;  // byte offset inside the slot's buffers
  std::atomic<uint8_t> st{CH_FREE};
};

enum SlotState : int { SL_FAILED = -1, SL_IDLE, SL_STAGING, SL_SENT };  // SENT: every DMA enqueued and `copied` recorded
struct Slot {
  std::unique_ptr<Chunk[]> chunk;
  size_t chunk_cap = 0;
  std::atomic<uint32_t> n_chunks{0};  // of the batch being staged
  std::atomic<uint32_t> next{0};      // the next chunk nobody has taken (>= n_chunks: none left)
  int n_groups = 0;
  PinBuf<uint8_t> pin;   // [16 * cap]
  DevBuf<EventRec> dev;  // [cap]
  size_t cap = 0;  // events, of both (slot_capacity)
  Event copied, pf_done, main_done, aux_done;
  bool pf_rec = false, main_rec = false, aux_rec = false;
  // by_camera staging (a plain call that starts on the left camera while the right one is still on its
  // way): the left array is a DMA of its own, `copiedL` is recorded behind it
  Event copiedL;
  int n_left_groups = 0;             // groups [0, n_left_groups) are the left array's (0: not by camera, or a pinned source)
  std::atomic<bool> left_enq{false}; // the left array's DMA is enqueued and copiedL recorded
  uint32_t n_left_chunks = 0;        // chunks [0, n_left_chunks) are the left array's (by_camera)
  bool pull = false;                 // the groups go to the device by k_stage_pull instead of by DMA (a plain call's batch)
  // ... with the chunks packed to 8 bytes per event where their events allow it (by_camera staging: chunks of one
  // size, a group = whole chunks of one array): one {base second, packed?} pair per chunk, pinned, read by the kernel
  bool pack = false;
  uint32_t pack_epc = 0;             // events per chunk
  PinBuf<uint32_t> desc;             // {base second, packed?} per chunk
  Clock::time_point t_begin;  // (trace) when stager_begin opened the batch for taking
  bool in_use = false;
  std::atomic<int> state{SL_IDLE};
  Group grp[kMaxGroups];
  std::atomic<uint32_t> groups_left{0};
  std::atomic<int> busy{0};  // threads inside this slot's chunks (or about to take one)
  bool staging() const { return state.load(std::memory_order_acquire) == SL_STAGING; }
};
}  // namespace

// Work is handed out without a lock (a thread that loses its CPU while holding one would stop every other thread for a
// scheduler quantum: profiles/r04_stall_forensics.md): a slot's chunks are numbered, `next` is an atomic counter.
// Everything a thread does for a chunk may be done twice, so the calling thread, when it waits for a batch (wait_for),
// finishes whatever a helper has started and not finished instead of waiting for that helper.  What makes twice
// harmless: a chunk's bytes in the pinned buffer and its descriptor are functions of the caller's events alone, and
// packed or raw is settled from the source BEFORE a byte is written (stage_pack) — so every thread that writes a place
// writes the bytes that are published, and a transfer that reads it meanwhile reads those bytes whoever stored them; a
// group's DMA moves the same bytes again; `copied` recorded again only moves the event later.  The counters are NOT
// idempotent: they belong to the one thread that moves a chunk from TAKEN to DONE.
// (the members release themselves, fe_res.h; stager_destroy deletes the stager once its threads have stopped and its
// stream is idle, so their order carries no dependency)
struct EventStager {
  esvio_fe_ctx* c = nullptr;
  Stream stream;
  Slot slot[kStageSlots];
  std::vector<std::thread> threads;
  std::mutex mu;  // (only the sleeping helpers' condition variable)
  std::condition_variable cv;
  std::atomic<int>* pending = nullptr;  // -> esvio_fe_ctx::stage_pending: chunks nobody has taken yet, all slots
  std::atomic<bool> stop{false};
  // (ESVIO_FE_TRACE) batches, bytes, time the calling thread waited for a batch's staging, chunks it
  // took itself meanwhile, batches a call left for the next one because they had not arrived yet
  uint64_t batches = 0, bytes_staged = 0, wait_ns = 0, caller_chunks = 0, skipped = 0, redone = 0;
  // A thread's first HIP calls cost milliseconds (measured: 7 ms inside the call whose DMA a RANSAC helper
  // was the first to enqueue): every thread that may enqueue a DMA does one dummy copy + event record on the
  // copy stream before it takes its first chunk
  Event gate_ev[4];                    // behind the last four DMAs
  std::atomic<uint32_t> gate_n{0}, gate_rec[4];  // DMAs issued; gate_rec[t & 3] == t + 1: DMA t's event is recorded
  std::atomic<uint64_t> gate_expired{0};
  PinBuf<uint8_t> warm_pin;
  DevBuf<uint8_t> warm_dev;
  Event warm_ev;
  void warm_thread() {
    (void)hipSetDevice(c->dev);
    if (warm_pin && warm_dev && hipMemcpyAsync(warm_dev, warm_pin, 16, hipMemcpyHostToDevice, stream) != hipSuccess) (void)hipGetLastError();
    if (warm_ev && hipEventRecord(warm_ev, stream) != hipSuccess) (void)hipGetLastError();
  }
  std::atomic<uint64_t> chunks_packed{0}, chunks_raw{0};  // chunks of packing slots that went out packed / raw (esvio_fe_staging_counters)
  // (trace) time inside stage_chunk, chunks, from a batch's opening to its chunk 0 being taken / its left array's last
  // group / its last group being on its way
  std::atomic<uint64_t> chunk_ns{0}, chunk_cnt{0}, first_take_ns{0}, left_sent_ns{0}, all_sent_ns{0};
  bool pack_enabled = true;  // (ESVIO_FE_STAGE_PACK=0, A/B and tests: every chunk raw)
  uint64_t begin_ns = 0, left_ns = 0, left_calls = 0, pin_ns = 0;  // (trace) by-camera staging: stager_begin, stager_attach_left

  // one DMA on the copy stream.  Never more than two in flight: the third makes the runtime bring up another
  // copy engine inside this very call (7-9 ms) — the stream runs them one after the other anyway, so DMA
  // number t waits (bounded) for number t - 2 to be over
  bool dma(void* dst, const void* src, size_t len) {
    const uint32_t t = gate_n.fetch_add(1, std::memory_order_acq_rel);
    if (t >= 2) {
      const auto tg0 = Clock::now();
      const uint32_t w = (t - 2) & 3u;
      for (unsigned spin = 0;; spin++) {
        if (gate_rec[w].load(std::memory_order_acquire) == t - 1 && hipEventQuery(gate_ev[w]) == hipSuccess) break;
        (void)hipGetLastError();  // (hipErrorNotReady)
        if ((spin & 15) == 15 && Clock::now() - tg0 > std::chrono::microseconds(400)) {
          gate_expired.fetch_add(1, std::memory_order_relaxed);
          break;
        }
        cpu_relax();
      }
    }
    const bool ok = hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, stream) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    if (hipEventRecord(gate_ev[t & 3u], stream) != hipSuccess) (void)hipGetLastError();
    gate_rec[t & 3u].store(t + 1, std::memory_order_release);
    return ok;
  }

  void enqueue_dma(Slot& s, Group& g) {
    if (s.pull) {
      // a batch the calling thread waits for: the device pulls the group out of the pinned buffer itself
      // (k_stage_pull: lower latency than a copy engine, and the copy engines' state stays out of the call)
      (void)hipGetLastError();  // (whatever this thread's earlier calls left behind is not this launch's)
      if (s.pack)
        launch_stage_pull_packed(stream, s.pin + g.off, (uint8_t*)s.dev + g.off, g.len, s.desc + 2 * (size_t)g.first_chunk, s.pack_epc);
      else
        launch_stage_pull(stream, s.pin + g.off, (uint8_t*)s.dev + g.off, g.len);
      if (hipGetLastError() != hipSuccess) s.state.store(SL_FAILED, std::memory_order_release);
    } else {
      // an announced batch, staged whole frames ahead: one DMA (a 5 MB pull kernel on the copy stream costs the
      // compute streams 0.025 ms/step in replay mode, the copy engine nothing)
      if (!dma((uint8_t*)s.dev + g.off, s.pin + g.off, g.len)) s.state.store(SL_FAILED, std::memory_order_release);
    }
    g.dma_enq.store(true, std::memory_order_release);
    if ((int)(&g - s.grp) < s.n_left_groups) {
      // the left array's last DMA to be enqueued (whoever sees them all enqueued; twice does no harm: every
      // DMA whose flag is set is in the stream already)
      bool all = true;
      for (int i = 0; i < s.n_left_groups; i++) all = all && s.grp[i].dma_enq.load(std::memory_order_acquire);
      if (all) {
        if (c->trace) left_sent_ns.fetch_add(ns_since(s.t_begin));
        if (hipEventRecord(s.copiedL, stream) != hipSuccess) s.state.store(SL_FAILED, std::memory_order_release);
        s.left_enq.store(true, std::memory_order_release);
      }
    }
  }
  void finish_batch(Slot& s) {  // every group's DMA is enqueued: the event the compute streams wait for
    if (c->trace) all_sent_ns.fetch_add(ns_since(s.t_begin));
    int expect = SL_STAGING;
    if (hipEventRecord(s.copied, stream) != hipSuccess)
      s.state.store(SL_FAILED, std::memory_order_release);
    else
      (void)s.state.compare_exchange_strong(expect, SL_SENT, std::memory_order_acq_rel);  // (SENT already: a redone batch)
  }

  // the chunk is in the pinned buffer: its group's DMA if it was the group's last, the batch's event if
  // that was the last group
  void chunk_done(Slot& s, const Chunk& ch) {
    Group& g = s.grp[ch.group];
    if (g.chunks_left.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    enqueue_dma(s, g);
    if (s.groups_left.fetch_sub(1, std::memory_order_acq_rel) == 1) finish_batch(s);
  }

  // the chunk's bytes and descriptor into their pinned places — the same ones whoever does it and however often; returns whether packed
  bool stage_chunk(Slot& s, uint32_t idx) {
    const Chunk& ch = s.chunk[idx];
    uint32_t base = 0;
    const bool packed = s.pack && stage_pack(s.pin + ch.off, ch.src, ch.len, &base);
    if (!packed) stage_copy(s.pin + ch.off, ch.src, ch.len);
    if (s.pack) {
      s.desc[2 * idx] = base;
      s.desc[2 * idx + 1] = packed ? 1u : 0u;
    }
    return packed;
  }

  // A TAKEN chunk (this thread's own, or a straggler's being redone) to DONE.  Returns whether this thread is the one
  // that got it there: it counts the chunk and does what follows from its being in (chunk_done)
  bool finish_chunk(Slot& s, uint32_t idx) {
    const auto t0 = c->trace ? Clock::now() : Clock::time_point();
    const bool packed = stage_chunk(s, idx);
    if (c->trace) chunk_ns.fetch_add(ns_since(t0)), chunk_cnt.fetch_add(1);
    Chunk& ch = s.chunk[idx];
    uint8_t taken = CH_TAKEN;
    if (!ch.st.compare_exchange_strong(taken, CH_DONE, std::memory_order_acq_rel)) return false;
    if (s.pack) (packed ? chunks_packed : chunks_raw).fetch_add(1, std::memory_order_relaxed);
    chunk_done(s, ch);
    return true;
  }

  // Take and finish the slot's next chunk if its number is below `upper` (n_chunks: any chunk; n_left_chunks: the
  // calling thread while it waits for the LEFT array — a right-array chunk taken then would keep it busy past the
  // moment the left DMA is on its way).  `busy` goes up BEFORE the claim — stager_abandon / stager_release wait for
  // it — and the slot may have been closed, or reopened for another batch, until it has: state and next are looked at again
  bool take(Slot& s, uint32_t upper) {
    auto open = [&] {
      return s.staging() && s.next.load(std::memory_order_relaxed) < std::min(upper, s.n_chunks.load(std::memory_order_acquire));
    };
    if (!open()) return false;
    s.busy.fetch_add(1, std::memory_order_acq_rel);
    bool did = false;
    if (open()) {
      const uint32_t idx = s.next.fetch_add(1, std::memory_order_acq_rel);  // (may be >= upper after all, a right chunk: run it)
      uint8_t q = CH_FREE;
      if (idx < s.n_chunks.load(std::memory_order_acquire)) {
        pending->fetch_sub(1, std::memory_order_acq_rel);
        if (s.chunk[idx].st.compare_exchange_strong(q, CH_TAKEN, std::memory_order_acq_rel)) {  // (else: somebody else's already)
          if (c->trace && idx == 0) first_take_ns.fetch_add(ns_since(s.t_begin));
          finish_chunk(s, idx);
        }
        did = true;
      }
    }
    s.busy.fetch_sub(1, std::memory_order_acq_rel);
    return did;
  }

  // any thread: take one chunk of any batch being staged, if there is one
  bool try_one() {
    if (pending->load(std::memory_order_acquire) <= 0) return false;
    for (Slot& s : slot)
      if (take(s, s.n_chunks.load(std::memory_order_acquire))) return true;
    return false;
  }

  // The calling thread, waiting for slot k with nothing left to take: whatever some helper has started
  // and not finished is done again here — a chunk taken and not copied, a complete group whose DMA is
  // not enqueued, a complete batch whose event is not recorded.
  void finish_for(int k) {
    Slot& s = slot[k];
    const uint32_t n = s.n_chunks.load(std::memory_order_acquire);
    for (uint32_t i = 0; i < n; i++)
      if (s.chunk[i].st.load(std::memory_order_acquire) == CH_TAKEN && finish_chunk(s, i)) redone++;
    bool all = true;
    for (int g = 0; g < s.n_groups; g++) {
      Group& gr = s.grp[g];
      if (gr.chunks_left.load(std::memory_order_acquire) != 0) {
        all = false;
      } else if (!gr.dma_enq.load(std::memory_order_acquire)) {  // (its last chunk's thread has not got to it)
        enqueue_dma(s, gr);
        redone++;
      }
    }
    if (all && s.staging()) finish_batch(s);
  }

  // The calling thread until done() says so: it takes chunks itself (take_one) and, after ~25 us with nothing to
  // take — some helper has started something and is not finishing it — redoes what is stuck in slot k instead of
  // waiting for that helper.  Returns the chunks it took.
  template <class Done, class Take>
  uint64_t wait_for(int k, Done done, Take take_one) {
    uint64_t took = 0;
    unsigned idle = 0;
    while (!done()) {
      if (take_one()) {
        took++;
        idle = 0;
      } else if (++idle > 1000) {
        finish_for(k);
        idle = 0;
      } else {
        cpu_relax();
      }
    }
    return took;
  }

  void worker() {
    warm_thread();
    for (;;) {
      if (try_one()) continue;
      std::unique_lock<std::mutex> g(mu);
      cv.wait(g, [&] { return stop.load(std::memory_order_acquire) || pending->load(std::memory_order_acquire) > 0; });
      if (stop.load(std::memory_order_acquire)) return;
    }
  }
};

void stager_copy_bytes(uint8_t* dst, const uint8_t* src, size_t len) { stage_copy(dst, src, len); }
bool stager_pack_bytes(uint8_t* dst, const uint8_t* src, size_t len, uint32_t* base_sec) { return stage_pack(dst, src, len, base_sec); }
void stager_counters(esvio_fe_ctx* c, uint64_t out4[4]) {
  out4[0] = out4[1] = out4[2] = out4[3] = 0;
  if (EventStager* st = c->stager) {
    out4[0] = st->batches;
    out4[1] = st->bytes_staged;
    out4[2] = st->chunks_packed.load(std::memory_order_relaxed);
    out4[3] = st->chunks_raw.load(std::memory_order_relaxed);
  }
}

// what a spinning RANSAC helper does between jobs (host::ransac_pool_set_idle_work): one chunk
static bool stager_idle_work(void* arg) {
  EventStager* st = (EventStager*)arg;
  static thread_local int dev_set = -1;
  if (dev_set != st->c->dev) {  // (the helper enqueues a group's DMA when it copies the group's last chunk)
    st->warm_thread();
    dev_set = st->c->dev;
  }
  return st->try_one();
}

void stager_share_pool(esvio_fe_ctx* c) {
  if (!c->pool) return;
  if (c->stager)
    host::ransac_pool_set_idle_work(c->pool, &c->stage_pending, stager_idle_work, c->stager);
  else
    host::ransac_pool_set_idle_work(c->pool, nullptr, nullptr, nullptr);
}

int stager_threads_from_env() {
  if (const char* v = getenv("ESVIO_FE_STAGE_THREADS")) return std::max(0, std::min(8, atoi(v)));
  return 2;
}

static int stager_get(esvio_fe_ctx* c, EventStager** out) {
  if (!c->stager) {
    EventStager* st = new EventStager();
    st->c = c;
    st->pending = &c->stage_pending;
    c->stage_pending.store(0, std::memory_order_release);
    c->stager = st;  // (from here on a failure leaves through stager_destroy)
    constexpr size_t kWarmBytes = 64;
    bool ok = st->stream.create() == hipSuccess;
    for (Slot& s : st->slot)
      ok = ok && s.copied.create() == hipSuccess && s.copiedL.create() == hipSuccess && s.pf_done.create() == hipSuccess &&
           s.aux_done.create() == hipSuccess && s.main_done.create() == hipSuccess;
    ok = ok && st->warm_pin.alloc(c, kWarmBytes) == 0 && st->warm_dev.alloc(c, kWarmBytes) == 0 && st->warm_ev.create() == hipSuccess;
    for (int i = 0; i < 4; i++) {
      st->gate_rec[i].store(0, std::memory_order_relaxed);
      ok = ok && st->gate_ev[i].create() == hipSuccess;
    }
    if (!ok) {
      stager_destroy(c);
      return fail(c, ESVIO_FE_EHIP, "stream, event or allocation (event staging) failed");
    }
    std::memset(st->warm_pin, 0, kWarmBytes);
    if (const char* v = getenv("ESVIO_FE_STAGE_PACK")) st->pack_enabled = atoi(v) != 0;
    for (int i = 0; i < c->stage_threads; i++) st->threads.emplace_back([st] { st->worker(); });
    stager_share_pool(c);  // the RANSAC helpers, spinning between jobs anyway, take chunks as well
  }
  *out = c->stager;
  return 0;
}

// [p, p + len) is page-locked memory the runtime knows: first AND last byte (a batch that begins inside a registered
// range and runs past its end is staged like pageable memory — k_stage_pull reading beyond the mapping would be a fatal
// queue error, not a return code)
static bool host_range_is_pinned(const void* p, size_t len) {
  auto pinned = [](const void* q) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // (an ordinary malloc'ed pointer is "invalid value" to the runtime)
      return false;
    }
    return a.type == hipMemoryTypeHost;
  };
  return len && pinned(p) && pinned((const uint8_t*)p + len - 1);
}

static int slot_capacity(esvio_fe_ctx* c, Slot& s, size_t n) {
  if (n <= s.cap) return 0;
  s.cap = 0;
  s.pin.release();
  const size_t cap = std::max<size_t>(n + n / 4, 1 << 16);
  if (int rc = s.dev.alloc(c, cap)) return rc;
  if (int rc = s.pin.alloc(c, cap * 16)) return rc;
  s.cap = cap;
  return 0;
}

// the slot's chunk table (and, beside it, the pinned descriptor pairs of a packed batch) for `bytes` in chunks of cb
static int slot_chunks(esvio_fe_ctx* c, Slot& s, size_t bytes, size_t cb) {
  const size_t chunks = (bytes + cb - 1) / cb;
  if (chunks + 4 > s.chunk_cap) {  // (+: a chunk never straddles the two source arrays)
    s.chunk_cap = chunks + 4 + chunks / 4;
    s.chunk.reset(new Chunk[s.chunk_cap]);
  }
  if (2 * s.chunk_cap > s.desc.cap)
    if (int rc = s.desc.alloc(c, 2 * s.chunk_cap)) return rc;
  return 0;
}

// esvio_fe_reserve: every idle slot sized for batches of n events
int stager_reserve(esvio_fe_ctx* c, size_t n_events) {
  if (!stager_enabled(c)) return 0;
  EventStager* st = nullptr;
  if (int rc = stager_get(c, &st)) return rc;
  for (Slot& s : st->slot)
    if (!s.in_use) {
      if (int rc = slot_capacity(c, s, n_events)) return rc;
      if (int rc = slot_chunks(c, s, n_events * 16, chunk_bytes(true))) return rc;
    }
  return 0;
}

struct BatchSrc {  // ---- stager_begin, step by step.  What the caller hands over:
  const uint8_t *left, *right;
  size_t bL, bR;     // bytes of the two arrays: the left one's place in the slot's buffers is [0, bL), the right one's [bL, bL + bR)
  bool pinL, pinR;   // the array is page-locked memory the runtime knows: [lo, hi) is the pageable part's place
  size_t lo() const { return pinL ? bL : 0; }
  size_t hi() const { return pinR ? bL : bL + bR; }
};

// A free slot, big enough, its copy stream ordered behind the kernels that read the slot's previous batch (the
// transfers overwrite its device buffer), its by-batch flags cleared
static int slot_acquire(esvio_fe_ctx* c, EventStager* st, size_t n_events, int* k_out) {
  int k = 0;
  // (a slot a straggling helper is still inside — its chunk was redone by the calling thread — is passed over)
  while (k < kStageSlots && (st->slot[k].in_use || st->slot[k].busy.load(std::memory_order_acquire) != 0)) k++;
  if (k == kStageSlots) return fail(c, ESVIO_FE_EINTERNAL, "no free event staging slot");
  Slot& s = st->slot[k];
  if (int rc = slot_capacity(c, s, n_events)) return rc;
  if (s.pf_rec) HIPCHK(c, hipStreamWaitEvent(st->stream, s.pf_done, 0));
  if (s.main_rec) HIPCHK(c, hipStreamWaitEvent(st->stream, s.main_done, 0));
  if (s.aux_rec) HIPCHK(c, hipStreamWaitEvent(st->stream, s.aux_done, 0));
  s.pf_rec = s.main_rec = s.aux_rec = false;
  s.n_left_chunks = s.n_left_groups = 0;
  s.left_enq.store(false, std::memory_order_release);
  s.n_chunks.store(0, std::memory_order_release);
  s.next.store(0, std::memory_order_release);
  *k_out = k;
  return 0;
}

// A pinned array: one transfer straight from it, now.
// (a batch the calling thread waits for: pulled by a kernel, as its pageable groups are — hipMemcpyAsync out of
// hipHostRegister'ed memory ran at 10 GB/s on this stack: the plain call took 0.77 ms against 0.40 with the pull
// kernel and 0.45 from pageable memory; an announced batch: the copy engine, which costs the compute streams nothing)
static bool send_pinned(EventStager* st, Slot& s, void* dst, const void* src, size_t len) {
  if (!s.pull) return st->dma(dst, src, len);
  // (hipHostMalloc memory is mapped at its host address; hipHostRegister'ed memory need not be: ask)
  // The kernel reads uint4s: a source that is not 16-byte aligned (an EventArray inside a deserialisation buffer is
  // only 8-byte aligned in general), or whose first and last byte are mapped by two different registrations that do
  // not continue each other on the device side, goes through the copy engine instead.
  void *dp = nullptr, *dp_last = nullptr;
  if (hipHostGetDevicePointer(&dp, const_cast<void*>(src), 0) != hipSuccess || !dp || ((uintptr_t)dp & 15) != 0 ||
      ((uintptr_t)dst & 15) != 0 ||
      hipHostGetDevicePointer(&dp_last, (uint8_t*)const_cast<void*>(src) + len - 1, 0) != hipSuccess ||
      (uint8_t*)dp_last != (uint8_t*)dp + len - 1) {
    (void)hipGetLastError();
    return st->dma(dst, src, len);
  }
  (void)hipGetLastError();
  launch_stage_pull(st->stream, dp, dst, len);
  return hipGetLastError() == hipSuccess;
}

// ... both arrays' pinned parts, and copiedL where that settles the left array: it is on its way already, or there is none
static int send_pinned_parts(esvio_fe_ctx* c, EventStager* st, Slot& s, const BatchSrc& b, bool by_camera) {
  bool ok = !b.pinL || send_pinned(st, s, s.dev, b.left, b.bL);
  if (ok && by_camera && (b.pinL || !b.bL)) {
    HIPCHK(c, hipEventRecord(s.copiedL, st->stream));
    s.left_enq.store(true, std::memory_order_release);
  }
  ok = ok && (!b.pinR || send_pinned(st, s, (uint8_t*)s.dev + b.bL, b.right, b.bR));
  return ok ? 0 : fail(c, ESVIO_FE_EHIP, "event staging from pinned memory failed");
}

// The pageable part into groups (one transfer each) of whole chunks of cb bytes, a chunk never straddling the two
// source arrays: the slot's group and chunk tables and their counts, nothing else — no HIP call.  Returns the chunks.
// by_camera: the left and the right array are two groups each (group k's transfer runs under the memcpy of group
// k + 1; the left array's can be waited for on their own); otherwise <= dma_groups groups over the whole range
static uint32_t cut_batch(Slot& s, const BatchSrc& b, size_t cb, int dma_groups, bool by_camera) {
  int ng = 0;
  uint32_t nch = 0;
  auto split = [&](size_t a0, size_t b0, int want) {  // [a0, b0) into <= want groups of whole chunks
    const size_t nc = (b0 - a0 + cb - 1) / cb;
    const int k = (int)std::min<size_t>((size_t)std::max(1, want), nc);
    const size_t per = (nc + k - 1) / k;
    for (size_t o = a0; o < b0 && ng < kMaxGroups; o += per * cb) {
      s.grp[ng].off = o;
      s.grp[ng].len = (ng == kMaxGroups - 1 ? b0 : std::min(b0, o + per * cb)) - o;
      ng++;
    }
  };
  if (by_camera) {
    if (!b.pinL && b.bL) {
      split(0, b.bL, 2);
      s.n_left_groups = ng;
    }
    if (!b.pinR && b.bR) split(b.bL, b.bL + b.bR, 2);
  } else if (b.hi() > b.lo()) {
    split(b.lo(), b.hi(), std::min(dma_groups, kMaxGroups));
  }
  for (int g = 0; g < ng; g++) {
    Group& gr = s.grp[g];
    gr.first_chunk = nch;
    gr.dma_enq.store(false, std::memory_order_relaxed);
    for (size_t o = gr.off, end; o < gr.off + gr.len; o = end) {
      const bool in_left = o < b.bL;
      end = std::min(std::min(o + cb, gr.off + gr.len), in_left ? b.bL : gr.off + gr.len);
      Chunk& ch = s.chunk[nch++];
      ch.group = g;
      ch.src = in_left ? b.left + o : b.right + (o - b.bL);
      ch.off = o;
      ch.len = end - o;
      ch.st.store(CH_FREE, std::memory_order_relaxed);
    }
    gr.chunks_left.store(nch - gr.first_chunk, std::memory_order_relaxed);
    if (g < s.n_left_groups) s.n_left_chunks = nch;
  }
  s.n_groups = ng;
  s.groups_left.store((uint32_t)ng, std::memory_order_relaxed);
  return nch;
}

// The slot is the batch's from here on: open for taking, the helpers woken — or, with nothing pageable in it, complete
static int slot_open(esvio_fe_ctx* c, EventStager* st, Slot& s, uint32_t nch) {
  if (!nch && hipEventRecord(s.copied, st->stream) != hipSuccess) return fail(c, ESVIO_FE_EHIP, "hipEventRecord (event staging) failed");
  s.in_use = true;
  s.n_chunks.store(nch, std::memory_order_release);
  s.t_begin = Clock::now();
  s.state.store(nch ? SL_STAGING : SL_SENT, std::memory_order_release);
  if (nch) {
    st->pending->fetch_add((int)nch, std::memory_order_acq_rel);
    { std::lock_guard<std::mutex> g(st->mu); }  // (a helper between its predicate and its sleep sees the count)
    st->cv.notify_all();
  }
  return 0;
}

// Start staging [left; right] into a free slot: returns at once, the helpers do the work.
// dma_groups: pieces the pageable part of the batch is moved in (1: an announced batch, nobody waits for it: one
// DMA; more: a plain call's batch, piece k goes to the device — by k_stage_pull — under the memcpy of piece k+1)
// by_camera: the left array and the right array are two pieces each (dma_groups is ignored), and the left
// one's arrival can be waited for on its own (stager_attach_left)
int stager_begin(esvio_fe_ctx* c, const esvio_fe_event* left, size_t nL, const esvio_fe_event* right, size_t nR,
                 int dma_groups, int* slot_out, bool by_camera) {
  EventStager* st = nullptr;
  if (int rc = stager_get(c, &st)) return rc;
  NsScope lap{st->begin_ns};  // (the stager's one-time set-up above — stream, events, threads: ~9 ms — is not part of a batch's figure)
  const auto tp0 = Clock::now();
  const BatchSrc b{(const uint8_t*)left, (const uint8_t*)right, nL * 16, nR * 16, host_range_is_pinned(left, nL * 16),
                   host_range_is_pinned(right, nR * 16)};
  st->pin_ns += ns_since(tp0);
  int k = 0;
  if (int rc = slot_acquire(c, st, nL + nR, &k)) return rc;
  Slot& s = st->slot[k];
  s.pull = by_camera || dma_groups > 1;  // (a batch the calling thread waits for)
  // by-camera staging of a batch the call waits for: chunks of one size, every group whole chunks of one array —
  // what the packed form needs (k_stage_pull_packed finds an event's chunk by division)
  const size_t cb = chunk_bytes(by_camera);
  s.pack = st->pack_enabled && by_camera;
  s.pack_epc = (uint32_t)(cb / 16);
  st->bytes_staged += b.bL + b.bR;
  st->batches++;
  if (int rc = send_pinned_parts(c, st, s, b, by_camera)) return rc;
  if (b.hi() > b.lo())
    if (int rc = slot_chunks(c, s, b.hi() - b.lo(), cb)) return rc;
  if (int rc = slot_open(c, st, s, cut_batch(s, b, cb, dma_groups, by_camera))) return rc;
  *slot_out = k;
  return 0;
}

bool stager_ready(esvio_fe_ctx* c, int slot) {
  const bool r = !c->stager->slot[slot].staging();
  if (!r) c->stager->skipped++;
  return r;
}

// wait until every DMA of the slot's batch is enqueued (the calling thread takes chunks itself
// meanwhile), then make stream `s` wait for them; device pointers out
int stager_attach(esvio_fe_ctx* c, int slot, size_t nL, hipStream_t s, const EventRec** dL, const EventRec** dR) {
  EventStager* st = c->stager;
  Slot& sl = st->slot[slot];
  if (sl.staging()) {
    NsScope w{st->wait_ns};
    st->caller_chunks += st->wait_for(slot, [&] { return !sl.staging(); }, [&] { return st->try_one(); });
  }
  if (sl.state.load(std::memory_order_acquire) != SL_SENT) {
    // a DMA could not be enqueued: chunks of this slot may still be queued or being copied from the
    // caller's memory, which is the caller's again once this call has returned — finish them first
    stager_abandon(c, slot);
    return fail(c, ESVIO_FE_EHIP, "staging the event batch failed");
  }
  HIPCHK(c, hipStreamWaitEvent(s, sl.copied, 0));
  stager_ptrs(c, slot, nL, dL, dR);
  return 0;
}

// by_camera staging: wait (taking the left array's chunks meanwhile) until the LEFT array's DMA is enqueued and make
// stream `s` wait for it; the right array may still be on its way (stager_attach follows for it)
int stager_attach_left(esvio_fe_ctx* c, int slot, hipStream_t s, const EventRec** dL) {
  EventStager* st = c->stager;
  Slot& sl = st->slot[slot];
  NsScope lap{st->left_ns};
  st->left_calls++;
  st->caller_chunks += st->wait_for(
      slot, [&] { return sl.left_enq.load(std::memory_order_acquire) || !sl.staging(); }, [&] { return st->take(sl, sl.n_left_chunks); });
  const int stt = sl.state.load(std::memory_order_acquire);
  const bool left = sl.left_enq.load(std::memory_order_acquire);
  if (stt == SL_FAILED || (!left && stt != SL_SENT)) {
    stager_abandon(c, slot);
    return fail(c, ESVIO_FE_EHIP, "staging the event batch failed (left array)");
  }
  // (the whole batch can be complete — finish_for closed it — while the thread that sent the last left
  // group has not got to recording copiedL yet: the batch's own event covers the left array as well)
  HIPCHK(c, hipStreamWaitEvent(s, left ? sl.copiedL : sl.copied, 0));
  *dL = sl.dev;
  return 0;
}

// give a slot back whose batch will not be tracked (a failed call): nothing of the caller's memory is
// read after this returns
void stager_abandon(esvio_fe_ctx* c, int slot) {
  if (slot < 0 || !c->stager) return;
  EventStager* st = c->stager;
  Slot& sl = st->slot[slot];
  {  // chunks of this slot nobody has taken: never will be
    const uint32_t n = sl.n_chunks.load(std::memory_order_acquire);
    const uint32_t nx = sl.next.exchange(n, std::memory_order_acq_rel);
    if (nx < n) st->pending->fetch_sub((int)(n - nx), std::memory_order_acq_rel);
    sl.state.store(SL_FAILED, std::memory_order_release);  // (closed for taking)
  }
  while (sl.busy.load(std::memory_order_acquire) != 0) cpu_relax();  // chunks a thread holds: waited for
  (void)hipStreamSynchronize(st->stream);  // (DMAs straight from a pinned source, groups already enqueued)
  for (int g2 = 0; g2 < kMaxGroups; g2++) sl.grp[g2].chunks_left.store(0, std::memory_order_relaxed);
  sl.groups_left.store(0, std::memory_order_relaxed);
  sl.state.store(SL_IDLE, std::memory_order_release);
  sl.in_use = false;
}

// where the slot's batch will be on the device (known as soon as the slot is taken)
void stager_ptrs(esvio_fe_ctx* c, int slot, size_t nL, const EventRec** dL, const EventRec** dR) {
  Slot& sl = c->stager->slot[slot];
  *dL = sl.dev;
  *dR = sl.dev + nL;
}

// the kernels enqueued on `s` so far are the last ones on that stream to read the slot's device buffer
int stager_mark_read(esvio_fe_ctx* c, int slot, hipStream_t s, bool main_stream) {
  Slot& sl = c->stager->slot[slot];
  HIPCHK(c, hipEventRecord(main_stream ? sl.main_done : sl.pf_done, s));
  (main_stream ? sl.main_rec : sl.pf_rec) = true;
  return 0;
}
// ... and on a third stream (the stereo stream, where a plain call runs the right camera's update)
int stager_mark_read_aux(esvio_fe_ctx* c, int slot, hipStream_t s) {
  Slot& sl = c->stager->slot[slot];
  HIPCHK(c, hipEventRecord(sl.aux_done, s));
  sl.aux_rec = true;
  return 0;
}

// the batch has been tracked.  The caller's memory is free again when its track call returns: a
// DMA straight from a pinned source has to be over by then (it long is; the wait costs ~1 us)
int stager_release(esvio_fe_ctx* c, int slot) {
  if (slot < 0 || !c->stager) return 0;
  Slot& sl = c->stager->slot[slot];
  sl.in_use = false;
  if (sl.state.load(std::memory_order_acquire) == SL_SENT) HIPCHK(c, hipEventSynchronize(sl.copied));
  // (a helper whose chunk was redone may still be inside its own copy of it: it reads the caller's memory)
  while (sl.busy.load(std::memory_order_acquire) != 0) cpu_relax();
  return 0;
}

// every queued chunk done, every slot free (esvio_fe_reset)
void stager_drain(esvio_fe_ctx* c) {
  EventStager* st = c->stager;
  if (!st) return;
  for (int k = 0; k < kStageSlots; k++) {
    Slot& s = st->slot[k];
    (void)st->wait_for(k, [&] { return !s.staging(); }, [&] { return st->try_one(); });
    while (s.busy.load(std::memory_order_acquire) != 0) cpu_relax();
    s.in_use = false;
  }
  (void)hipStreamSynchronize(st->stream);
}

void stager_destroy(esvio_fe_ctx* c) {
  EventStager* st = c->stager;
  if (!st) return;
  if (c->pool) host::ransac_pool_set_idle_work(c->pool, nullptr, nullptr, nullptr);
  st->stop.store(true, std::memory_order_release);
  { std::lock_guard<std::mutex> g(st->mu); }
  st->cv.notify_all();
  for (std::thread& t : st->threads) t.join();
  if (c->trace && st->batches)
    fprintf(stderr, "[esvio_fe trace] host-event staging: %llu batches, %.1f MB, %d helper threads; calling thread waited "
            "%.3f ms per batch (took %llu chunks itself, redid %llu a helper had not finished), %llu take-ups postponed to the next call\n",
            (unsigned long long)st->batches, st->bytes_staged / 1e6, (int)st->threads.size(),
            st->wait_ns / 1e6 / st->batches, (unsigned long long)st->caller_chunks, (unsigned long long)st->redone,
            (unsigned long long)st->skipped);
  if (c->trace && st->batches)
    fprintf(stderr, "[esvio_fe trace] host-event staging, calling thread per batch: stager_begin %.1f us (pinned-or-not query %.1f), "
            "wait for the left array %.1f us (%llu by-camera batches), wait for the whole batch %.1f us; %llu DMAs went out without waiting for the one two before\n",
            st->begin_ns / 1e3 / st->batches, st->pin_ns / 1e3 / st->batches, st->left_calls ? st->left_ns / 1e3 / st->left_calls : 0.0,
            (unsigned long long)st->left_calls, st->wait_ns / 1e3 / st->batches, (unsigned long long)st->gate_expired.load());
  if (c->trace && st->chunk_cnt.load())
    fprintf(stderr, "[esvio_fe trace] host-event staging: %.2f us inside a chunk's copy / packing on average (%llu chunks), chunk 0 taken %.1f us after "
            "the batch's opening, the left array's last group enqueued after %.1f us, the batch's after %.1f us\n",
            st->chunk_ns.load() / 1e3 / st->chunk_cnt.load(), (unsigned long long)st->chunk_cnt.load(), st->first_take_ns.load() / 1e3 / st->batches,
            st->left_sent_ns.load() / 1e3 / std::max<uint64_t>(1, st->left_calls), st->all_sent_ns.load() / 1e3 / st->batches);
  if (st->stream) (void)hipStreamSynchronize(st->stream);
  delete st;
  c->stager = nullptr;
}

}  // namespace fe
}  // namespace esvio
