// fe_aedat.h — the host walk over a libcaer / AEDAT 3.1 packet stream (include/esvio_fe.h has the rule).
// No HIP in here: inline functions over a plain state struct, so that the library, the test tap, the stand-alone
// sanitizer program and tools/aedat_seq_decode.cpp all run the same lines.
//
// The packet chain is a linked list — each header says where the next one lies — so it is walked on the host, at one
// cache line per packet.  The event walk gathers the polarity records of a chunk, and nothing else, into one packed array
// and writes a run table beside it (per run of records with one eventTSOverflow: the index of its first record); the
// device decodes that array one record per lane.  The side walk decodes special and IMU6 packets where they lie: they
// are few.  A record cut by the chunk's end waits in the state and is completed by the next chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/esvio_fe.h"

namespace esvio {
namespace aedat {

constexpr uint32_t kHeaderBytes = 28, kMaxRecordBytes = 36;
constexpr int kSpecial = 0, kPolarity = 1, kImu6 = 3;
constexpr uint64_t kStampLimitNs = 4294967296ull * 1000000000ull;  // sec >= 2^32

// One walker's state (a handle has two per camera: the event call's and the side call's).  Between packets
// payload_left == 0; all zero is the fresh state.
struct Walk {
  uint8_t hdr[kHeaderBytes];     // the header bytes collected so far
  uint32_t hdr_have;             // 0..27
  int32_t type, ev_size, overflow;  // the open packet
  uint32_t decoded;              // this walker decodes the open packet's records (else it is skipped whole)
  uint64_t events_left;          // records of a decoded packet still to come
  uint64_t payload_left;         // payload bytes still to come, records and padding
  uint8_t rec[kMaxRecordBytes];  // the bytes of a record cut by the chunk's end
  uint32_t rec_have;             // 0..ev_size-1
};

struct Run {  // the records from `first` on (up to the next run's first) have this eventTSOverflow
  uint32_t first;
  int32_t overflow;
};

inline int32_t rd_i32(const uint8_t* p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
inline uint32_t rd_u32(const uint8_t* p) { return (uint32_t)rd_i32(p); }
inline int16_t rd_i16(const uint8_t* p) { return (int16_t)((uint32_t)p[0] | (uint32_t)p[1] << 8); }
inline float rd_f32(const uint8_t* p) {
  const uint32_t u = rd_u32(p);
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// The stamp of a record: false = BAD.  ts64 >= 2^53 is BAD whatever the offset (|t_offset_ns| <= 2^62), and below it
// ts64 * 1000 + t_offset_ns lies in [-2^62, 2^64): the sum modulo 2^64 is exact when it is not negative, and a negative
// sum lands at or above 2^63 — beyond the limit either way.
inline bool stamp(int32_t ts, int32_t overflow, int64_t t_offset_ns, uint32_t* sec, uint32_t* nsec, uint64_t* ticks_ns) {
  *sec = *nsec = 0, *ticks_ns = 0;
  if (ts < 0 || overflow < 0) return false;
  const uint64_t ts64 = (uint64_t)overflow << 31 | (uint32_t)ts;
  if (ts64 >= (1ull << 53)) return false;
  const uint64_t u = ts64 * 1000u + (uint64_t)t_offset_ns;
  if (u >= kStampLimitNs) return false;
  *ticks_ns = u, *sec = (uint32_t)(u / 1000000000u), *nsec = (uint32_t)(u % 1000000000u);
  return true;
}

// What one walk call produces.  Pointers may be null: the walk then counts only.
struct Out {
  // the event walk
  Run* runs = nullptr;          // room for runs_cap entries
  size_t runs_cap = 0;
  uint8_t* payload = nullptr;   // room for events_cap 8-byte records
  size_t events_cap = 0;
  uint64_t n_runs = 0, n_events = 0;  // counted whether stored or not
  int32_t last_overflow = 0;          // (of the run open at n_runs - 1)
  uint64_t polarity_packets = 0;
  // the side walk
  esvio_fe_imu_sample* imu = nullptr;
  size_t imu_cap = 0;
  esvio_fe_trigger* trig = nullptr;
  size_t trig_cap = 0;
  uint64_t n_imu = 0, n_trig = 0, resets = 0, other_specials = 0, invalid = 0, bad = 0;
  uint64_t special_packets = 0, imu_packets = 0;
  // both
  uint64_t other_packets = 0;
  const char* why = nullptr;  // a malformed header: which rule it breaks
};

enum Mode { kEvents = 0, kSide = 1 };

// a complete header -> the open packet; false: malformed (out->why says how)
inline bool open_packet(Walk* w, Mode mode, Out* out) {
  const int32_t type = rd_i16(w->hdr), size = rd_i32(w->hdr + 4), ts_off = rd_i32(w->hdr + 8), overflow = rd_i32(w->hdr + 12);
  const int32_t capacity = rd_i32(w->hdr + 16), number = rd_i32(w->hdr + 20);
  if (size <= 0) return out->why = "eventSize <= 0", false;
  if (capacity < 0) return out->why = "eventCapacity < 0", false;
  if (number < 0) return out->why = "eventNumber < 0", false;
  if (number > capacity) return out->why = "eventNumber > eventCapacity", false;
  if (type == kSpecial || type == kPolarity || type == kImu6) {
    if (size != (type == kImu6 ? 36 : 8)) return out->why = "eventSize differs from the type's", false;
    if (ts_off != 4) return out->why = "eventTSOffset differs from the type's", false;
  }
  w->type = type, w->ev_size = size, w->overflow = overflow;
  w->decoded = mode == kEvents ? type == kPolarity : (type == kSpecial || type == kImu6);
  w->events_left = w->decoded ? (uint64_t)number : 0;
  w->payload_left = (uint64_t)capacity * (uint64_t)size;
  if (type == kPolarity)
    out->polarity_packets++;
  else if (type == kSpecial)
    out->special_packets++;
  else if (type == kImu6)
    out->imu_packets++;
  else
    out->other_packets++;
  return true;
}

// `count` whole records of the open packet at p
inline void take_records(const Walk& w, Mode mode, const uint8_t* p, uint64_t count, int64_t t_offset_ns, uint32_t flags, Out* out) {
  if (mode == kEvents) {
    if (out->n_runs == 0 || out->last_overflow != w.overflow) {
      if (out->runs && out->n_runs < out->runs_cap) out->runs[out->n_runs] = Run{(uint32_t)out->n_events, w.overflow};
      out->n_runs++, out->last_overflow = w.overflow;
    }
    if (out->payload && out->n_events + count <= out->events_cap) memcpy(out->payload + out->n_events * 8, p, (size_t)count * 8);
    out->n_events += count;
    return;
  }
  for (uint64_t k = 0; k < count; k++, p += w.ev_size) {
    const uint32_t data = rd_u32(p);
    if (!(data & 1u) && !(flags & ESVIO_FE_AEDAT_KEEP_INVALID)) {
      out->invalid++;
      continue;
    }
    const uint32_t stype = (data >> 1) & 0x7fu;
    if (w.type == kSpecial && (stype < 2 || stype > 4)) {  // no record: no stamp to be BAD
      if (stype == 1)
        out->resets++;
      else
        out->other_specials++;
      continue;
    }
    uint32_t sec, nsec;
    uint64_t ticks;
    if (!stamp(rd_i32(p + 4), w.overflow, t_offset_ns, &sec, &nsec, &ticks)) {
      out->bad++;
      continue;
    }
    if (w.type == kSpecial) {
      if (out->trig && out->n_trig < out->trig_cap) {
        esvio_fe_trigger t;
        memset(&t, 0, sizeof t);
        t.sec = sec, t.nsec = nsec, t.id = (uint8_t)stype, t.value = stype != 3;
        out->trig[out->n_trig] = t;
      }
      out->n_trig++;
    } else {
      if (out->imu && out->n_imu < out->imu_cap) {
        // davis_ros_driver/src/driver.cpp:735-741: the float negated, widened, then the operations left to right
        const float ax = rd_f32(p + 8), ay = rd_f32(p + 12), az = rd_f32(p + 16);
        const float gx = rd_f32(p + 20), gy = rd_f32(p + 24), gz = rd_f32(p + 28);
        const double g = 9.81, pi = 3.14159265358979323846;
        esvio_fe_imu_sample s;
        memset(&s, 0, sizeof s);
        s.sec = sec, s.nsec = nsec;
        s.acc[0] = -ax * g, s.acc[1] = ay * g, s.acc[2] = -az * g;
        s.gyr[0] = -gx / 180.0 * pi, s.gyr[1] = gy / 180.0 * pi, s.gyr[2] = -gz / 180.0 * pi;
        out->imu[out->n_imu] = s;
      }
      out->n_imu++;
    }
  }
}

// The walk: *w advanced by the n bytes at `bytes`.  Returns false at a malformed header; the caller works on a copy of
// the state and takes it over when the whole call succeeds.  Reads bytes[0 .. n) and nothing else.
inline bool walk(Walk* w, Mode mode, const uint8_t* bytes, size_t n, int64_t t_offset_ns, uint32_t flags, Out* out) {
  size_t pos = 0;
  while (pos < n) {
    if (w->payload_left == 0) {  // between packets: the header
      const size_t take = n - pos < kHeaderBytes - w->hdr_have ? n - pos : kHeaderBytes - w->hdr_have;
      memcpy(w->hdr + w->hdr_have, bytes + pos, take);
      w->hdr_have += (uint32_t)take, pos += take;
      if (w->hdr_have < kHeaderBytes) break;
      if (!open_packet(w, mode, out)) return false;
      w->hdr_have = 0;
      continue;
    }
    if (w->events_left) {
      const uint32_t size = (uint32_t)w->ev_size;
      if (w->rec_have) {  // the record the last chunk cut
        const size_t take = n - pos < size - w->rec_have ? n - pos : size - w->rec_have;
        memcpy(w->rec + w->rec_have, bytes + pos, take);
        w->rec_have += (uint32_t)take, pos += take, w->payload_left -= take;
        if (w->rec_have < size) break;
        take_records(*w, mode, w->rec, 1, t_offset_ns, flags, out);
        w->rec_have = 0, w->events_left--;
        continue;
      }
      const uint64_t fit = (n - pos) / size, whole = fit < w->events_left ? fit : w->events_left;
      if (whole) {
        take_records(*w, mode, bytes + pos, whole, t_offset_ns, flags, out);
        pos += (size_t)(whole * size), w->payload_left -= whole * size, w->events_left -= whole;
        continue;
      }
      const size_t take = n - pos;  // fewer bytes than a record: they wait
      memcpy(w->rec, bytes + pos, take);
      w->rec_have = (uint32_t)take, pos = n, w->payload_left -= take;
    } else {  // padding, or a packet this walker skips whole
      const uint64_t skip = w->payload_left < n - pos ? w->payload_left : n - pos;
      pos += (size_t)skip, w->payload_left -= skip;
    }
  }
  return true;
}

// ---- the file header (host only; the rule: include/esvio_fe.h) ----
inline int file_header(const void* bytes, size_t n, esvio_fe_aedat_header_info* out) {
  if (!out || (n && !bytes)) return ESVIO_FE_EINVAL;
  memset(out, 0, sizeof *out);
  const char* b = (const char*)bytes;
  size_t pos = 0;
  bool ended = false, first = true;
  while (!ended) {
    if (pos == n) break;
    if (b[pos] != '#') {
      ended = true;
      break;
    }
    const char* nl = (const char*)memchr(b + pos, '\n', n - pos);
    if (!nl) break;
    const char* p = b + pos;
    const char* end = nl;
    if (end > p && end[-1] == '\r') end--;
    pos = (size_t)(nl - b) + 1;
    const size_t len = (size_t)(end - p);
    if (len == 12 && memcmp(p, "#!END-HEADER", 12) == 0) {
      ended = true;
    } else if (first && len >= 9 && memcmp(p, "#!AER-DAT", 9) == 0) {  // "#!AER-DAT<a>.<b>": 10 a + b
      const char* q = p + 9;
      int64_t a = 0, f = 0;
      bool ok = q < end && *q >= '0' && *q <= '9';
      for (; q < end && *q >= '0' && *q <= '9' && a < 100000; q++) a = a * 10 + (*q - '0');
      ok = ok && q + 1 < end && *q == '.' && q[1] >= '0' && q[1] <= '9';
      if (ok) {
        for (q++; q < end && *q >= '0' && *q <= '9' && f < 100000; q++) f = f * 10 + (*q - '0');
        if (q == end && a < 100000 && f < 10) out->version = (int32_t)(10 * a + f);
      }
    }
    first = false;
  }
  out->payload_offset = pos;
  out->complete = ended ? 1 : 0;
  return 0;
}

}  // namespace aedat
}  // namespace esvio
