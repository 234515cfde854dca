// fe_aedat.h — the host walk over a libcaer / AEDAT 3.1 packet stream (include/esvio_fe.h has the rule).
// No HIP in here: inline functions over a plain state struct, so that the library, the test tap, the stand-alone
// sanitizer program and tools/aedat_seq_decode.cpp all run the same lines.
//
// The packet chain is a linked list — each header says where the next one lies — so it is walked on the host, at one
// cache line per packet.  The event walk gathers the polarity records of a chunk, and nothing else, into one packed array
// and writes a run table beside it (per run of records with one eventTSOverflow: the index of its first record); the
// device decodes that array one record per lane.  The side walk decodes special and IMU6 packets where they lie: they
// are few.  A record cut by the chunk's end waits in the state and is completed by the next chunk.  The frame walk
// ("AEDAT 3.1 frames") gathers each emitted frame event's pixel bytes, and nothing else, each from a 16-byte boundary, and
// lists the frames; the pixel bytes of a frame that the call's end cuts wait in a carry buffer beside the state (Carry),
// the way fe_bag.h's image mode keeps an Image payload.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/esvio_fe.h"

namespace esvio {
namespace aedat {

constexpr uint32_t kHeaderBytes = 28, kMaxRecordBytes = 36;
constexpr int kSpecial = 0, kPolarity = 1, kImu6 = 3;
constexpr int kFrame = 2;
constexpr uint32_t kFrameHead = 36;  // a frame event's head: info, four stamps, lengthX/Y, positionX/Y
constexpr uint64_t kStampLimitNs = 4294967296ull * 1000000000ull;  // sec >= 2^32

// One walker's state (a handle has three per camera: the event call's, the side call's and the frame call's).  Between
// packets payload_left == 0; all zero is the fresh state.
struct Walk {
  uint8_t hdr[kHeaderBytes];     // the header bytes collected so far
  uint32_t hdr_have;             // 0..27
  int32_t type, ev_size, overflow;  // the open packet
  uint32_t decoded;              // this walker decodes the open packet's records (else it is skipped whole)
  uint64_t events_left;          // records of a decoded packet still to come
  uint64_t payload_left;         // payload bytes still to come, records and padding
  uint8_t rec[kMaxRecordBytes];  // the bytes of a record cut by the chunk's end
  uint32_t rec_have;             // 0..ev_size-1
  // the frame walk alone (rec holds the open frame event's head, which stays until the event ends)
  uint32_t ev_off;               // bytes of the open frame event that have come, 0..ev_size-1
  uint32_t slot;                 // its position within its packet
  uint32_t emit;                 // it is emitted when its last pixel byte comes (else: dropped, BAD, or its pixels are behind us)
  uint32_t f_sec, f_nsec;        // ... with this stamp
  uint32_t carry_buf;            // which of the Carry's two buffers holds its pixel bytes so far
  uint64_t pix_left;             // its pixel bytes still to come
  uint64_t carry_len;            // ... and how many wait in the Carry
};

// The pixel bytes of a frame that a call's end cut, beside the frame walker's state (Walk::carry_buf, carry_len say which
// buffer and how much of it counts).  Two buffers, used as fe_bag.h's Carry is: a call whose first frame was waiting in
// one puts what it leaves waiting into the other, so a call that fails after its gathering walk has overwritten nothing
// of the state it goes back to.  A frame still open at the call's end grows in place, behind the bytes that count.
struct Carry {
  std::vector<uint8_t> buf[2];
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
  // the frame walk: want_w x want_h the only size taken (0: any); pix null: counted only; carry null: nothing waits
  uint32_t want_w = 0, want_h = 0;
  Carry* carry = nullptr;
  uint8_t* pix = nullptr;  // room for pix_cap bytes: the emitted frames' pixel bytes, each from a 16-byte boundary
  size_t pix_cap = 0;
  esvio_fe_aedat_frame* frames = nullptr;
  size_t frames_cap = 0;
  uint64_t n_pix_bytes = 0, n_frames = 0, frame_packets = 0;  // counted whether stored or not
  uint32_t first_stamp[2] = {0, 0}, last_stamp[2] = {0, 0};   // (sec, nsec) of the first / last emitted frame
  // all
  uint64_t other_packets = 0;
  const char* why = nullptr;  // a malformed header or event, or a refused frame: which rule it breaks
  char why_buf[160];
};

enum Mode { kEvents = 0, kSide = 1, kFrames = 2 };

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
  if (mode == kFrames && type == kFrame) {
    if (size < (int32_t)kFrameHead) return out->why = "a frame packet's eventSize is below 36", false;
    if ((size - (int32_t)kFrameHead) & 1) return out->why = "a frame packet's eventSize - 36 is odd", false;
    if (ts_off != 12) return out->why = "a frame packet's eventTSOffset is not 12", false;
  }
  w->type = type, w->ev_size = size, w->overflow = overflow;
  w->decoded = mode == kEvents ? type == kPolarity : mode == kSide ? (type == kSpecial || type == kImu6) : type == kFrame;
  w->events_left = w->decoded ? (uint64_t)number : 0;
  w->payload_left = (uint64_t)capacity * (uint64_t)size;
  if (type == kPolarity)
    out->polarity_packets++;
  else if (type == kSpecial)
    out->special_packets++;
  else if (type == kImu6)
    out->imu_packets++;
  else if (mode == kFrames && type == kFrame)
    out->frame_packets++, w->slot = 0;
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

// ---- the frame walk (the rule: include/esvio_fe.h "AEDAT 3.1 frames") ----
// The open frame event's head is complete (w->rec): what becomes of the event.  false: malformed or refused (out->why).
inline bool frame_head(Walk* w, int64_t t_offset_ns, uint32_t flags, Out* out) {
  const uint32_t info = rd_u32(w->rec);
  w->emit = 0, w->pix_left = 0;
  if (!(info & 1u) && !(flags & ESVIO_FE_AEDAT_KEEP_INVALID)) {
    out->invalid++;
    return true;
  }
  const int64_t lx = rd_i32(w->rec + 20), ly = rd_i32(w->rec + 24), ch = (info >> 1) & 7u;
  const uint64_t room = (uint64_t)((uint32_t)w->ev_size - kFrameHead);
  if (lx < 1) return out->why = "a frame event's lengthX is below 1", false;
  if (ly < 1) return out->why = "a frame event's lengthY is below 1", false;
  // lengthX * lengthY * channels * 2 > eventSize - 36 in exact integers: the first product is below 2^62
  if (ch && (uint64_t)(lx * ly) > room / (uint64_t)(2 * ch)) return out->why = "a frame event's lengthX * lengthY * channels * 2 exceeds eventSize - 36", false;
  if (ch != 1 && ch != 3) {
    snprintf(out->why_buf, sizeof out->why_buf, "a frame event with %d channels: 1 (mono8) and 3 (rgb8) are taken", (int)ch);
    return out->why = out->why_buf, false;
  }
  if (out->want_w && (lx != (int64_t)out->want_w || ly != (int64_t)out->want_h)) {
    snprintf(out->why_buf, sizeof out->why_buf, "a frame event of %d x %d, the handle's size is %u x %u: cv::resize is out of scope", (int)lx, (int)ly,
             out->want_w, out->want_h);
    return out->why = out->why_buf, false;
  }
  const int64_t s = rd_i32(w->rec + 12), e = rd_i32(w->rec + 16);
  const int64_t ts = s + (e - s) / 2;  // (between s and e: an int32)
  uint64_t ticks;
  if (!stamp((int32_t)ts, w->overflow, t_offset_ns, &w->f_sec, &w->f_nsec, &ticks)) {
    out->bad++;
    return true;
  }
  w->emit = 1, w->pix_left = (uint64_t)(lx * ly) * (uint64_t)(2 * ch);
  return true;
}

// `take` pixel bytes of the open frame event at p.  The event's last ones: the frame, the waiting bytes in front, goes to
// out->pix at the next 16-byte boundary and is listed.  Else the call ends inside it: they wait.
inline void frame_pixels(Walk* w, const uint8_t* p, uint64_t take, uint32_t start_buf, Out* out) {
  if (take < w->pix_left) {
    if (w->carry_len == 0) w->carry_buf = start_buf ^ 1u;  // (never the buffer the call's first frame waited in)
    if (out->carry) {
      std::vector<uint8_t>& b = out->carry->buf[w->carry_buf & 1u];
      if (b.size() < w->carry_len + take) b.resize((size_t)(w->carry_len + take));
      memcpy(b.data() + w->carry_len, p, (size_t)take);
    }
    w->carry_len += take, w->pix_left -= take;
    return;
  }
  const uint64_t total = w->carry_len + take;
  if (out->pix && out->carry && out->n_pix_bytes + total <= out->pix_cap) {
    if (w->carry_len) memcpy(out->pix + out->n_pix_bytes, out->carry->buf[w->carry_buf & 1u].data(), (size_t)w->carry_len);
    memcpy(out->pix + out->n_pix_bytes + w->carry_len, p, (size_t)take);
  }
  out->n_pix_bytes += (total + 15) & ~(uint64_t)15;
  if (out->frames && out->n_frames < out->frames_cap) {
    static_assert(sizeof(esvio_fe_aedat_frame) == 80 && offsetof(esvio_fe_aedat_frame, exposure_us) == 24 && offsetof(esvio_fe_aedat_frame, index) == 72,
                  "esvio_fe_aedat_frame layout");
    const uint32_t info = rd_u32(w->rec);
    esvio_fe_aedat_frame f;
    memset(&f, 0, sizeof f);
    f.stamp_sec = w->f_sec, f.stamp_nsec = w->f_nsec;
    f.ts_startframe = rd_i32(w->rec + 4), f.ts_endframe = rd_i32(w->rec + 8);
    f.ts_startexposure = rd_i32(w->rec + 12), f.ts_endexposure = rd_i32(w->rec + 16);
    f.exposure_us = (int64_t)f.ts_endexposure - (int64_t)f.ts_startexposure;
    f.length_x = rd_i32(w->rec + 20), f.length_y = rd_i32(w->rec + 24), f.position_x = rd_i32(w->rec + 28), f.position_y = rd_i32(w->rec + 32);
    f.channels = (int32_t)((info >> 1) & 7u), f.color_filter = (int32_t)((info >> 4) & 15u), f.roi = (int32_t)((info >> 8) & 127u);
    f.valid = (int32_t)(info & 1u), f.slot = (int32_t)w->slot, f.ts_overflow = w->overflow;
    f.index = out->n_frames;
    out->frames[out->n_frames] = f;
  }
  if (out->n_frames == 0) out->first_stamp[0] = w->f_sec, out->first_stamp[1] = w->f_nsec;
  out->last_stamp[0] = w->f_sec, out->last_stamp[1] = w->f_nsec;
  out->n_frames++;
  w->carry_len = 0, w->pix_left = 0, w->emit = 0;
}

// the bytes at bytes[*pos .. n) that belong to the open frame event: its head, its pixels, what lies behind them
inline bool frame_bytes(Walk* w, const uint8_t* bytes, size_t n, size_t* pos, uint32_t start_buf, int64_t t_offset_ns, uint32_t flags, Out* out) {
  if (w->ev_off < kFrameHead) {
    const size_t take = n - *pos < kFrameHead - w->ev_off ? n - *pos : kFrameHead - w->ev_off;
    memcpy(w->rec + w->ev_off, bytes + *pos, take);
    w->ev_off += (uint32_t)take, *pos += take, w->payload_left -= take;
    if (w->ev_off < kFrameHead) return true;
    if (!frame_head(w, t_offset_ns, flags, out)) return false;
  }
  if (w->pix_left) {
    if (*pos == n) return true;
    const uint64_t take = w->pix_left < n - *pos ? w->pix_left : n - *pos;
    frame_pixels(w, bytes + *pos, take, start_buf, out);
    *pos += (size_t)take, w->ev_off += (uint32_t)take, w->payload_left -= take;
    if (w->pix_left) return true;
  }
  const uint64_t rest = (uint32_t)w->ev_size - w->ev_off, skip = rest < n - *pos ? rest : n - *pos;
  *pos += (size_t)skip, w->ev_off += (uint32_t)skip, w->payload_left -= skip;
  if (w->ev_off == (uint32_t)w->ev_size) w->ev_off = 0, w->events_left--, w->slot++;
  return true;
}

// The walk: *w advanced by the n bytes at `bytes`.  Returns false at a malformed header (in the frame walk: or event, or
// a refused frame); the caller works on a copy of
// the state and takes it over when the whole call succeeds.  Reads bytes[0 .. n) and nothing else.
inline bool walk(Walk* w, Mode mode, const uint8_t* bytes, size_t n, int64_t t_offset_ns, uint32_t flags, Out* out) {
  size_t pos = 0;
  const uint32_t start_buf = w->carry_len ? w->carry_buf : w->carry_buf ^ 1u;  // the Carry buffer whose bytes count at the call's start
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
    if (w->events_left && mode == kFrames) {
      if (!frame_bytes(w, bytes, n, &pos, start_buf, t_offset_ns, flags, out)) return false;
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
