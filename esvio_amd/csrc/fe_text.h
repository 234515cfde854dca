// Text event files ("x y p t" / "t x y p" lines): what the host and the device share of the rule in include/esvio_fe.h
// "text event files".  No HIP in here: the library, the stand-alone sanitizer program of tests/test_text_host_sanitized.py
// and tools/text_seq_decode.cpp include it; compiled by hipcc the line classifier is the kernels' too (ESVIO_TEXT_HD).
//   classify      one line's body -> its class and, for an event line, the record's fields
//   State, carry  the camera's state between two calls: the unterminated tail, or "inside an overlong line"
//   decode_chunk  the rule's sequential reading of one call (the bridge the device path replaces; the sanitizer program)
//   parse_imu, parse_images   the two side files, host only
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <charconv>

#if defined(__HIPCC__)
#define ESVIO_TEXT_HD __host__ __device__ __forceinline__
#else
#define ESVIO_TEXT_HD inline
#endif

namespace esvio {
namespace text {

constexpr uint32_t kMaxBody = 64;  // a longer body is malformed
constexpr uint32_t kMaxTail = 65;  // an unterminated body and the '\r' that may belong to its terminator
constexpr int kTxyp = 1, kXypt = 2;                  // esvio_fe_text_format::order
constexpr int kSecDecimal = 1, kIntUs = 2, kIntNs = 3;  // esvio_fe_text_format::time
constexpr uint32_t kEnd = 1u, kSkipMalformed = 2u;   // esvio_fe_text_format::flags
constexpr uint64_t kTickLimit = 4294967296ull * 1000000000ull;  // sec < 2^32

enum Class { kEvent = 0, kBad = 1, kComment = 2, kBlank = 3, kMalformed = 4 };  // kBad: an event line whose stamp is BAD

struct Line {  // an event line's fields (kEvent; kBad: x, y, pol alone)
  uint32_t x, y, pol, sec, nsec;
  int64_t ticks;
};

ESVIO_TEXT_HD bool is_sep(uint8_t c) { return c == ' ' || c == '\t' || c == ','; }
ESVIO_TEXT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// the stamp token b[s, e) -> nanoseconds (*huge: beyond every stamp an offset could bring back); false: malformed
ESVIO_TEXT_HD bool stamp_token(const uint8_t* b, uint32_t s, uint32_t e, int time, uint64_t* ns, bool* huge) {
  uint64_t v = 0;
  uint32_t i = s;
  while (i < e && is_digit(b[i])) {
    if (i - s >= 19) return false;  // a 20th digit
    v = v * 10u + (uint64_t)(b[i] - '0');
    i++;
  }
  if (i == s) return false;
  *huge = false;
  if (time != kSecDecimal) {
    if (i != e) return false;
    if (time == kIntUs) {
      if (v > 0xffffffffffffffffull / 1000u) *huge = true;
      v *= 1000u;
    }
    *ns = v;
    return true;
  }
  if (i - s > 10) return false;
  uint64_t frac = 0;
  uint32_t nf = 0;
  if (i < e) {
    if (b[i] != '.') return false;
    i++;
    if (i == e) return false;
    for (; i < e; i++) {
      if (!is_digit(b[i])) return false;
      if (nf < 9) frac = frac * 10u + (uint64_t)(b[i] - '0'), nf++;  // digits behind the ninth are dropped
    }
    for (; nf < 9; nf++) frac *= 10u;
  }
  *ns = v * 1000000000ull + frac;  // < 10^19 + 10^9: inside 64 bits
  return true;
}

// ticks = ns + t_offset in exact integers (|t_offset| <= 2^62); false: BAD (ticks < 0 or sec >= 2^32)
ESVIO_TEXT_HD bool stamp_ticks(uint64_t ns, bool huge, int64_t t_offset, Line* out) {
  if (huge) return false;
  if (t_offset >= 0) {
    if (ns >= kTickLimit) return false;  // (ticks >= ns)
  } else if (ns >= kTickLimit + ((uint64_t)1 << 62)) {  // (ticks >= ns - 2^62; the bound is below 2^63)
    return false;
  }
  const int64_t ticks = (int64_t)ns + t_offset;
  if (ticks < 0 || (uint64_t)ticks >= kTickLimit) return false;
  out->ticks = ticks;
  out->sec = (uint32_t)((uint64_t)ticks / 1000000000ull);
  out->nsec = (uint32_t)((uint64_t)ticks % 1000000000ull);
  return true;
}

// One line: b[0, len) is its body (the terminator taken off).  The class, and for an event line its fields.
ESVIO_TEXT_HD int classify(const uint8_t* b, uint32_t len, int order, int time, int64_t t_offset, Line* out) {
  if (len > kMaxBody) return kMalformed;
  uint32_t i = 0, e = len;
  while (i < e && is_sep(b[i])) i++;
  while (e > i && is_sep(b[e - 1])) e--;
  if (i == e) return kBlank;
  if (b[i] == '#' || b[i] == '%') return kComment;
  uint64_t ns = 0;
  bool huge = false;
  for (int k = 0; k < 4; k++) {
    if (i == e) return kMalformed;  // fewer than four tokens
    const uint32_t s = i;
    while (i < e && !is_sep(b[i])) i++;
    const uint32_t t = i;
    while (i < e && is_sep(b[i])) i++;
    const int field = order == kTxyp ? (k + 3) & 3 : k;  // 0 x, 1 y, 2 p, 3 t
    if (field == 3) {
      if (!stamp_token(b, s, t, time, &ns, &huge)) return kMalformed;
    } else if (field == 2) {
      if (t - s == 1 && (b[s] == '0' || b[s] == '1'))
        out->pol = (uint32_t)(b[s] - '0');
      else if (t - s == 2 && b[s] == '-' && b[s + 1] == '1')
        out->pol = 0;
      else
        return kMalformed;
    } else {
      if (t - s > 5) return kMalformed;
      uint32_t v = 0;
      for (uint32_t j = s; j < t; j++) {
        if (!is_digit(b[j])) return kMalformed;
        v = v * 10u + (uint32_t)(b[j] - '0');
      }
      if (v > 65535u) return kMalformed;
      if (field == 0)
        out->x = v;
      else
        out->y = v;
    }
  }
  if (i != e) return kMalformed;  // a fifth token
  return stamp_ticks(ns, huge, t_offset, out) ? kEvent : kBad;
}

// ---- the state between two calls
struct State {
  uint8_t tail[kMaxTail] = {};  // the unterminated bytes behind the last terminator (skip: none)
  uint8_t skip = 0;             // inside a line whose body has passed 64 bytes: discarded up to its terminator
  uint32_t len = 0;
  uint64_t skip_len = 0;        // skip: the bytes of that line so far
};
// L unterminated bytes whose last one is `last`: has the body passed 64 bytes?  (A '\r' in the 65th place may still
// belong to the terminator.)
ESVIO_TEXT_HD bool overlong(uint64_t L, uint8_t last) { return L > kMaxTail || (L == kMaxTail && last != '\r'); }

// The state behind n more bytes, whatever they hold (the library hands it a whole host chunk, terminators included;
// classifying the lines those end is the caller's or the device's business): everything up to the last '\n' is gone,
// the bytes behind it are the tail — joined to the old one when the chunk holds no '\n' — or the line is overlong
inline void carry(State* st, const uint8_t* bytes, size_t n) {
  if (!n) return;
  size_t from = n;
  while (from > 0 && bytes[from - 1] != '\n') from--;
  if (from == 0 && st->skip) {
    st->skip_len += n;
    return;
  }
  const size_t rest = n - from;
  const uint64_t L = (from ? 0 : st->len) + rest;
  if (overlong(L, bytes[n - 1])) {
    st->skip = 1, st->skip_len = L, st->len = 0;
    return;
  }
  if (from) st->len = 0;
  st->skip = 0, st->skip_len = 0;
  memcpy(st->tail + st->len, bytes + from, rest);
  st->len = (uint32_t)L;
}

struct Format {
  int order, time;
  uint32_t flags;
};
struct Event {  // esvio_fe_event's bytes
  uint16_t x, y;
  uint32_t sec, nsec;
  uint8_t polarity, pad[3];
};
static_assert(sizeof(Event) == 16, "the record's layout");
struct Counts {
  uint64_t events = 0, lines = 0, comments = 0, blank = 0, malformed = 0, bad = 0;
  int64_t first_malformed = 0, first_t_ns = 0, last_t_ns = 0;
  uint32_t carried = 0;
};

// The rule's sequential reading of one call: *st advanced by the chunk, the records to dst[0, cap).  0, or -1 for a
// failure of the rule (a malformed line without kSkipMalformed, a BAD line, more events than cap): the counts are exact
// and *st is as it was.
inline int decode_chunk(State* st, const Format& f, const uint8_t* bytes, size_t n, int64_t t_offset, Event* dst, size_t cap,
                        Counts* out) {
  State s = *st;
  Counts c;
  auto line = [&](const uint8_t* body, uint32_t len, bool over, int64_t at) {
    Line l{};
    const int cls = over ? (int)kMalformed : classify(body, len, f.order, f.time, t_offset, &l);
    c.lines++;
    if (cls == kComment) c.comments++;
    if (cls == kBlank) c.blank++;
    if (cls == kMalformed && !c.malformed++) c.first_malformed = at;
    if (cls == kBad) c.bad++;
    if (cls == kEvent || cls == kBad) {
      if (c.events < cap && cls == kEvent)
        dst[c.events] = Event{(uint16_t)l.x, (uint16_t)l.y, l.sec, l.nsec, (uint8_t)l.pol, {0, 0, 0}};
      if (cls == kEvent) {
        if (!c.events) c.first_t_ns = l.ticks;
        c.last_t_ns = l.ticks;
      }
      c.events++;
    }
  };
  uint8_t buf[kMaxTail + 1];
  size_t pos = 0;
  while (pos < n) {
    const uint8_t* nl = (const uint8_t*)memchr(bytes + pos, '\n', n - pos);
    if (!nl) break;
    const size_t seg = (size_t)(nl - (bytes + pos));
    const int64_t at = (int64_t)pos - (int64_t)(s.skip ? s.skip_len : s.len);
    if (s.skip || s.len + seg > kMaxTail) {
      line(nullptr, 0, true, at);
    } else {
      memcpy(buf, s.tail, s.len);
      memcpy(buf + s.len, bytes + pos, seg);
      uint32_t len = (uint32_t)(s.len + seg);
      if (len && buf[len - 1] == '\r') len--;
      line(buf, len, false, at);
    }
    s = State();
    pos += seg + 1;
  }
  carry(&s, bytes + pos, n - pos);
  if (f.flags & kEnd) {
    if (s.skip)
      line(nullptr, 0, true, (int64_t)n - (int64_t)s.skip_len);
    else if (s.len)
      line(s.tail, s.len, false, (int64_t)n - (int64_t)s.len);
    s = State();
  }
  c.carried = s.len;
  if (out) *out = c;
  if ((c.malformed && !(f.flags & kSkipMalformed)) || c.bad || c.events > cap) return -1;
  *st = s;
  return 0;
}

// ---- the side files: imu.txt ("t ax ay az gx gy gz") and images.txt ("t path"), whole files, host only.  Lines,
// blanks and comments as in the event file; the stamp is the event file's SEC_DECIMAL token; a line of up to
// kSideMaxBody bytes.
constexpr size_t kSideMaxBody = 4096;
struct ImuSample {  // esvio_fe_imu_sample's bytes
  uint32_t sec, nsec;
  double acc[3], gyr[3];
};
// calls on_line(body, len, line_begin) for every line that is neither blank nor a comment; false from it ends the walk
template <class F>
inline bool side_lines(const uint8_t* bytes, size_t n, F on_line) {
  size_t pos = 0;
  while (pos < n) {
    const uint8_t* nl = (const uint8_t*)memchr(bytes + pos, '\n', n - pos);
    size_t end = nl ? (size_t)(nl - bytes) : n;
    const size_t next = nl ? end + 1 : n;
    if (nl && end > pos && bytes[end - 1] == '\r') end--;
    size_t i = pos;
    while (i < end && is_sep(bytes[i])) i++;
    while (end > i && is_sep(bytes[end - 1])) end--;
    if (i < end && bytes[i] != '#' && bytes[i] != '%')
      if (end - i > kSideMaxBody || !on_line(bytes + i, end - i, i)) return false;
    pos = next;
  }
  return true;
}
inline bool side_stamp(const uint8_t* b, size_t len, int64_t t_offset, Line* l) {
  uint64_t ns;
  bool huge;
  return len <= 64 && stamp_token(b, 0, (uint32_t)len, kSecDecimal, &ns, &huge) && stamp_ticks(ns, huge, t_offset, l);
}
// 0; -1: a line that does not read (*n_out: the samples in front of it); -2: more samples than cap (*n_out: the number needed)
inline int parse_imu(const uint8_t* bytes, size_t n, int64_t t_offset, ImuSample* out, size_t cap, size_t* n_out) {
  size_t cnt = 0;
  const bool ok = side_lines(bytes, n, [&](const uint8_t* b, size_t len, size_t) {
    ImuSample smp{};
    size_t i = 0;
    for (int k = 0; k < 7; k++) {
      if (i == len) return false;
      const size_t s = i;
      while (i < len && !is_sep(b[i])) i++;
      const size_t t = i;
      while (i < len && is_sep(b[i])) i++;
      if (k == 0) {
        Line l{};
        if (!side_stamp(b + s, t - s, t_offset, &l)) return false;
        smp.sec = l.sec, smp.nsec = l.nsec;
        continue;
      }
      double v = 0;
      const char* first = (const char*)b + s;
      const char* last = (const char*)b + t;
      if (*first == '+') return false;
      const auto r = std::from_chars(first, last, v);  // locale-independent, the nearest double
      if (r.ec != std::errc() || r.ptr != last) return false;
      (k <= 3 ? smp.acc[k - 1] : smp.gyr[k - 4]) = v;
    }
    if (i != len) return false;
    if (cnt < cap) out[cnt] = smp;
    cnt++;
    return true;
  });
  *n_out = cnt;
  return !ok ? -1 : cnt > cap ? -2 : 0;
}
// stamps[i]: ticks in nanoseconds; the path is bytes[path_off[i], + path_len[i]): what follows the stamp and its blanks
// (spaces and tabs), up to the line's end without trailing separators
inline int parse_images(const uint8_t* bytes, size_t n, int64_t t_offset, int64_t* stamps, uint64_t* path_off, uint32_t* path_len,
                        size_t cap, size_t* n_out) {
  size_t cnt = 0;
  const bool ok = side_lines(bytes, n, [&](const uint8_t* b, size_t len, size_t begin) {
    size_t i = 0;
    while (i < len && b[i] != ' ' && b[i] != '\t') i++;
    Line l{};
    if (!side_stamp(b, i, t_offset, &l)) return false;
    while (i < len && (b[i] == ' ' || b[i] == '\t')) i++;
    if (i == len) return false;
    if (cnt < cap) stamps[cnt] = l.ticks, path_off[cnt] = begin + i, path_len[cnt] = (uint32_t)(len - i);
    cnt++;
    return true;
  });
  *n_out = cnt;
  return !ok ? -1 : cnt > cap ? -2 : 0;
}

}  // namespace text
}  // namespace esvio
