// fe_bag.h — the host walk over a rosbag v2.0 record stream (include/esvio_fe.h has the rule).
// No HIP in here: inline functions over a plain state struct, so that the library, the test tap, the stand-alone
// sanitizer program and tools/bag_seq_decode.cpp all run the same lines.
//
// A bag is a chain of records, each of which says how long it is, so it is walked on the host.  The event walk gathers
// the 13-byte wire events of the chunk's EventArray messages, and nothing else, densely per camera and lists the
// messages it completes; the side walk decodes the Imu messages where they lie: they are few.  Whatever is cut by the
// call's end — a length word, a header, a message's fixed part, an event — waits in the state.  The image walk gathers the
// pixel payloads of the sensor_msgs/Image messages of its two topics, each at a 16-byte boundary, and lists them; the
// bytes of a payload that the call's end cuts wait in a carry buffer beside the state (Carry), which may be megabytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/esvio_fe.h"

namespace esvio {
namespace bag {

constexpr uint32_t kMagicBytes = 13, kMaxHeader = 4096, kMaxValue = 255, kMaxConns = 64, kEventBytes = 13, kImuBody = 296;
constexpr uint32_t kFieldKeep = 9 + kMaxValue;  // the bytes of a connection field that are looked at: "md5sum=" + a value, with room
constexpr char kMagic[] = "#ROSBAG V2.0\n";
constexpr char kEventType[] = "dvs_msgs/EventArray", kEventMd5[] = "5e8beee5a6c107e504c2e78903c224b8", kImuType[] = "sensor_msgs/Imu";
constexpr char kImageType[] = "sensor_msgs/Image";
constexpr uint32_t kMaxEncoding = 32;  // bytes of an Image message's encoding string
constexpr uint32_t kImageFixed = 37;   // an Image message without frame_id, encoding and data: 16 + 12 + 1 + 4 + 4
enum Role { kNone = 0, kLeft = 1, kRight = 2, kImu = 3, kImgLeft = 4, kImgRight = 5 };
enum EncodingClass { kEncNone = 0, kEncMono = 1, kEncBgr = 2, kEncRgb = 3 };  // esvio_fe_bag_image::encoding
inline bool is_image_role(uint32_t role) { return role == kImgLeft || role == kImgRight; }
inline uint32_t encoding_bpp(int cls) { return cls == kEncMono ? 1u : 3u; }
// getImageFromMsg's accepted encodings (stereo_image_tracker_node.cpp:261-307) -> the class, kEncNone: every other string
inline int encoding_class(const uint8_t* s, uint32_t n) {
  const struct {
    const char* name;
    int cls;
  } known[] = {{"mono8", kEncMono}, {"8UC1", kEncMono}, {"bgr8", kEncBgr}, {"8UC3", kEncBgr}, {"rgb8", kEncRgb}};
  for (const auto& k : known)
    if (n == strlen(k.name) && memcmp(s, k.name, n) == 0) return k.cls;
  return kEncNone;
}

// role - 1 -> the topic (len 0: none).  0..2: esvio_fe_bag_set_topics', read by the event and the side walk; 3..4:
// esvio_fe_bag_set_image_topics', read by the image walk.
struct Topics {
  uint32_t len[5] = {0, 0, 0, 0, 0};
  char name[5][kMaxValue + 1] = {};
};

// esvio_fe_bag_set_topics' check and copy; false: *why says which rule `in` breaks (null `in`: no topic has a role)
inline bool set_topics(const esvio_fe_bag_topics* in, Topics* out, const char** why) {
  Topics t;
  for (int r = 3; r < 5; r++) t.len[r] = out->len[r], memcpy(t.name[r], out->name[r], sizeof t.name[r]);  // (the image topics stay)
  const char* src[3] = {in ? in->left : nullptr, in ? in->right : nullptr, in ? in->imu : nullptr};
  for (int r = 0; r < 3; r++) {
    if (!src[r]) continue;
    const size_t n = strlen(src[r]);
    if (n == 0 || n > kMaxValue) return *why = "a topic must hold 1 to 255 bytes", false;
    for (int q = 0; q < r; q++)
      if (t.len[q] == n && memcmp(t.name[q], src[r], n) == 0) return *why = "two roles name the same topic", false;
    t.len[r] = (uint32_t)n;
    memcpy(t.name[r], src[r], n);
  }
  *out = t;
  return true;
}
// esvio_fe_bag_set_image_topics' check and copy: the same string rules, and no image topic may be one that has a role
// from set_topics
inline bool set_image_topics(const char* left, const char* right, Topics* out, const char** why) {
  Topics t = *out;
  const char* src[2] = {left, right};
  for (int r = 0; r < 2; r++) {
    t.len[3 + r] = 0;
    memset(t.name[3 + r], 0, sizeof t.name[3 + r]);
    if (!src[r]) continue;
    const size_t n = strlen(src[r]);
    if (n == 0 || n > kMaxValue) return *why = "a topic must hold 1 to 255 bytes", false;
    for (int q = 0; q < 3 + r; q++)
      if (t.len[q] == n && memcmp(t.name[q], src[r], n) == 0)
        return *why = q < 3 ? "an image topic that has a role from esvio_fe_bag_set_topics" : "two roles name the same topic", false;
    t.len[3 + r] = (uint32_t)n;
    memcpy(t.name[3 + r], src[r], n);
  }
  *out = t;
  return true;
}

// the phases: what the next bytes are.  C: collected into buf until `need`; S: `left` bytes passed over
enum Phase {
  P_HLEN = 0,  // C 4   header_len
  P_HDR,       // C     the header
  P_DLEN,      // C 4   data_len
  P_SKIP,      // S     data nobody reads
  P_CFLEN,     // C 4   a connection field's length
  P_CFIELD,    // C     its first kFieldKeep bytes at the most
  P_CFSKIP,    // S     the rest of it
  P_MHEAD,     // C 16  seq, stamp, L
  P_MFRAME,    // S     frame_id
  P_MEVHEAD,   // C 12  height, width, n
  P_MEVENTS,   //       whole events where they lie
  P_MCARRY,    // C 13  an event the call's end cut
  P_MIMU,      // C 296 the Imu body
  P_MIMHEAD,   // C 12  an Image message's height, width, Le
  P_MIMENC,    // C     its encoding, is_bigendian, step, D: Le + 9 bytes
  P_MIMDATA,   //       its pixel payload where it lies
};

struct Conn {
  uint32_t id, role;
};

// One walker's state (a handle has three: the event call's, the side call's and the image call's).  All zero is the
// fresh state.
struct Walk {
  uint32_t phase, need, have;
  uint64_t left;        // S phases: bytes still to pass over
  uint64_t data_left;   // bytes of the open record's data still to come
  uint64_t chunk_left;  // bytes of the open chunk still to come
  uint32_t in_chunk;
  uint32_t op, conn, t_sec, t_nsec, role;  // the open record (role: of a connection record's topic, or of a message's conn)
  uint32_t c_type, c_md5;                  // the open connection record: type / md5sum seen and right
  uint64_t cf_rest;                        // ... the bytes of the open field behind the kept ones
  uint32_t seq, st_sec, st_nsec, height, width;  // the open message
  uint64_t data_len, frame_len, ev_left, msg_first, msg_count;
  uint64_t emitted[2];  // events emitted per camera since the last reset
  uint32_t step, enc, bigendian;  // the open Image message (its payload bytes still to come: ev_left)
  uint32_t carry_buf;             // ... which of the Carry's two buffers holds its bytes so far
  uint64_t carry_len;             // ... and how many they are
  uint32_t n_conn;
  Conn conns[kMaxConns];
  uint8_t buf[kMaxHeader];
};

inline uint32_t rd_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd_u64(const uint8_t* p) { return (uint64_t)rd_u32(p) | (uint64_t)rd_u32(p + 4) << 32; }

enum Mode { kEvents = 0, kSide = 1, kImages = 2 };

// The bytes of an Image payload that a call's end cut, beside the image walker's state (Walk::carry_buf, carry_len say
// which buffer and how much of it counts).  Two buffers: a call whose first message was waiting in one puts what it
// leaves waiting into the other, so a call that fails after its gathering walk has overwritten nothing of the state it
// goes back to.  A payload still open at the call's end grows in place, behind the bytes that count.
struct Carry {
  std::vector<uint8_t> buf[2];
};

// What one walk call produces.  Pointers may be null: the walk then counts only.
struct Out {
  // the event walk
  uint8_t* payload[2] = {nullptr, nullptr};  // room for events_cap[cam] 13-byte wire events
  size_t events_cap[2] = {0, 0};
  esvio_fe_bag_message* msgs = nullptr;
  size_t msgs_cap = 0;
  uint64_t n_events[2] = {0, 0}, n_cam_msgs[2] = {0, 0}, n_msgs = 0;  // counted whether stored or not
  // the side walk
  esvio_fe_imu_sample* imu = nullptr;
  size_t imu_cap = 0;
  uint64_t n_imu = 0, bad = 0;
  // the image walk: want_w x want_h the only size taken (0: any); pix null: counted only; carry null: nothing waits
  uint32_t want_w = 0, want_h = 0;
  Carry* carry = nullptr;
  uint8_t* pix = nullptr;  // room for pix_cap bytes: the completed messages' payloads, each from a 16-byte boundary
  size_t pix_cap = 0;
  esvio_fe_bag_image* imgs = nullptr;
  size_t imgs_cap = 0;
  uint64_t n_pix_bytes = 0, n_imgs = 0, n_cam_imgs[2] = {0, 0};  // counted whether stored or not
  uint32_t first_stamp[2][2] = {}, last_stamp[2][2] = {};        // per camera (sec, nsec) of its first / last completed message
  // all
  uint64_t other_messages = 0, other_records = 0, chunks = 0, connections = 0;
  const char* why = nullptr;  // a malformed stream: which rule it breaks
  char why_buf[400];
};

// a field "name=value" of n bytes at p: is its name `name`?  *v, *vn: the value
inline bool field_is(const uint8_t* p, uint32_t n, const char* name, const uint8_t** v, uint32_t* vn) {
  const size_t k = strlen(name);
  if (n < k + 1 || memcmp(p, name, k) != 0 || p[k] != '=') return false;
  *v = p + k + 1, *vn = n - (uint32_t)k - 1;
  return true;
}

// the fields of a record header
struct Header {
  int op = -1;
  bool has_conn = false, has_time = false, has_topic = false, has_size = false, has_compression = false;
  bool has_index_pos = false, has_conn_count = false, has_chunk_count = false;
  uint32_t conn = 0, t_sec = 0, t_nsec = 0, size = 0, conn_count = 0, chunk_count = 0, topic_len = 0, compression_len = 0;
  uint64_t index_pos = 0;
  const uint8_t *topic = nullptr, *compression = nullptr;
};
// false: malformed (*why says how).  A fixed-size field of another length leaves its has_ flag false: it is malformed
// where the op needs it.
inline bool parse_header(const uint8_t* h, uint32_t n, Header* out, const char** why) {
  uint32_t pos = 0;
  while (pos < n) {
    if (n - pos < 4) return *why = "a field overruns its header", false;
    const uint32_t fl = rd_u32(h + pos);
    pos += 4;
    if (fl > n - pos) return *why = "a field overruns its header", false;
    const uint8_t* f = h + pos;
    pos += fl;
    if (!memchr(f, '=', fl)) return *why = "a header field without '='", false;
    const uint8_t* v;
    uint32_t vn;
    if (field_is(f, fl, "op", &v, &vn)) {
      if (vn != 1) return *why = "an op field that is not 1 byte long", false;
      out->op = v[0];
    } else if (field_is(f, fl, "conn", &v, &vn)) {
      out->has_conn = vn == 4;
      if (vn == 4) out->conn = rd_u32(v);
    } else if (field_is(f, fl, "time", &v, &vn)) {
      out->has_time = vn == 8;
      if (vn == 8) out->t_sec = rd_u32(v), out->t_nsec = rd_u32(v + 4);
    } else if (field_is(f, fl, "topic", &v, &vn)) {
      out->has_topic = true, out->topic = v, out->topic_len = vn;
    } else if (field_is(f, fl, "size", &v, &vn)) {
      out->has_size = vn == 4;
      if (vn == 4) out->size = rd_u32(v);
    } else if (field_is(f, fl, "compression", &v, &vn)) {
      out->has_compression = true, out->compression = v, out->compression_len = vn;
    } else if (field_is(f, fl, "index_pos", &v, &vn)) {
      out->has_index_pos = vn == 8;
      if (vn == 8) out->index_pos = rd_u64(v);
    } else if (field_is(f, fl, "conn_count", &v, &vn)) {
      out->has_conn_count = vn == 4;
      if (vn == 4) out->conn_count = rd_u32(v);
    } else if (field_is(f, fl, "chunk_count", &v, &vn)) {
      out->has_chunk_count = vn == 4;
      if (vn == 4) out->chunk_count = rd_u32(v);
    }
  }
  if (out->op < 0) return *why = "a header without op", false;
  return true;
}
inline bool bag_header_fields(const Header& h, const char** why) {
  if (!h.has_index_pos || !h.has_conn_count || !h.has_chunk_count)
    return *why = "a bag header record without index_pos (8 bytes), conn_count or chunk_count (4 bytes)", false;
  return true;
}

inline uint32_t topic_role(const Topics& t, Mode mode, const uint8_t* topic, uint32_t n) {
  for (uint32_t r = mode == kImages ? 3 : 0; r < (mode == kImages ? 5u : 3u); r++)
    if (t.len[r] && t.len[r] == n && memcmp(t.name[r], topic, n) == 0) return r + 1;
  return kNone;
}
inline int find_conn(const Walk& w, uint32_t id) {
  for (uint32_t k = 0; k < w.n_conn; k++)
    if (w.conns[k].id == id) return (int)k;
  return -1;
}
inline void collect(Walk* w, uint32_t phase, uint32_t need) { w->phase = phase, w->need = need, w->have = 0; }
inline void skip(Walk* w, uint32_t phase, uint64_t n) { w->phase = phase, w->left = n; }
inline bool malformed(Out* out, const char* why) { return out->why = why, false; }
inline bool malformed_topic(Out* out, const char* what, const Topics& t, uint32_t role) {
  snprintf(out->why_buf, sizeof out->why_buf, "%s on topic %s", what, t.name[role - 1]);
  return out->why = out->why_buf, false;
}

// a record's last data byte is behind us: the next record, or the chunk's end
inline bool next_record(Walk* w, Out* out) {
  if (w->in_chunk) {
    if (w->chunk_left == 0)
      w->in_chunk = 0;
    else if (w->chunk_left < 4)
      return malformed(out, "a record overruns its chunk");
  }
  collect(w, P_HLEN, 4);
  return true;
}

// a complete header and data_len: the record is open
inline bool open_record(Walk* w, const Topics& topics, Mode mode, Out* out) {
  const uint64_t dl = w->data_len;
  if (w->in_chunk) {
    if (w->op != 2 && w->op != 7) return malformed(out, "a record inside a chunk that is neither message data nor a connection");
    if (dl > w->chunk_left) return malformed(out, "a record overruns its chunk");
  }
  w->data_left = dl;
  switch (w->op) {
    case 5:
      out->chunks++;
      w->in_chunk = 1, w->chunk_left = dl, w->data_left = 0;
      return next_record(w, out);
    case 7:
      w->c_type = w->c_md5 = 0;
      if (dl == 0) break;
      if (dl < 4) return malformed(out, "a field overruns its connection data");
      collect(w, P_CFLEN, 4);
      return true;
    case 2: {
      const int k = find_conn(*w, w->conn);
      w->role = k < 0 ? (uint32_t)kNone : w->conns[k].role;
      if (w->role == kNone) {
        out->other_messages++;
        skip(w, P_SKIP, dl);
        return true;
      }
      if (is_image_role(w->role) && dl < kImageFixed + 1)
        return malformed_topic(out, "an Image message whose data_len is not 37 + L + Le + D", topics, w->role);
      if (dl < (w->role == kImu ? 16 + kImuBody : 28))
        return malformed_topic(out, w->role == kImu ? "an Imu message whose data_len is not 16 + L + 296" : "an EventArray message whose data_len is not 28 + L + 13 n", topics, w->role);
      collect(w, P_MHEAD, 16);
      return true;
    }
    case 3:
    case 4:
    case 6:
      skip(w, P_SKIP, dl);
      return true;
    default:
      out->other_records++;
      skip(w, P_SKIP, dl);
      return true;
  }
  // (a connection record without data)
  w->phase = P_CFSKIP, w->left = 0;
  return true;
}

// the open connection record's last data byte is behind us
inline bool close_conn(Walk* w, const Topics& topics, Out* out) {
  out->connections++;
  const int k = find_conn(*w, w->conn);
  if (k >= 0 && w->conns[k].role != w->role) return malformed(out, "a repeated conn id with another topic");
  if (w->role != kNone) {
    if (!w->c_type)
      return malformed_topic(out, is_image_role(w->role) ? "a connection whose type is not sensor_msgs/Image" : w->role == kImu ? "a connection whose type is not sensor_msgs/Imu" : "a connection whose type is not dvs_msgs/EventArray", topics, w->role);
    if ((w->role == kLeft || w->role == kRight) && !w->c_md5) return malformed_topic(out, "a connection whose md5sum is not dvs_msgs/EventArray's (5e8beee5a6c107e504c2e78903c224b8)", topics, w->role);
    if (k < 0) {
      if (w->n_conn == kMaxConns) return malformed(out, "more than 64 connections with a role");
      w->conns[w->n_conn++] = Conn{w->conn, w->role};
    }
  }
  return next_record(w, out);
}

inline void close_message(Walk* w, Mode mode, Out* out) {
  const int cam = (int)w->role - 1;
  if (mode == kEvents) {
    if (out->msgs && out->n_msgs < out->msgs_cap) {
      esvio_fe_bag_message m;
      memset(&m, 0, sizeof m);
      m.cam = cam, m.seq = w->seq, m.stamp_sec = w->st_sec, m.stamp_nsec = w->st_nsec, m.time_sec = w->t_sec, m.time_nsec = w->t_nsec;
      m.height = w->height, m.width = w->width, m.first = w->msg_first, m.count = w->msg_count;
      out->msgs[out->n_msgs] = m;
    }
    out->n_msgs++, out->n_cam_msgs[cam]++;
  }
}

// `take` bytes of the open Image message's payload at p.  The message's last ones: the payload, the waiting bytes in
// front, goes to out->pix at the next 16-byte boundary and the message is listed.  Else the call ends inside it: they wait.
inline void take_pixels(Walk* w, const uint8_t* p, uint64_t take, uint32_t start_buf, Out* out) {
  if (take < w->ev_left) {
    if (w->carry_len == 0) w->carry_buf = start_buf ^ 1u;  // (never the buffer the call's first message waited in)
    if (out->carry) {
      std::vector<uint8_t>& b = out->carry->buf[w->carry_buf];
      if (b.size() < w->carry_len + take) b.resize((size_t)(w->carry_len + take));
      memcpy(b.data() + w->carry_len, p, (size_t)take);
    }
    w->carry_len += take, w->ev_left -= take;
    return;
  }
  const int cam = (int)w->role - (int)kImgLeft;
  const uint64_t total = w->carry_len + take;
  if (out->pix && out->carry && out->n_pix_bytes + total <= out->pix_cap) {
    if (w->carry_len) memcpy(out->pix + out->n_pix_bytes, out->carry->buf[w->carry_buf].data(), (size_t)w->carry_len);
    memcpy(out->pix + out->n_pix_bytes + w->carry_len, p, (size_t)take);
  }
  out->n_pix_bytes += (total + 15) & ~(uint64_t)15;
  if (out->imgs && out->n_imgs < out->imgs_cap) {
    // the row as its 14 words, so that the padding word in front of `index` is 0 too: a row is compared byte for byte
    static_assert(sizeof(esvio_fe_bag_image) == 56 && offsetof(esvio_fe_bag_image, is_bigendian) == 40 && offsetof(esvio_fe_bag_image, index) == 48,
                  "esvio_fe_bag_image layout");
    const uint64_t index = out->n_cam_imgs[cam];
    const uint32_t row[14] = {(uint32_t)cam, w->seq, w->st_sec, w->st_nsec, w->t_sec, w->t_nsec, w->height, w->width, w->step, w->enc, w->bigendian, 0u,
                              (uint32_t)index, (uint32_t)(index >> 32)};
    memcpy(&out->imgs[out->n_imgs], row, sizeof row);
  }
  if (out->n_cam_imgs[cam] == 0) out->first_stamp[cam][0] = w->st_sec, out->first_stamp[cam][1] = w->st_nsec;
  out->last_stamp[cam][0] = w->st_sec, out->last_stamp[cam][1] = w->st_nsec;
  out->n_imgs++, out->n_cam_imgs[cam]++;
  w->carry_len = 0, w->ev_left = 0;
}

// `count` whole wire events of the open message at p
inline void take_events(Walk* w, Mode mode, const uint8_t* p, uint64_t count, Out* out) {
  const int cam = (int)w->role - 1;
  if (mode == kEvents) {
    if (out->payload[cam] && out->n_events[cam] + count <= out->events_cap[cam])
      memcpy(out->payload[cam] + out->n_events[cam] * kEventBytes, p, (size_t)count * kEventBytes);
    out->n_events[cam] += count;
  }
  w->emitted[cam] += count, w->ev_left -= count;
}

// a collect phase has its bytes: what they say, and what comes next.  false: malformed
inline bool collected(Walk* w, const Topics& topics, Mode mode, Out* out) {
  const uint8_t* b = w->buf;
  switch (w->phase) {
    case P_HLEN: {
      const uint32_t hl = rd_u32(b);
      if (hl > kMaxHeader) return malformed(out, "header_len > 4096");
      if (w->in_chunk && (uint64_t)hl + 4 > w->chunk_left) return malformed(out, "a record overruns its chunk");
      collect(w, P_HDR, hl);
      return true;
    }
    case P_HDR: {
      Header h;
      const char* why = nullptr;
      if (!parse_header(b, w->need, &h, &why)) return malformed(out, why);
      w->op = (uint32_t)h.op, w->conn = h.conn, w->t_sec = h.t_sec, w->t_nsec = h.t_nsec, w->role = kNone;
      if (h.op == 3 && !bag_header_fields(h, &why)) return malformed(out, why);
      if (h.op == 5) {
        if (!h.has_compression || !h.has_size) return malformed(out, "a chunk record without compression or size (4 bytes)");
        if (h.compression_len != 4 || memcmp(h.compression, "none", 4) != 0)
          return malformed(out, "a compressed chunk: run `rosbag decompress` on the bag first (only compression=none is read)");
        w->seq = h.size;  // (kept until data_len is known)
      }
      if (h.op == 7) {
        if (!h.has_conn || !h.has_topic) return malformed(out, "a connection record without conn (4 bytes) or topic");
        if (h.topic_len > kMaxValue) return malformed(out, "a topic longer than 255 bytes");
        w->role = topic_role(topics, mode, h.topic, h.topic_len);
      }
      if (h.op == 2 && (!h.has_conn || !h.has_time)) return malformed(out, "a message record without conn (4 bytes) or time (8 bytes)");
      collect(w, P_DLEN, 4);
      return true;
    }
    case P_DLEN:
      w->data_len = rd_u32(b);
      if (w->op == 5 && w->seq != w->data_len) return malformed(out, "a chunk whose size differs from its data_len");
      return open_record(w, topics, mode, out);
    case P_CFLEN: {
      const uint32_t fl = rd_u32(b);
      if (fl > w->data_left) return malformed(out, "a field overruns its connection data");
      const uint32_t keep = fl < kFieldKeep ? fl : kFieldKeep;
      w->cf_rest = fl - keep;
      collect(w, P_CFIELD, keep);
      return true;
    }
    case P_CFIELD: {
      if (!memchr(b, '=', w->need)) return malformed(out, "a connection field without '='");
      const uint8_t* v;
      uint32_t vn;
      if (w->role != kNone && field_is(b, w->need, "type", &v, &vn)) {
        const char* want = is_image_role(w->role) ? kImageType : w->role == kImu ? kImuType : kEventType;
        w->c_type = w->cf_rest == 0 && vn == strlen(want) && memcmp(v, want, vn) == 0;
      } else if ((w->role == kLeft || w->role == kRight) && field_is(b, w->need, "md5sum", &v, &vn)) {
        w->c_md5 = w->cf_rest == 0 && vn == strlen(kEventMd5) && memcmp(v, kEventMd5, vn) == 0;
      }
      skip(w, P_CFSKIP, w->cf_rest);
      return true;
    }
    case P_MHEAD: {
      w->seq = rd_u32(b), w->st_sec = rd_u32(b + 4), w->st_nsec = rd_u32(b + 8), w->frame_len = rd_u32(b + 12);
      if (is_image_role(w->role)) {
        if (w->frame_len > w->data_len - (kImageFixed + 1)) return malformed_topic(out, "an Image message whose data_len is not 37 + L + Le + D", topics, w->role);
      } else if (w->role == kImu) {
        if (w->data_len != 16 + w->frame_len + kImuBody) return malformed_topic(out, "an Imu message whose data_len is not 16 + L + 296", topics, w->role);
      } else if (w->frame_len > w->data_len - 28) {
        return malformed_topic(out, "an EventArray message whose data_len is not 28 + L + 13 n", topics, w->role);
      }
      skip(w, P_MFRAME, w->frame_len);
      return true;
    }
    case P_MEVHEAD: {
      w->height = rd_u32(b), w->width = rd_u32(b + 4);
      const uint64_t n = rd_u32(b + 8);
      if (w->data_len != 28 + w->frame_len + kEventBytes * n) return malformed_topic(out, "an EventArray message whose data_len is not 28 + L + 13 n", topics, w->role);
      w->ev_left = w->msg_count = n, w->msg_first = w->emitted[w->role - 1];
      w->phase = P_MEVENTS;
      return true;
    }
    case P_MIMHEAD: {
      w->height = rd_u32(b), w->width = rd_u32(b + 4);
      const uint32_t le = rd_u32(b + 8);
      if (le > kMaxEncoding) return malformed_topic(out, "an Image message whose encoding is longer than 32 bytes", topics, w->role);
      if (le > w->data_len - (kImageFixed + 1) - w->frame_len) return malformed_topic(out, "an Image message whose data_len is not 37 + L + Le + D", topics, w->role);
      if (w->height == 0 || w->width == 0) return malformed_topic(out, "an Image message with height or width 0", topics, w->role);
      collect(w, P_MIMENC, le + 9);
      return true;
    }
    case P_MIMENC: {
      const uint32_t le = w->need - 9;
      w->bigendian = b[le], w->step = rd_u32(b + le + 1);
      const uint64_t d = rd_u32(b + le + 5);
      if (d != (uint64_t)w->step * w->height) return malformed_topic(out, "an Image message whose data length is not step * height", topics, w->role);
      if (w->data_len != kImageFixed + w->frame_len + le + d) return malformed_topic(out, "an Image message whose data_len is not 37 + L + Le + D", topics, w->role);
      w->enc = (uint32_t)encoding_class(b, le);
      if (w->enc == kEncNone) {
        char name[kMaxEncoding + 1];
        for (uint32_t k = 0; k < le; k++) name[k] = b[k] >= 0x20 && b[k] < 0x7f ? (char)b[k] : '?';
        name[le] = 0;
        snprintf(out->why_buf, sizeof out->why_buf, "an Image message with encoding \"%s\" on topic %s: mono8, 8UC1, bgr8, 8UC3 and rgb8 are taken", name,
                 topics.name[w->role - 1]);
        return out->why = out->why_buf, false;
      }
      if (w->step < (uint64_t)w->width * encoding_bpp((int)w->enc)) return malformed_topic(out, "an Image message whose step is below width * bytes per pixel", topics, w->role);
      if (out->want_w && (w->width != out->want_w || w->height != out->want_h)) {
        snprintf(out->why_buf, sizeof out->why_buf, "an Image message of %u x %u on topic %s, the handle's size is %u x %u: cv::resize is out of scope",
                 w->width, w->height, topics.name[w->role - 1], out->want_w, out->want_h);
        return out->why = out->why_buf, false;
      }
      w->ev_left = d, w->carry_len = 0;
      w->phase = P_MIMDATA;
      return true;
    }
    case P_MCARRY:
      take_events(w, mode, b, 1, out);
      w->phase = P_MEVENTS;
      return true;
    case P_MIMU: {
      if (mode == kSide) {
        if (w->st_nsec >= 1000000000u) {
          out->bad++;
        } else {
          if (out->imu && out->n_imu < out->imu_cap) {
            esvio_fe_imu_sample s;
            memset(&s, 0, sizeof s);
            s.sec = w->st_sec, s.nsec = w->st_nsec;
            memcpy(s.gyr, b + 104, 24);  // behind orientation (32) and its covariance (72)
            memcpy(s.acc, b + 200, 24);  // behind angular_velocity (24) and its covariance (72)
            out->imu[out->n_imu] = s;
          }
          out->n_imu++;
        }
      }
      return next_record(w, out);
    }
  }
  return malformed(out, "(the walker's state is not one of its phases)");
}

// a skip phase is through
inline bool skipped(Walk* w, const Topics& topics, Mode mode, Out* out) {
  switch (w->phase) {
    case P_SKIP:
      return next_record(w, out);
    case P_CFSKIP:
      if (w->data_left == 0) return close_conn(w, topics, out);
      if (w->data_left < 4) return malformed(out, "a field overruns its connection data");
      collect(w, P_CFLEN, 4);
      return true;
    case P_MFRAME:
      if (is_image_role(w->role)) {
        collect(w, P_MIMHEAD, 12);
      } else if (w->role == kImu) {
        if (mode == kSide)
          collect(w, P_MIMU, kImuBody);
        else
          skip(w, P_SKIP, kImuBody);
      } else {
        collect(w, P_MEVHEAD, 12);
      }
      return true;
  }
  return malformed(out, "(the walker's state is not one of its phases)");
}

inline void consumed(Walk* w, uint64_t n) {
  if (w->in_chunk) w->chunk_left -= n;
  if (w->phase >= P_SKIP) w->data_left -= n;
}

// The walk: *w advanced by the n bytes at `bytes`.  Returns false at a malformed stream (out->why says how); the caller
// works on a copy of the state and takes it over when the whole call succeeds.  Reads bytes[0 .. n) and nothing else.
inline bool walk(Walk* w, const Topics& topics, Mode mode, const uint8_t* bytes, size_t n, Out* out) {
  size_t pos = 0;
  const uint32_t start_buf = w->carry_len ? w->carry_buf : w->carry_buf ^ 1u;  // the Carry buffer whose bytes count at the call's start
  if (w->phase == P_HLEN && w->need == 0) w->need = 4;  // the fresh state
  for (;;) {
    switch (w->phase) {
      case P_SKIP:
      case P_CFSKIP:
      case P_MFRAME: {
        if (w->left) {
          if (pos == n) return true;
          const uint64_t take = w->left < n - pos ? w->left : n - pos;
          pos += (size_t)take, w->left -= take;
          consumed(w, take);
          if (w->left) return true;
        }
        if (!skipped(w, topics, mode, out)) return false;
        break;
      }
      case P_MEVENTS: {
        if (w->ev_left == 0) {
          close_message(w, mode, out);
          if (!next_record(w, out)) return false;
          break;
        }
        if (pos == n) return true;
        const uint64_t fit = (n - pos) / kEventBytes, whole = fit < w->ev_left ? fit : w->ev_left;
        if (whole) {
          take_events(w, mode, bytes + pos, whole, out);
          pos += (size_t)(whole * kEventBytes);
          consumed(w, whole * kEventBytes);
        } else {
          collect(w, P_MCARRY, kEventBytes);  // fewer bytes than an event: they wait
        }
        break;
      }
      case P_MIMDATA: {
        if (pos == n) return true;
        const uint64_t take = w->ev_left < n - pos ? w->ev_left : n - pos;
        take_pixels(w, bytes + pos, take, start_buf, out);
        pos += (size_t)take;
        consumed(w, take);
        if (w->ev_left) return true;
        if (!next_record(w, out)) return false;
        break;
      }
      default: {  // the collect phases
        if (w->have < w->need) {
          if (pos == n) return true;
          const size_t take = n - pos < w->need - w->have ? n - pos : w->need - w->have;
          memcpy(w->buf + w->have, bytes + pos, take);
          w->have += (uint32_t)take, pos += take;
          consumed(w, take);
          if (w->have < w->need) return true;
        }
        if (!collected(w, topics, mode, out)) return false;
        break;
      }
    }
  }
}

// ---- the magic and the bag header record (host only; the rule: include/esvio_fe.h) ----
inline int file_header(const void* bytes, size_t n, esvio_fe_bag_header_info* out) {
  if (!out || (n && !bytes)) return ESVIO_FE_EINVAL;
  memset(out, 0, sizeof *out);
  const uint8_t* b = (const uint8_t*)bytes;
  const size_t m = n < kMagicBytes ? n : kMagicBytes;
  if (m && memcmp(b, kMagic, m) != 0) return ESVIO_FE_EINVAL;
  if (n < kMagicBytes) return 0;
  out->payload_offset = kMagicBytes, out->version = 20;
  if (n - kMagicBytes < 4) return 0;
  const uint32_t hl = rd_u32(b + kMagicBytes);
  if (hl > kMaxHeader) return ESVIO_FE_EINVAL;
  if (n - kMagicBytes - 4 < (size_t)hl + 4) return 0;
  Header h;
  const char* why = nullptr;
  if (!parse_header(b + kMagicBytes + 4, hl, &h, &why) || h.op != 3 || !bag_header_fields(h, &why)) return ESVIO_FE_EINVAL;
  out->index_pos = h.index_pos, out->conn_count = h.conn_count, out->chunk_count = h.chunk_count, out->complete = 1;
  return 0;
}

}  // namespace bag
}  // namespace esvio
