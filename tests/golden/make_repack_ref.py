#!/usr/bin/env python3
"""Regenerates tests/golden/repack_ref_*.npz: the messages the REFERENCE'S OWN compiled re-chunking tool writes for
small event streams.

Run by hand on a machine that has the reference tree, never by a test:

    python tests/golden/make_repack_ref.py <reference>/dependences/events_repacking_helper

src/EventMessageEditor.cpp is compiled unchanged with g++ into a temporary directory outside the repository, against the
small stand-in headers below — the generator's own code: ros::Time (fromSec / toSec restated from recall of roscpp),
ros::init and ROS_INFO that do nothing, rosbag::Bag / View that read and write one flat binary file each, and the two
dvs_msgs types.  Nothing of the tool, source or compiled, is stored: the fixtures hold our input streams and the
messages it wrote.

What this pins is the tool's CONTROL FLOW: the first-event origin, the >= test, ONE advance per event (so that after a
gap its windows lag behind their header stamps), empty messages, the tail it never writes, 30 Hz.  It does NOT pin
roscpp's rounding in ros::Time(double): the stand-in restates it, exactly as tests/slice_ref.py does.

Inputs per file (topic 0 .. 3 of the tool's fixed list): short streams without window jumps — monotonic, equal stamps,
back-steps — and two with gaps.  Event i carries x = i & 0xffff, y = i >> 16, so a message's events identify themselves.
Every file stays far below the largest file already in tests/golden (712 434 bytes).
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BYTES = 712434
TOPICS_IN = ["/DAVIS346_left/events", "/DAVIS346_right/events", "/DVXplorer_left/events", "/DVXplorer_right/events"]
TOPICS_OUT = ["/DAVIS346_left/30HZ_events", "/DAVIS346_right/30HZ_events", "/DVXplorer_left/30HZ_events",
              "/DVXplorer_right/30HZ_events"]

# ---- the stand-in headers (the generator's own code).  Flat files, little-endian:
#   input : per message  u32 topic_len, topic bytes, u32 width, u32 height, u32 n, n x {u16 x, u16 y, u32 sec, u32 nsec, u8 p}
#   output: per message  u32 topic_len, topic bytes, u32 stamp.sec, u32 stamp.nsec (bag->write's time), u32 header.sec,
#           u32 header.nsec, u32 width, u32 height, u32 n, n x the same 13 bytes
HEADERS = {
    "ros/ros.h": r"""
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
namespace ros {
struct Time {
  uint32_t sec = 0, nsec = 0;
  Time() {}
  Time(uint32_t s, uint32_t n) : sec(s), nsec(n) {}
  explicit Time(double t) { fromSec(t); }
  Time& fromSec(double t) {  // roscpp's, restated from recall
    const double fl = std::floor(t);
    uint64_t s = (uint64_t)fl, n = (uint64_t)std::round((t - fl) * 1e9);
    s += n / 1000000000ull;
    n %= 1000000000ull;
    sec = (uint32_t)s, nsec = (uint32_t)n;
    return *this;
  }
  double toSec() const { return (double)sec + 1e-9 * (double)nsec; }
};
inline void init(int&, char**, const char*) {}
}  // namespace ros
#define ROS_INFO(...) ((void)0)
""",
    "std_msgs/Int32.h": "#pragma once\n",
    "dvs_msgs/Event.h": r"""
#pragma once
#include <ros/ros.h>
namespace dvs_msgs {
struct Event {
  uint16_t x = 0, y = 0;
  ros::Time ts;
  uint8_t polarity = 0;
};
}  // namespace dvs_msgs
""",
    "dvs_msgs/EventArray.h": r"""
#pragma once
#include <dvs_msgs/Event.h>
namespace dvs_msgs {
struct Header { ros::Time stamp; };
struct EventArray {
  typedef std::shared_ptr<const EventArray> ConstPtr;
  Header header;
  uint32_t height = 0, width = 0;
  std::vector<Event> events;
};
}  // namespace dvs_msgs
""",
    "rosbag/bag.h": r"""
#pragma once
#include <dvs_msgs/EventArray.h>
namespace rosbag {
namespace bagmode { enum BagMode { Write = 1, Read = 2 }; }
struct StoredMessage { std::string topic; std::shared_ptr<dvs_msgs::EventArray> msg; };
struct Bag {
  FILE* f = nullptr;
  std::vector<StoredMessage> stored;  // (Read: the whole file)
  static uint32_t u32(FILE* f, bool* ok) { uint32_t v = 0; *ok = fread(&v, 4, 1, f) == 1; return v; }
  void open(const char* path, int mode) {
    f = fopen(path, mode == bagmode::Read ? "rb" : "wb");
    if (!f || mode != bagmode::Read) return;
    for (;;) {
      bool ok;
      const uint32_t tl = u32(f, &ok);
      if (!ok) break;
      StoredMessage m;
      m.topic.resize(tl);
      if (tl && fread(&m.topic[0], 1, tl, f) != tl) abort();
      m.msg = std::make_shared<dvs_msgs::EventArray>();
      m.msg->width = u32(f, &ok), m.msg->height = u32(f, &ok);
      const uint32_t n = u32(f, &ok);
      m.msg->events.resize(n);
      for (uint32_t i = 0; i < n; i++) {
        dvs_msgs::Event& e = m.msg->events[i];
        if (fread(&e.x, 2, 1, f) != 1 || fread(&e.y, 2, 1, f) != 1 || fread(&e.ts.sec, 4, 1, f) != 1 ||
            fread(&e.ts.nsec, 4, 1, f) != 1 || fread(&e.polarity, 1, 1, f) != 1) abort();
      }
      stored.push_back(m);
    }
  }
  bool isOpen() const { return f != nullptr; }
  void write(const char* topic, const ros::Time& t, const dvs_msgs::EventArray& a) {
    const std::string tp(topic);
    const uint32_t head[7] = {(uint32_t)tp.size(), t.sec, t.nsec, a.header.stamp.sec, a.header.stamp.nsec, a.width, a.height};
    fwrite(&head[0], 4, 1, f);
    fwrite(tp.data(), 1, tp.size(), f);
    fwrite(&head[1], 4, 6, f);
    const uint32_t n = (uint32_t)a.events.size();
    fwrite(&n, 4, 1, f);
    for (const dvs_msgs::Event& e : a.events) {
      fwrite(&e.x, 2, 1, f), fwrite(&e.y, 2, 1, f), fwrite(&e.ts.sec, 4, 1, f), fwrite(&e.ts.nsec, 4, 1, f);
      fwrite(&e.polarity, 1, 1, f);
    }
  }
  void close() { if (f) fclose(f); f = nullptr; }
};
}  // namespace rosbag
""",
    "rosbag/view.h": r"""
#pragma once
#include <rosbag/bag.h>
namespace rosbag {
struct TopicQuery { std::string topic; explicit TopicQuery(const std::string& t) : topic(t) {} };
struct MessageInstance {
  std::shared_ptr<dvs_msgs::EventArray> msg;
  template <class T> std::shared_ptr<const T> instantiate() const { return msg; }
};
struct View {
  std::vector<MessageInstance> items;
  View(Bag& bag, const TopicQuery& q) {
    for (const StoredMessage& m : bag.stored)
      if (m.topic == q.topic) items.push_back(MessageInstance{m.msg});
  }
  std::vector<MessageInstance>::const_iterator begin() const { return items.begin(); }
  std::vector<MessageInstance>::const_iterator end() const { return items.end(); }
};
}  // namespace rosbag
""",
}


def build(helper_dir, work):
    for rel, text in HEADERS.items():
        path = os.path.join(work, "include", rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    exe = os.path.join(work, "event_message_editor")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++14", "-ffp-contract=off", "-I" + os.path.join(work, "include"),
                           os.path.join(helper_dir, "src", "EventMessageEditor.cpp"), "-o", exe])
    return exe


def write_input(path, topics, msg_events=7):
    """topics: per input topic (sec, nsec) arrays; cut into messages of msg_events events (the tool ignores the edges)"""
    with open(path, "wb") as f:
        for name, (sec, nsec) in zip(TOPICS_IN, topics):
            for a in range(0, len(sec), msg_events):
                b = min(a + msg_events, len(sec))
                f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<III", 346, 260, b - a))
                for i in range(a, b):
                    f.write(struct.pack("<HHIIB", i & 0xffff, i >> 16, int(sec[i]), int(nsec[i]), i & 1))


def read_output(path):
    """-> per output topic: (bag stamps [k, 2], header stamps [k, 2], counts [k], event ids [sum])"""
    out = {t: ([], [], [], []) for t in TOPICS_OUT}
    with open(path, "rb") as f:
        data = f.read()
    o = 0
    while o < len(data):
        (tl,) = struct.unpack_from("<I", data, o)
        topic = data[o + 4:o + 4 + tl].decode()
        o += 4 + tl
        bs, bn, hs, hn, w, h, n = struct.unpack_from("<7I", data, o)
        o += 28
        assert (w, h) == (346, 260)
        st = out[topic]
        st[0].append((bs, bn)), st[1].append((hs, hn)), st[2].append(n)
        for _ in range(n):
            x, y, _s, _n, _p = struct.unpack_from("<HHIIB", data, o)
            o += 13
            st[3].append(x | y << 16)
    return [out[t] for t in TOPICS_OUT]


def streams(rng, kind):
    """four topics' (sec, nsec) of one fixture"""
    period = 1e9 / 30
    topics = []
    for t in range(4):
        n = [240, 320, 180, 400][t]
        t0 = int(rng.integers(1, 2000)) * 1000000000 + int(rng.integers(0, 1000000000))
        if kind == "nojump":
            # steps below 0.9 periods (no event jumps a window), a quarter of them zero (equal stamps), and — topics 1 and
            # 3 — back-steps of up to 1.5 periods against the running maximum
            step = rng.integers(0, int(0.9 * period), n)
            step[rng.random(n) < 0.25] = 0
            back = (rng.random(n) < 0.2) & bool(t & 1)
            back[0] = False
            step[back] = 0  # (an event that steps back adds nothing to the running maximum the next one steps from)
            ns = t0 + np.cumsum(step)
            ns[back] -= rng.integers(0, int(1.5 * period), int(back.sum()))
        else:
            # gaps: most steps small, a few of 2 .. 6 periods (the tool's windows then lag behind their header stamps)
            step = rng.integers(0, int(0.4 * period), n)
            gap = rng.random(n) < 0.06
            step[gap] = rng.integers(int(2 * period), int(6 * period), int(gap.sum()))
            ns = t0 + np.cumsum(step)
        topics.append((ns // 1000000000, ns % 1000000000))
    return topics


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20261019)
    with tempfile.TemporaryDirectory() as work:
        exe = build(sys.argv[1], work)
        for name, kind in (("nojump_a", "nojump"), ("nojump_b", "nojump"), ("gaps_a", "gaps"), ("gaps_b", "gaps")):
            topics = streams(rng, kind)
            src, dst = os.path.join(work, name + ".in"), os.path.join(work, name + ".out")
            write_input(src, topics)
            subprocess.check_call([exe, src, dst])
            arrays = {"frequency": np.float64(30.0)}
            for t, ((sec, nsec), (bag, hdr, cnt, ids)) in enumerate(zip(topics, read_output(dst))):
                arrays["t%d_sec" % t], arrays["t%d_nsec" % t] = np.asarray(sec, np.uint32), np.asarray(nsec, np.uint32)
                arrays["t%d_bag_stamp" % t] = np.asarray(bag, np.uint32).reshape(-1, 2)
                arrays["t%d_header_stamp" % t] = np.asarray(hdr, np.uint32).reshape(-1, 2)
                arrays["t%d_count" % t] = np.asarray(cnt, np.uint32)
                arrays["t%d_events" % t] = np.asarray(ids, np.uint32)
            path = os.path.join(HERE, "repack_ref_%s.npz" % name)
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            assert size < MAX_BYTES, (path, size)
            print(path, size, "bytes;", [int(arrays["t%d_count" % t].size) for t in range(4)], "messages")


if __name__ == "__main__":
    main()
