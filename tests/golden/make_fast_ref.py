#!/usr/bin/env python3
"""Regenerates tests/golden/fast_ref_*.npz: FAST-9/10 corners, FAST-10 scores and 3x3 non-max survivors
as the REFERENCE'S OWN compiled code gives them.

Run by hand on a machine that has the reference tree, never by a test:

    python tests/golden/make_fast_ref.py <reference>/dependences/fast_neon-master

The library's plain C++ sources (src/fast_9.cpp, fast_10.cpp, fast_10_score.cpp, nonmax_3x3.cpp: no
dependency at all) are compiled unchanged with g++ into a temporary directory outside the repository and
linked with the small driver below, which only reads an image, calls fast::fast_corner_detect_9 / _10,
fast::fast_corner_score_10 and fast::fast_nonmax_3x3 (include/fast/fast.h:22-47) and writes what they
return.  Nothing of the library, source or compiled, is stored: the fixtures hold our input images and
its recorded outputs.

Inputs: time surfaces rendered by the CPU oracle from esvio_amd.synth.SceneStream at the sensor sizes
of configs C1 / C3 / C5, one of them after equalize (CLAHE + normalize), a uniform-noise image, and
small hand-made images at the edges of the definition.  Per image and barrier: detect_9 xy, detect_10
xy, score_10, nonmax indices; per image the library's one-core CPU time per call at barrier 20
(context for the GPU figures in KERNELS.md, not a test).

Every file stays below the largest file already in tests/golden (712 434 bytes): the low barriers are
stored for the small sizes only.
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from esvio_amd.events import event_times  # noqa: E402
from esvio_amd.synth import SceneStream  # noqa: E402
from oracle import oracle as O  # noqa: E402

MAX_BYTES = 712434
TIME_BARRIER = 20

DRIVER = r"""
// driver of tests/golden/make_fast_ref.py (the repository's own code)
#include <fast/fast.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace fast;
static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
template <class T> static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  int32_t hdr[4];
  if (fread(hdr, 4, 4, fi) != 4) return 4;
  const int W = hdr[0], H = hdr[1], nb = hdr[2], tb = hdr[3];
  std::vector<int32_t> barriers(nb);
  if ((int)fread(barriers.data(), 4, nb, fi) != nb) return 4;
  std::vector<fast_byte> img((size_t)W * H);
  if (fread(img.data(), 1, img.size(), fi) != img.size()) return 4;
  fclose(fi);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 5;
  for (int b = 0; b < nb; b++) {
    std::vector<fast_xy> c9, c10;
    std::vector<int> sc, nm;
    fast_corner_detect_9(img.data(), W, H, W, (short)barriers[b], c9);
    fast_corner_detect_10(img.data(), W, H, W, (short)barriers[b], c10);
    fast_corner_score_10(img.data(), W, c10, barriers[b], sc);
    fast_nonmax_3x3(c10, sc, nm);
    int32_t n;
    n = (int32_t)c9.size();  put(fo, &n, 1); put(fo, (const int16_t*)c9.data(), 2 * c9.size());
    n = (int32_t)c10.size(); put(fo, &n, 1); put(fo, (const int16_t*)c10.data(), 2 * c10.size());
    put(fo, sc.data(), sc.size());
    n = (int32_t)nm.size();  put(fo, &n, 1); put(fo, nm.data(), nm.size());
  }
  double best[4] = {1e30, 1e30, 1e30, 1e30};
  for (int rep = 0; rep < 7; rep++) {
    std::vector<fast_xy> c9, c10;
    std::vector<int> sc, nm;
    double t0 = now_ms();
    fast_corner_detect_9(img.data(), W, H, W, (short)tb, c9);
    double t1 = now_ms();
    fast_corner_detect_10(img.data(), W, H, W, (short)tb, c10);
    double t2 = now_ms();
    fast_corner_score_10(img.data(), W, c10, tb, sc);
    double t3 = now_ms();
    fast_nonmax_3x3(c10, sc, nm);
    double t4 = now_ms();
    const double d[4] = {t1 - t0, t2 - t1, t3 - t2, t4 - t3};
    for (int k = 0; k < 4; k++) if (d[k] < best[k]) best[k] = d[k];
  }
  put(fo, best, 4);
  fclose(fo);
  return 0;
}
"""
# (fast::fast_xy is two shorts, fast.h:11-15: the driver writes the vectors' storage as int16 pairs)


def build_driver(fast_dir, tmp):
    srcs = [os.path.join(fast_dir, "src", f) for f in ("fast_9.cpp", "fast_10.cpp", "fast_10_score.cpp", "nonmax_3x3.cpp")]
    drv = os.path.join(tmp, "driver.cpp")
    with open(drv, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "fast_ref_driver")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-O2", "-std=c++14", "-I" + os.path.join(fast_dir, "include"), drv] + srcs + ["-o", exe])
    ver = subprocess.check_output([cxx, "--version"]).decode().splitlines()[0]
    return exe, ver + " -O2"


def run_ref(exe, tmp, img, barriers):
    H, W = img.shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i", W, H, len(barriers), TIME_BARRIER))
        f.write(struct.pack("<%di" % len(barriers), *barriers))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype, n, pos).copy()
        pos += a.nbytes
        return a

    res = {}
    for b in barriers:
        n9 = int(take(np.int32, 1)[0])
        d9 = take(np.int16, 2 * n9).reshape(-1, 2)
        n10 = int(take(np.int32, 1)[0])
        d10 = take(np.int16, 2 * n10).reshape(-1, 2)
        s10 = take(np.int32, n10)
        nnm = int(take(np.int32, 1)[0])
        nm = take(np.int32, nnm)
        res[b] = (d9, d10, s10, nm)
    cpu_ms = take(np.float64, 4)
    assert pos == len(buf)
    return res, cpu_ms


def time_surfaces(W, H, batches, rate, equalize=False, seed=7):
    """left time surface of the oracle's tracker after `batches` scene-stream batches"""
    s = SceneStream(W, H, rate=rate, seed=seed)
    tr = O.Tracker(O.make_config(W, H, max_cnt=150, min_dist=10, f_ransac=1))
    for _ in range(batches):
        L, R, _ = s.next_batch()
        tr.track_event(event_times(L)[-1], L, R, True)
    ts = tr.time_surface(0).copy()
    if equalize:
        ts = O.normalize_minmax(O.clahe(ts))
    return np.ascontiguousarray(ts, np.uint8)


def small_images():
    out = {}
    W, H = 48, 44
    a = np.zeros((H, W), np.uint8)
    a[3, 3] = 200          # a corner on the first pixel the detector visits ...
    a[H - 4, W - 4] = 90   # ... and on the last
    out["edges"] = a
    a = np.full((H, W), 30, np.uint8)
    a[10, 10:13] = 200     # three equal scores in a row: each suppresses its neighbour
    a[10, 20:24] = 200     # four (the ends see each other on their rings)
    a[20:23, 10] = 180     # a column
    a[20:24, 20] = 180
    for k in range(3):     # a diagonal
        a[30 + k, 30 + k] = 220
    a[34, 8:10] = 5        # dark ones, two in a row
    a[36, 40] = 250        # unequal neighbours: the larger survives
    a[36, 41] = 251
    out["plateaus"] = a
    out["constant"] = np.full((H, W), 77, np.uint8)
    rng = np.random.default_rng(5)
    a = np.kron(rng.integers(0, 256, (H // 4, W // 4)), np.ones((4, 4))).astype(np.int64)
    a = np.clip(a + rng.integers(-6, 7, (H, W)), 0, 255).astype(np.uint8)
    out["blocks"] = a      # 4x4 blocks + small noise: many real corners with close scores
    out["tiny7x7"] = rng.integers(0, 256, (7, 7)).astype(np.uint8)   # CPU restatement only
    c = np.full((7, 7), 10, np.uint8)
    c[3, 3] = 120
    out["tiny7x7c"] = c
    out["tiny6x9"] = rng.integers(0, 256, (9, 6)).astype(np.uint8)
    return out


def save(path, images, results, compiler):
    d = {"names": np.array(list(images)), "compiler": np.array(compiler)}
    for name, img in images.items():
        res, cpu_ms = results[name]
        d[name + "_img"] = img
        d[name + "_barriers"] = np.array(list(res), np.int32)
        d[name + "_cpu_ms"] = cpu_ms   # detect_9, detect_10, score_10, nonmax_3x3 at barrier 20: min of 7
        for b, (d9, d10, s10, nm) in res.items():
            d["%s_b%d_d9" % (name, b)] = d9
            d["%s_b%d_d10" % (name, b)] = d10
            d["%s_b%d_s10" % (name, b)] = s10
            d["%s_b%d_nm" % (name, b)] = nm
    np.savez_compressed(path, **d)
    sz = os.path.getsize(path)
    print("%-32s %7d bytes  %s" % (os.path.basename(path), sz,
                                   "  ".join("%s:%s" % (n, {b: len(r[1]) for b, r in results[n][0].items()}) for n in images)))
    assert sz < MAX_BYTES, "%s: %d bytes, limit %d" % (path, sz, MAX_BYTES)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    fast_dir = os.path.abspath(sys.argv[1])
    O.build()
    with tempfile.TemporaryDirectory(prefix="fast_ref_") as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        exe, compiler = build_driver(fast_dir, tmp)
        rng = np.random.default_rng(11)
        files = {
            "fast_ref_ts_346x260.npz": ({"ts346": time_surfaces(346, 260, 4, 1e6)}, {"ts346": [0, 7, 20, 40]}),
            "fast_ref_noise_346x260.npz": ({"noise346": rng.integers(0, 256, (260, 346)).astype(np.uint8)},
                                           {"noise346": [0, 7, 20, 40]}),
            "fast_ref_ts_640x480.npz": ({"ts640": time_surfaces(640, 480, 4, 3e6)}, {"ts640": [0, 7, 20, 40]}),
            "fast_ref_eq_640x480.npz": ({"eq640": time_surfaces(640, 480, 3, 3e6, equalize=True, seed=9)},
                                        {"eq640": [7, 20, 40]}),
            "fast_ref_ts_1280x720.npz": ({"ts1280": time_surfaces(1280, 720, 3, 6e6)}, {"ts1280": [20, 40]}),
        }
        sm = small_images()
        files["fast_ref_small.npz"] = (sm, {n: [0, 1, 7, 20, 40, 100, 255] for n in sm})
        for fname, (images, barriers) in files.items():
            results = {n: run_ref(exe, tmp, img, barriers[n]) for n, img in images.items()}
            save(os.path.join(HERE, fname), images, results, compiler)


if __name__ == "__main__":
    main()
