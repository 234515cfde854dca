"""esvio_fe_bow_* micro-benchmark: loop detection on a SYNTHETIC vocabulary — a seeded random k = 10, L = 6 tree of the
shipped brief_k10L6.bin's size (1 111 110 nodes, 10^6 words; the shipped file itself is not at hand, so nothing here says
how its clusters behave) — with 215 and 3711 descriptors per keyframe (the keyframe micro-benchmark's corner counts) and
databases of 100 and 2000 entries.  A keyframe's descriptors are drawn from a pool of 50 000 random descriptors, so that
keyframes share words.  Per case: every kernel per launch from the LIBRARY'S OWN TIMERS (esvio_fe_bow_kernel_stats and
k_radix_pass of esvio_fe_get_kernel_stats: HIP events round the launch), the bytes the walk and the score kernel move,
the wall time of esvio_fe_bow_transform, _query and _detect_loop with the descriptors in device memory.  The norm chain
on its own: k_bow_vector on 3711 descriptors that fall into nearly as many words (3577 in the recorded run) against
3711 descriptors that fall into 37.
Beside them tools/bow_seq.cpp: the same rules as scalar loops on one core — this repository's own, NOT DBoW2's code,
which was not measured.  Per figure: the median of BLOCKS blocks of REPS after a warm-up block, and the blocks' min - max.
One process, one pass, no retries; run it under a time limit:

    g++ -O2 -std=c++17 tools/bow_seq.cpp -o tools/_bin/bow_seq
    timeout -k 10 900 python tools/bow_microbench.py > profiles/bow_microbench.txt
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402

BLOCKS, REPS = 5, 20
K, LEVELS = 10, 6
COUNTS, ENTRIES, POOL = (215, 3711), (100, 2000), 50000
SEQ = os.path.join(ROOT, "tools", "_bin", "bow_seq")
SEQ_ENTRIES = 100  # the one-core bridge builds its database itself: the small one only


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def vocabulary(seed):
    """the file image of a full K-ary tree of LEVELS levels in breadth-first ids: parent(i) = (i - 1) // K"""
    rng = np.random.default_rng(seed)
    n = sum(K ** l for l in range(1, LEVELS + 1))
    words = K ** LEVELS
    rec = np.zeros(n, np.dtype([("id", "<i4"), ("parent", "<i4"), ("w", "<f8"), ("d", "<u8", 4)]))
    rec["id"] = np.arange(1, n + 1)
    rec["parent"] = (rec["id"] - 1) // K
    rec["w"] = np.log(5000.0 / rng.integers(1, 4000, n))
    rec["d"] = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    wrec = np.zeros(words, np.dtype([("node", "<i4"), ("word", "<i4")]))
    wrec["node"] = np.arange(n - words + 1, n + 1)
    wrec["word"] = np.arange(words)
    return np.array([K, LEVELS, 0, 0, n, words], "<i4").tobytes() + rec.tobytes() + wrec.tobytes()


def timed(fn):
    out = []
    for _ in range(BLOCKS + 1):
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        out.append((time.perf_counter() - t0) / REPS * 1e6)
    return med(out[1:])


def alloc(L, data):
    p = C.c_void_p()
    assert L.esvio_fe_mem_alloc(FE.DEVICE, max(int(data.nbytes), 16), C.byref(p)) == 0
    assert L.esvio_fe_mem_upload(p, FE._p(data), data.nbytes) == 0
    return p


def kernels(ft, fn, names):
    """per launch, by the library's timers: {name: ((median, min, max) us, launches per call, bytes per launch)}"""
    per = {}
    for _ in range(BLOCKS + 1):
        ft.set_profiling(True)
        ft.reset_kernel_stats()
        for _ in range(REPS):
            fn()
        st = dict(ft.bow_kernel_stats(), k_radix_pass=ft.kernel_stats()["k_radix_pass"])
        ft.set_profiling(False)
        for k in names:
            v = st[k]
            if v["launches"]:
                per.setdefault(k, []).append((v["ms"] / v["launches"] * 1e3, v["launches"] // REPS, v["alg_bytes"] // v["launches"]))
    return {k: (med([p[0] for p in v[1:]]), v[0][1], v[0][2]) for k, v in per.items()}


def main():
    L = FE.load_library()
    t0 = time.perf_counter()
    voc = vocabulary(1)
    rc, info = FE.bow_vocabulary_header(voc)
    assert rc == 0, info
    print("loop detection on a SYNTHETIC vocabulary: seeded random k = %d, L = %d, %d nodes, %d words, %.1f MB file (built and checked in %.1f s);"
          % (K, LEVELS, info["nodes"], info["words"], len(voc) / 1e6, time.perf_counter() - t0))
    print("medians of %d blocks of %d (min - max); kernel times from the library's timers (HIP events round a launch)" % (BLOCKS, REPS))
    ft = FE.FeatureTracker(FE.make_config(346, 260, max_cnt=150, min_dist=10))
    h = ft._hd.h
    t0 = time.perf_counter()
    ft.bow_set_vocabulary(voc)
    print("esvio_fe_bow_set_vocabulary: %.2f s (check, layout, upload); device memory of the tree and tables: %.1f MB"
          % (time.perf_counter() - t0, ((info["nodes"] + 1) * (32 + 8 + 4 + 8) + info["words"] * 8) / 1e6))
    rng = np.random.default_rng(2)
    pool = rng.integers(0, 1 << 32, (POOL, 8), dtype=np.uint64).astype(np.uint32)
    res, nres, m = (FE.BowResult * 64)(), C.c_int32(0), C.c_int32(0)
    for n in COUNTS:
        frames = [pool[rng.integers(0, POOL, n)] for _ in range(max(ENTRIES))]
        query = np.ascontiguousarray(pool[rng.integers(0, POOL, n)])
        dq = alloc(L, query)
        first = ft.bow_transform(query)

        def transform():
            assert L.esvio_fe_bow_transform(h, dq, n, FE.DEVICE, None, None, None, None, 0, C.byref(nres)) == 0

        ks = kernels(ft, transform, ("k_bow_walk", "k_radix_pass", "k_bow_vector"))
        walk_bytes = n * (32 + 32 * K * LEVELS + 20)
        print("%d descriptors -> %d words:" % (n, first["n_bow"]))
        us = ks["k_bow_walk"][0]
        print("    k_bow_walk     %7.2f us per launch (%.2f - %.2f); %d child descriptors of 32 B per descriptor: %.2f MB = %.0f GB/s; %d dependent levels: bound by load latency, not bandwidth"
              % (us + (K * LEVELS, walk_bytes / 1e6, walk_bytes / us[0] / 1e3, LEVELS)))
        print("    k_radix_pass   %7.2f us per launch (%.2f - %.2f), %d per call" % (ks["k_radix_pass"][0] + (ks["k_radix_pass"][1],)))
        print("    k_bow_vector   %7.2f us per launch (%.2f - %.2f)" % ks["k_bow_vector"][0])
        print("    esvio_fe_bow_transform, descriptors in device memory, nothing copied back: %.1f us (%.1f - %.1f)" % timed(transform))
        if n == max(COUNTS):  # the norm chain on its own: the same count of descriptors in 1 % of the words
            few = np.ascontiguousarray(query[rng.integers(0, n // 100, n)])
            dfew = alloc(L, few)
            kf = kernels(ft, lambda: L.esvio_fe_bow_transform(h, dfew, n, FE.DEVICE, None, None, None, None, 0, C.byref(nres)), ("k_bow_vector",))
            a, b = ks["k_bow_vector"][0][0], kf["k_bow_vector"][0][0]
            print("    k_bow_vector on %d descriptors in %d words: %.2f us (%.2f - %.2f); the difference, %.2f us, is the sequential norm chain over %d words (and %d divisions)"
                  % ((n, ft.bow_transform(few)["n_bow"]) + kf["k_bow_vector"][0] + (a - b, first["n_bow"], first["n_bow"])))
            L.esvio_fe_mem_free(FE.DEVICE, dfew)
        done = 0
        for entries in ENTRIES:
            for fr in frames[done:entries]:
                ft.bow_add(np.ascontiguousarray(fr))
            done = entries
            assert ft.bow_entries() == entries

            def query_dev():
                assert L.esvio_fe_bow_query(h, dq, n, FE.DEVICE, 4, -1, res, C.byref(nres)) == 0

            query_dev()
            ids = [res[j].id for j in range(nres.value)]
            words = sum(len(np.unique(ft.bow_transform(np.ascontiguousarray(fr))["bow_word"])) for fr in frames[:3]) // 3
            ks = kernels(ft, query_dev, ("k_bow_score", "k_bow_select"))
            us, sb = ks["k_bow_score"][0], ks["k_bow_score"][2]
            print("  database of %d entries (~%d words each):" % (entries, words))
            print("    k_bow_score    %7.2f us per launch (%.2f - %.2f); %.2f MB of entries, query words and results = %.0f GB/s; one binary search per entry word, the adds in order: latency and issue, not bandwidth"
                  % (us + (sb / 1e6, sb / us[0] / 1e3)))
            print("    k_bow_select   %7.2f us per launch (%.2f - %.2f), 4 results" % ks["k_bow_select"][0])
            print("    esvio_fe_bow_query (max_results 4, max_id -1), descriptors in device memory: %.1f us (%.1f - %.1f)" % timed(query_dev))
            if entries == SEQ_ENTRIES:
                with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
                    f.write(np.array([len(voc), n, entries, 3], np.int32).tobytes() + voc)
                    f.write(np.concatenate(frames[:entries]).tobytes() + query.tobytes())
                try:
                    seq = subprocess.check_output([SEQ, f.name]).decode().split()
                finally:
                    os.unlink(f.name)
                at = seq.index("ids")
                vals = dict(zip(seq[:at:2], seq[1:at:2]))
                assert int(vals["words_xor"]) == int(np.bitwise_xor.reduce(first["bow_word"])) and [int(v) for v in seq[at + 1:]] == ids, (vals, ids)
                print("    one core (tools/bow_seq.cpp, scalar loops, NOT DBoW2's code): transform %.0f us, transform + query %.0f us" % (float(vals["transform_us"]), float(vals["query_us"])))
        # detect_loop adds an entry per call: the database grows from 2000 to 2120 entries while it is timed
        frame_index = [ft.bow_entries()]

        def detect():
            assert L.esvio_fe_bow_detect_loop(h, dq, n, FE.DEVICE, frame_index[0], C.byref(m), None, None) == 0
            frame_index[0] += 1

        print("    esvio_fe_bow_detect_loop (query of the entries below frame_index - 50, add), database growing from %d: %.1f us (%.1f - %.1f)" % ((frame_index[0],) + timed(detect)))
        ft.bow_clear()
        L.esvio_fe_mem_free(FE.DEVICE, dq)
    ft.close()


if __name__ == "__main__":
    main()
