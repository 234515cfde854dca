#!/usr/bin/env python3
"""esvio_fe_bow_create_vocabulary beside the same rule on one core.

    tools/voc_create_microbench.py [--sizes 65536,1048576] [--levels 3,6] [--k 10] [--seq-max 1048576] [--out FILE]

Per (n, L): prototype-plus-flips descriptors (n / 64 prototypes, 8 % of the bits flipped), n / 200 documents, TF_IDF.
Reports the call's wall time (the second of two calls: the first allocates), the library's own per-kernel timers for that
call (esvio_fe_bow_create_kernel_stats; the stable sorts are k_radix_pass of the track table, the document counts' walk
k_bow_walk of loop detection's), and the wall time of tools/_bin/voc_create_seq on one core of the same host in the same
run, whose file image must equal the library's byte for byte.  Sizes above --seq-max skip the one-core run and say so."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from esvio_amd import build as B  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402


def prototypes(n, seed):
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 2, (max(n // 64, 4), 256), dtype=np.uint8)
    out = np.empty((n, 8), np.uint32)
    for a in range(0, n, 1 << 16):  # in slabs: the bit matrix of 2^20 descriptors would take 256 MiB
        m = min(1 << 16, n - a)
        b = proto[rng.integers(0, len(proto), m)] ^ (rng.random((m, 256)) < 0.08).astype(np.uint8)
        out[a:a + m] = np.packbits(b, axis=1, bitorder="little").view("<u4")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--levels", default="3,6")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seq-max", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    seq = B.build_voc_seq()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    t = FE.FeatureTracker(FE.make_config(64, 64, device=0, max_cnt=10, min_dist=5))
    try:
        for n in [int(x) for x in a.sizes.split(",")]:
            desc = prototypes(n, 1)
            docs = np.linspace(0, n, max(n // 200, 1) + 1).astype(np.int64)
            for L in [int(x) for x in a.levels.split(",")]:
                t.bow_create_vocabulary(desc, docs, a.k, L, seed=1)
                t.set_profiling(True)
                t.reset_kernel_stats()
                before = (t.bow_create_kernel_stats(), t.kernel_stats(), t.bow_kernel_stats())
                t0 = time.perf_counter()
                rc, info = t.bow_create_vocabulary(desc, docs, a.k, L, seed=1)
                wall = (time.perf_counter() - t0) * 1e3
                after = (t.bow_create_kernel_stats(), t.kernel_stats(), t.bow_kernel_stats())
                t.set_profiling(False)
                image = t.bow_get_created(info["bytes"])
                say("n %d  k %d  L %d: call %.2f ms (timers on)  nodes %d  words %d  k-means nodes %d  passes %d  empty clusters %d"
                    % (n, a.k, L, wall, info["nodes"], info["words"], info["kmeans_nodes"], info["passes"], info["empty_clusters"]))
                t0 = time.perf_counter()
                t.bow_create_vocabulary(desc, docs, a.k, L, seed=1)
                say("    call, timers off: %.2f ms" % ((time.perf_counter() - t0) * 1e3))
                total = 0.0
                for tab_b, tab_a, pick in zip(before, after, (None, ("k_radix_pass",), ("k_bow_walk",))):
                    for name in tab_a:
                        if pick is not None and name not in pick:
                            continue
                        ms, k = tab_a[name]["ms"] - tab_b[name]["ms"], tab_a[name]["launches"] - tab_b[name]["launches"]
                        gb = (tab_a[name]["alg_bytes"] - tab_b[name]["alg_bytes"]) / 1e9
                        total += ms
                        say("    %-20s %9.3f ms  %6d launches  %8.3f GB algorithmic%s" % (name, ms, k, gb, "  %7.1f GB/s" % (gb / ms * 1e3) if ms > 0 else ""))
                say("    kernels in all       %9.3f ms" % total)
                if n > a.seq_max:
                    say("    one core: not run (n above --seq-max)")
                    continue
                with tempfile.TemporaryDirectory() as tmp:
                    fd, fo, fv = (os.path.join(tmp, x) for x in ("desc.u32", "docs.i64", "voc.bin"))
                    desc.astype("<u4").tofile(fd)
                    docs.astype("<i8").tofile(fo)
                    out = subprocess.check_output([seq, fd, str(n), fo, str(len(docs) - 1), str(a.k), str(L), "0", "1", fv]).decode().split()
                    same = open(fv, "rb").read() == image
                say("    one core (voc_create_seq): %.1f ms, image %s the library's" % (float(out[0]), "equals" if same else "DIFFERS FROM"))
                if not same:
                    return 1
    finally:
        t.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
