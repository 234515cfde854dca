#!/usr/bin/env python3
"""Regenerates tests/golden/bow_vector_ref.npz: what DBoW2's BowVector::addWeight, addIfNotExist and normalize(L1) leave
for seeded inputs, as the REFERENCE'S OWN compiled code gives it.

Run by hand on a machine that has the reference tree, never by a test:

    python tests/golden/make_bow_ref.py <reference>/pose_graph/src/ThirdParty/DBoW

BowVector.cpp needs nothing but a C++ compiler.  It is compiled unchanged with g++ into a temporary directory outside the
repository and linked with the small driver below, which only reads (word id, value) pairs, calls addWeight or
addIfNotExist for each in turn, then normalize(DBoW2::L1), and writes the map.  Nothing of the library, source or
compiled, is stored: the fixture holds our inputs and its recorded outputs.  The rest of DBoW2 (the vocabulary, the
database) includes OpenCV and boost and is not compiled here: its rules are cited by line in include/esvio_fe.h.

Cases (mode 0: addWeight, 1: addIfNotExist), values w = log(5000 / Ni) like an idf: one pair; one word hit 7 and 300
times; 40, 300 and 3711 pairs over few and over many words; all values 0.0 (no division)."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = r"""
// driver of tests/golden/make_bow_ref.py (the repository's own code)
#include "BowVector.h"
#include <cstdint>
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 3;
  int32_t cases;
  if (fread(&cases, 4, 1, fi) != 1) return 4;
  for (int c = 0; c < cases; c++) {
    int32_t hdr[2];
    if (fread(hdr, 4, 2, fi) != 2) return 4;
    std::vector<uint32_t> ids(hdr[1]);
    std::vector<double> vals(hdr[1]);
    if ((int)fread(ids.data(), 4, hdr[1], fi) != hdr[1] || (int)fread(vals.data(), 8, hdr[1], fi) != hdr[1]) return 4;
    DBoW2::BowVector v;
    for (int i = 0; i < hdr[1]; i++) {
      if (hdr[0] == 0) v.addWeight(ids[i], vals[i]);
      else v.addIfNotExist(ids[i], vals[i]);
    }
    v.normalize(DBoW2::L1);
    int32_t n = (int32_t)v.size();
    fwrite(&n, 4, 1, fo);
    for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
      uint32_t id = it->first;
      double val = it->second;
      fwrite(&id, 4, 1, fo);
      fwrite(&val, 8, 1, fo);
    }
  }
  fclose(fo);
  return 0;
}
"""


def cases():
    rng = np.random.default_rng(20261020)

    def idf(n):
        return np.log(5000.0 / rng.integers(1, 4000, n).astype(np.float64))
    out = []
    for mode in (0, 1):
        out.append((mode, np.array([5], np.uint32), idf(1)))
        for reps in (7, 300):
            out.append((mode, np.full(reps, 11, np.uint32), np.full(reps, idf(1)[0])))
        for n, words in ((40, 12), (300, 1000), (3711, 600), (3711, 1000000)):
            table = idf(min(words, 5000))  # a word's value is a function of the word
            ids = rng.integers(0, words, n).astype(np.uint32)
            out.append((mode, ids, table[ids % len(table)]))
        out.append((mode, np.arange(9, dtype=np.uint32)[::-1].copy(), np.zeros(9)))
    return out


def main(dbow_dir):
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe, fin, fout = (os.path.join(tmp, n) for n in ("driver.cpp", "driver", "in.bin", "out.bin"))
        open(drv, "w").write(DRIVER)
        subprocess.check_call(["g++", "-O3", "-std=c++11", "-I" + dbow_dir, os.path.join(dbow_dir, "BowVector.cpp"), drv, "-o", exe])
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", len(cs)))
            for mode, ids, vals in cs:
                f.write(struct.pack("<ii", mode, len(ids)) + ids.tobytes() + vals.astype("<f8").tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    arrays, pos = {"cases": np.int32(len(cs))}, 0
    for c, (mode, ids, vals) in enumerate(cs):
        n = struct.unpack_from("<i", raw, pos)[0]
        rec = np.frombuffer(raw, np.dtype([("id", "<u4"), ("val", "<f8")]), n, pos + 4)
        pos += 4 + 12 * n
        arrays.update({"mode_%d" % c: np.int32(mode), "in_ids_%d" % c: ids, "in_vals_%d" % c: vals,
                       "out_ids_%d" % c: rec["id"].copy(), "out_vals_%d" % c: rec["val"].copy()})
    assert pos == len(raw)
    path = os.path.join(HERE, "bow_vector_ref.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(cs), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
