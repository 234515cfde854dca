#!/usr/bin/env python3
"""A DBoW2 vocabulary file from a directory of per-keyframe descriptor arrays.

    tools/make_vocabulary.py DIR out.bin [--k 10] [--L 6] [--weighting 0] [--seed 1] [--max-passes 0]

DIR holds one .npy per keyframe (n_i x 8 uint32, as esvio_fe_kf_describe / FeatureTracker.keyframe_describe returns
kp_desc); the files are taken in sorted name order, one document each (an empty array is an empty document).  The tree is
trained on the device by esvio_fe_bow_create_vocabulary (include/esvio_fe.h "C, creating a vocabulary"); the file is what
the reference's loadBin and esvio_fe_bow_set_vocabulary read.  Prints the call's info as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esvio_amd import frontend as FE  # noqa: E402


def load_documents(folder):
    """-> (uint32 [n][8], int64 [n_docs + 1], file names)"""
    names = sorted(f for f in os.listdir(folder) if f.endswith(".npy"))
    if not names:
        raise SystemExit("no .npy files in %s" % folder)
    docs = []
    for f in names:
        a = np.load(os.path.join(folder, f))
        if a.size % 8:
            raise SystemExit("%s: %d values are no whole number of 8-word descriptors" % (f, a.size))
        docs.append(np.ascontiguousarray(a, np.uint32).reshape(-1, 8))
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return np.concatenate(docs), offsets, names


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("folder")
    ap.add_argument("out")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=6)
    ap.add_argument("--weighting", type=int, default=0, help="0 TF_IDF, 1 TF, 2 IDF, 3 BINARY")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-passes", type=int, default=0, help="0: 100")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    desc, offsets, names = load_documents(a.folder)
    t = FE.FeatureTracker(FE.make_config(64, 64, device=a.device, max_cnt=10, min_dist=5))
    try:
        rc, info = t.bow_create_vocabulary(desc, offsets, a.k, a.L, weighting=a.weighting, seed=a.seed, max_passes=a.max_passes, check=False)
        if rc:
            raise SystemExit("esvio_fe_bow_create_vocabulary: %d: %s" % (rc, info["message"]))
        data = t.bow_get_created(info["bytes"])
    finally:
        t.close()
    with open(a.out, "wb") as f:
        f.write(data)
    info.update(documents=len(names), descriptors=int(len(desc)), file=a.out)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.exit(main())
