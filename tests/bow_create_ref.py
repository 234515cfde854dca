"""Rule C of include/esvio_fe.h ("creating a vocabulary"): what DBoW2's TemplatedVocabulary::create does — HKmeansStep,
initiateClustersKMpp, FBrief::meanValue / distance, createWords, setNodeWeights — with the draws of C5 in place of rand().

create_loops() is the rule as plain sequential loops over Python ints in the reference's recursion order; create_numpy()
is the same rule with each node's inner loops as array operations, for inputs too large for the loops.  Both return
(file image, info dict); the image is format V (bow_ref.serialise), the info the counters of esvio_fe_bow_create_info.
Nothing here knows how the library lays the work out on the device.

A descriptor is bow_ref's 256-bit Python int (loops) or a row of eight uint32 (numpy)."""
import math

import numpy as np

from bow_ref import TF_IDF, TF, IDF, BINARY, desc_int, serialise  # noqa: F401

M64 = (1 << 64) - 1


# ---- C5: the draws --------------------------------------------------------------------------------------------------
def mix(z):
    """splitmix64's step on the state z: (z + gamma) finalised"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def root_key(seed):
    return mix(seed & M64)


def child_key(key, c):
    return mix(key ^ (c + 1))


def c5_draw(key, j, path=None):
    """draw j of the node with this key: 31 bits"""
    return mix(key ^ (((j + 1) << 32) & M64)) >> 33


def random_int(r, m):
    """RandomInt(0, m - 1) from the 31-bit r"""
    return int((float(r) / 2147483648.0) * float(m))


def random_value(r, s):
    """RandomValue<double>(0, s) from the 31-bit r"""
    return (float(r) / 2147483647.0) * float(s)


def popcount(x):
    return bin(x).count("1")


# ---- C2, C3 as loops ------------------------------------------------------------------------------------------------
def seed_centres(feats, k, draw):
    """C2: (centres, stopped short); draw(j) is the node's j-th draw"""
    m = len(feats)
    j = 0
    centres = [feats[random_int(draw(j), m)]]
    j += 1
    min_dist = [popcount(f ^ centres[0]) for f in feats]
    short = False
    while len(centres) < k:
        for i, f in enumerate(feats):
            if min_dist[i] > 0:
                d = popcount(f ^ centres[-1])
                if d < min_dist[i]:
                    min_dist[i] = d
        dist_sum = sum(min_dist)
        if dist_sum == 0:
            short = True
            break
        while True:
            cut_d = random_value(draw(j), dist_sum)
            j += 1
            if cut_d != 0.0:
                break
        pick, run = m - 1, 0
        for i, d in enumerate(min_dist):
            run += d
            if float(run) >= cut_d:
                pick = i
                break
        centres.append(feats[pick])
    return centres, short


def mean_value(group):
    """C3: bit i set iff more than floor(m / 2) of the group's features have it; the empty group gives 0"""
    if not group:
        return 0
    half = len(group) // 2
    out = 0
    for i in range(256):
        if sum((f >> i) & 1 for f in group) > half:
            out |= 1 << i
    return out


def kmeans_loops(feats, k, draw, max_passes):
    """C1 for m > k: (centres, assignment, passes, short seeding); passes is None where the guard stops the loop"""
    centres, short = seed_centres(feats, k, draw)
    last = None
    passes = 0
    while True:
        if passes == max_passes:
            return centres, last, None, short
        if last is not None:
            centres = [mean_value([f for f, a in zip(feats, last) if a == c]) for c in range(len(centres))]
        cur = []
        for f in feats:
            best, best_d = 0, popcount(f ^ centres[0])
            for c in range(1, len(centres)):
                d = popcount(f ^ centres[c])
                if d < best_d:
                    best, best_d = c, d
            cur.append(best)
        passes += 1
        if last is not None and cur == last:
            return centres, cur, passes, short
        last = cur


# ---- the same two as array operations -------------------------------------------------------------------------------
def _bits(desc):
    """[n][8] uint32 -> [n][256] float32 of 0 / 1, bit i of the descriptor in column i"""
    return np.unpackbits(np.ascontiguousarray(desc, "<u4").view(np.uint8).reshape(len(desc), 32), axis=1, bitorder="little").astype(np.float32)


def _dist(fb, cb):
    """Hamming distances [m][c] of bit rows (exact in float32: every value is at most 256)"""
    return (fb.sum(1)[:, None] + cb.sum(1)[None, :] - 2.0 * (fb @ cb.T)).astype(np.int64)


def kmeans_numpy(fb, k, draw, max_passes):
    m = len(fb)
    j = 0
    picks = [random_int(draw(j), m)]
    j += 1
    min_dist = _dist(fb, fb[picks[-1:]])[:, 0]
    short = False
    while len(picks) < k:
        d = _dist(fb, fb[picks[-1:]])[:, 0]
        min_dist = np.where(min_dist > 0, np.minimum(min_dist, d), min_dist)
        dist_sum = int(min_dist.sum())
        if dist_sum == 0:
            short = True
            break
        while True:
            cut_d = random_value(draw(j), dist_sum)
            j += 1
            if cut_d != 0.0:
                break
        hit = np.nonzero(np.cumsum(min_dist).astype(np.float64) >= cut_d)[0]
        picks.append(int(hit[0]) if len(hit) else m - 1)
    cb = fb[picks].copy()
    last = None
    passes = 0
    while True:
        if passes == max_passes:
            return cb, last, None, short
        if last is not None:
            onehot = np.zeros((len(cb), m), np.float32)
            onehot[last, np.arange(m)] = 1.0
            counts = (onehot @ fb).astype(np.int64)
            size = np.bincount(last, minlength=len(cb))
            cb = (counts > (size // 2)[:, None]).astype(np.float32)
        cur = np.argmin(_dist(fb, cb), axis=1)  # the first of equal distances
        passes += 1
        if last is not None and np.array_equal(cur, last):
            return cb, cur, passes, short
        last = cur


def _bits_int(row):
    return desc_int(np.packbits(row.astype(np.uint8), bitorder="little").view("<u4"))


# ---- C1, C4, C6 -----------------------------------------------------------------------------------------------------
class NotSettled(Exception):
    """the project's guard: .nodes k-means nodes had not settled after max_passes passes"""

    def __init__(self, nodes):
        Exception.__init__(self, "%d nodes not settled" % nodes)
        self.nodes = nodes


def _create(n, doc_offsets, k, L, weighting, scoring, seed, max_passes, draw, split, leaf_desc):
    """the recursion and everything behind it; split(idx list, draw_j) -> (centre ints, assignment, passes, short) is
    the k-means of one node, leaf_desc(i) feature i as an int"""
    doc_offsets = [int(o) for o in doc_offsets]
    assert doc_offsets[0] == 0 and doc_offsets[-1] == n and all(a <= b for a, b in zip(doc_offsets, doc_offsets[1:]))
    max_passes = max_passes or 100
    draw = draw or c5_draw
    nodes = [dict(parent=-1, desc=0, children=[], depth=0)]  # id = index, 0 the root
    info = dict(kmeans_nodes=0, passes=0, empty_clusters=0, short_seedings=0)
    unsettled = [0]

    def step(nid, idx, level, key, path):
        m = len(idx)
        if m <= k:
            centres, assign = [leaf_desc(i) for i in idx], list(range(m))
        else:
            info["kmeans_nodes"] += 1
            centres, assign, passes, short = split(idx, lambda j: draw(key, j, path))
            info["short_seedings"] += int(short)
            if passes is None:
                unsettled[0] += 1
                return
            info["passes"] = max(info["passes"], passes)
        groups = [[] for _ in centres]
        for i, a in zip(idx, assign):
            groups[int(a)].append(i)
        if m > k:
            info["empty_clusters"] += sum(1 for g in groups if not g)
        kids = []
        for d in centres:
            kids.append(len(nodes))
            nodes.append(dict(parent=nid, desc=d, children=[], depth=level))
            nodes[nid]["children"].append(kids[-1])
        if level < L:
            for c, g in enumerate(groups):
                if len(g) > 1:
                    step(kids[c], g, level + 1, child_key(key, c), path + (c,))

    step(0, list(range(n)), 1, root_key(seed), ())
    if unsettled[0]:
        raise NotSettled(unsettled[0])
    # C4
    leaves = [i for i in range(1, len(nodes)) if not nodes[i]["children"]]
    word_of = {nid: w for w, nid in enumerate(leaves)}
    weight = [0.0] * len(nodes)
    if weighting in (TF, BINARY):
        for nid in leaves:
            weight[nid] = 1.0
    else:
        ni = [0] * len(leaves)
        words = walk_all(nodes, n, leaf_desc, word_of)
        for d in range(len(doc_offsets) - 1):
            for w in set(words[doc_offsets[d]:doc_offsets[d + 1]]):
                ni[w] += 1
        n_docs = len(doc_offsets) - 1
        for w, nid in enumerate(leaves):
            weight[nid] = math.log(float(n_docs) / float(ni[w])) if ni[w] > 0 else 0.0
    data = serialise(k, L, scoring, weighting, [(i, nodes[i]["parent"], weight[i], nodes[i]["desc"]) for i in range(1, len(nodes))],
                     [(nid, w) for w, nid in enumerate(leaves)])
    info.update(nodes=len(nodes) - 1, words=len(leaves), depth=max(nodes[i]["depth"] for i in leaves),
                max_children=max(len(nd["children"]) for nd in nodes), bytes=len(data))
    return data, info


_walk_hook = [None]


def walk_all(nodes, n, leaf_desc, word_of):
    """W of every training feature on the finished tree: word ids in feature order"""
    if _walk_hook[0] is not None:
        return _walk_hook[0](nodes, n, word_of)
    out = []
    for i in range(n):
        f, node = leaf_desc(i), 0
        while nodes[node]["children"]:
            best, best_d = None, None
            for cid in nodes[node]["children"]:
                d = popcount(f ^ nodes[cid]["desc"])
                if best is None or d < best_d:
                    best, best_d = cid, d
            node = best
        out.append(word_of[node])
    return out


def _ints(desc):
    desc = np.asarray(desc, np.uint32).reshape(-1, 8)
    return [desc_int(r) for r in desc]


def create_loops(desc, doc_offsets, k, L, weighting=TF_IDF, scoring=0, seed=0, max_passes=0, draw=None):
    """desc: [n][8] uint32 or a list of 256-bit ints"""
    feats = list(desc) if len(desc) and isinstance(desc[0], int) else _ints(desc)
    limit = max_passes or 100

    def split(idx, draw_j):
        return kmeans_loops([feats[i] for i in idx], k, draw_j, limit)

    return _create(len(feats), doc_offsets, k, L, weighting, scoring, seed, max_passes, draw, split, lambda i: feats[i])


def create_numpy(desc, doc_offsets, k, L, weighting=TF_IDF, scoring=0, seed=0, max_passes=0, draw=None):
    desc = np.asarray(desc, np.uint32).reshape(-1, 8)
    bits = _bits(desc)
    feats = _ints(desc)
    limit = max_passes or 100

    def split(idx, draw_j):
        cb, assign, passes, short = kmeans_numpy(bits[np.asarray(idx)], k, draw_j, limit)
        return [_bits_int(r) for r in cb], assign, passes, short

    def walk(nodes, n, word_of):
        out = np.zeros(n, np.int64)

        def down(node, idx):
            kids = nodes[node]["children"]
            if not kids:
                out[idx] = word_of[node]
                return
            cb = _bits(np.array([[(nodes[c]["desc"] >> (32 * j)) & 0xffffffff for j in range(8)] for c in kids], np.uint32))
            best = np.argmin(_dist(bits[idx], cb), axis=1)
            for c, cid in enumerate(kids):
                sub = idx[best == c]
                if len(sub):
                    down(cid, sub)

        down(0, np.arange(n))
        return [int(w) for w in out]

    _walk_hook[0] = walk
    try:
        return _create(len(desc), doc_offsets, k, L, weighting, scoring, seed, max_passes, draw, split, lambda i: feats[i])
    finally:
        _walk_hook[0] = None


# ---- inputs the tests share -----------------------------------------------------------------------------------------
def low_entropy(n, seed):
    """descriptors whose first two bytes alone vary: duplicates, zero distances and ties in plenty"""
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 8), np.uint32)
    d[:, 0] = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    return d


def prototypes(n, n_proto, flip, seed):
    """n_proto random prototypes, each feature one of them with every bit flipped with probability `flip`"""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 2, (n_proto, 256), dtype=np.uint8)
    b = proto[rng.integers(0, n_proto, n)] ^ (rng.random((n, 256)) < flip).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(b, axis=1, bitorder="little")).view("<u4").astype(np.uint32).reshape(n, 8)


def uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)


def even_docs(n, n_docs):
    return [int(round(i * n / n_docs)) for i in range(n_docs + 1)]


def pick_ref(md, seg_off, cut_d):
    """C2's pick alone, as esvio_fe_bow_create_pick states it (include/esvio_fe_test.h): per segment the first rank whose
    running sum of md, as a double, is >= the segment's cut; the last rank if none; 0xffffffff for an empty segment or a
    cut that is not >= 0.  One value after the other."""
    out = []
    for s, cut in enumerate(cut_d):
        b, e = int(seg_off[s]), int(seg_off[s + 1])
        if e <= b or not cut >= 0.0:
            out.append(0xffffffff)
            continue
        run, pick = 0, e - b - 1
        for i in range(b, e):
            run += int(md[i])
            if float(run) >= cut:
                pick = i - b
                break
        out.append(pick)
    return np.array(out, np.uint32)
