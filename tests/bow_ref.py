"""The rules of include/esvio_fe.h "loop detection" (V, W, T, A, Q, L) read one step after another over dicts and lists:
what DBoW2's TemplatedVocabulary::transform, TemplatedDatabase::add / queryL1 and PoseGraph::detectLoop do, for the device
to be held to, value for value and bit for bit (a Python float is the IEEE double the rules are stated in).  Nothing here
knows the layout the library gives the tree on the device.  Also: a builder of synthetic vocabularies and the serialiser
of the binary file format — the shipped brief_k10L6.bin is not at hand, every vocabulary of the tests is made here.

A descriptor is a Python int of 256 bits: bit i of the descriptor is bit i of the int, so eight uint32 words w give
sum(w[j] << 32 j) and the file's four uint64 the same with 64."""
import math
import struct

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM = 0
LOOP_RESULTS, LOOP_GAP, LOOP_MIN_FIRST, LOOP_MIN_OTHER = 4, 50, 0.05, 0.015


def desc_int(words):
    """eight uint32 -> the 256-bit int"""
    return sum(int(w) << (32 * j) for j, w in enumerate(words))


def desc_words(d):
    """the 256-bit int -> eight uint32"""
    return np.array([(d >> (32 * j)) & 0xffffffff for j in range(8)], np.uint32)


def descs_array(ds):
    return np.array([desc_words(d) for d in ds], np.uint32).reshape(-1, 8)


# ---- V: the file ----------------------------------------------------------------------------------------------------
def serialise(k, L, scoring, weighting, nodes, words):
    """nodes: (node id, parent id, weight, descriptor int) in file order; words: (node id, word id) in file order"""
    out = [struct.pack("<6i", k, L, scoring, weighting, len(nodes), len(words))]
    for nid, pid, w, d in nodes:
        out.append(struct.pack("<iid4Q", nid, pid, w, *[(d >> (64 * j)) & 0xffffffffffffffff for j in range(4)]))
    for nid, wid in words:
        out.append(struct.pack("<ii", nid, wid))
    return b"".join(out)


def parse(data):
    """the file as loadBin reads it (trusting, like the reference): (header dict, nodes dict id -> dict(parent, weight,
    desc, children [in file order], word))"""
    k, L, scoring, weighting, n_nodes, n_words = struct.unpack_from("<6i", data, 0)
    nodes = {0: dict(parent=-1, weight=0.0, desc=0, children=[], word=-1)}
    recs = []
    for r in range(n_nodes):
        nid, pid, w, q0, q1, q2, q3 = struct.unpack_from("<iid4Q", data, 24 + 48 * r)
        recs.append((nid, pid))
        nodes[nid] = dict(parent=pid, weight=w, desc=q0 | q1 << 64 | q2 << 128 | q3 << 192, children=[], word=-1)
    for nid, pid in recs:
        nodes[pid]["children"].append(nid)
    for r in range(n_words):
        nid, wid = struct.unpack_from("<ii", data, 24 + 48 * n_nodes + 8 * r)
        nodes[nid]["word"] = wid
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, nodes=n_nodes, words=n_words), nodes


class TreeBuilder:
    """a tree node by node: add(parent) returns the new node's id (ids count up from 1); finish() numbers the leaves'
    words in id order and serialises, the node records shuffled if asked (child order is record order, so a shuffle
    changes it — parse() of the bytes is the truth the tests compare against)"""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.nodes = []  # [id, parent, weight, desc]

    def rand_desc(self):
        return desc_int(self.rng.integers(0, 1 << 32, 8, dtype=np.uint64))

    def add(self, parent, desc=None, weight=None):
        nid = len(self.nodes) + 1
        if weight is None:  # an idf: log(N / Ni)
            weight = math.log(5000.0 / float(self.rng.integers(1, 4000)))
        self.nodes.append([nid, parent, float(weight), self.rand_desc() if desc is None else desc])
        return nid

    def full(self, ks, parent=0):
        """a full tree below `parent`: ks[0] children, each with ks[1] children, ..."""
        if not ks:
            return
        for _ in range(ks[0]):
            self.full(ks[1:], self.add(parent))

    def finish(self, k=0, L=0, weighting=TF_IDF, scoring=L1_NORM, shuffle=False):
        parents = {n[1] for n in self.nodes}
        leaves = [n[0] for n in self.nodes if n[0] not in parents]
        recs = [tuple(n) for n in self.nodes]
        if shuffle:
            recs = [recs[j] for j in self.rng.permutation(len(recs))]
        return serialise(k, L, scoring, weighting, recs, [(nid, w) for w, nid in enumerate(leaves)])


def full_tree(ks, seed=0, weighting=TF_IDF, shuffle=False):
    b = TreeBuilder(seed)
    b.full(list(ks))
    return b.finish(k=max(ks), L=len(ks), weighting=weighting, shuffle=shuffle)


# ---- W, T -----------------------------------------------------------------------------------------------------------
class Vocabulary:
    def __init__(self, data):
        self.header, self.nodes = parse(data)
        self.weighting = self.header["weighting"]

    def word(self, d):
        """W: (word id, weight) of descriptor d"""
        node = self.nodes[0]
        while node["children"]:
            best, best_d = None, None
            for cid in node["children"]:
                dist = bin(d ^ self.nodes[cid]["desc"]).count("1")
                if best is None or dist < best_d:
                    best, best_d = cid, dist
            node = self.nodes[best]
        return node["word"], node["weight"]

    def vector(self, descs):
        """T: [(word, value)] in ascending word id"""
        pairs = [self.word(d) for d in descs]
        return bow_vector([(wid, w) for wid, w in pairs if w > 0], self.weighting in (TF_IDF, TF))


def bow_vector(pairs, repeat):
    """BowVector::addWeight (repeat) or addIfNotExist for every (word, value) pair in turn, then normalize(L1):
    [(word, value)] in ascending word id"""
    v = {}
    for wid, w in pairs:
        if repeat:
            v[wid] = v[wid] + w if wid in v else w
        elif wid not in v:
            v[wid] = w
    order = sorted(v)
    norm = 0.0
    for wid in order:
        norm += abs(v[wid])
    if norm > 0.0:
        for wid in order:
            v[wid] = v[wid] / norm
    return [(wid, v[wid]) for wid in order]


# ---- A, Q, L ---------------------------------------------------------------------------------------------------------
def raw_scores(q, entries, max_id):
    """Q's sums: {entry id: s_e} of the entries that take part and share a word with the vector q"""
    N = len(entries)
    out = {}
    for e, vec in enumerate(entries):
        if not (e < max_id or max_id == -1 or e == N - 1):
            continue
        dv_of = dict(vec)
        for wid, qv in q:  # ascending word id
            if wid in dv_of:
                dv = dv_of[wid]
                value = abs(qv - dv) - abs(qv) - abs(dv)
                out[e] = out[e] + value if e in out else value
    return out


def ranked(scores, max_results):
    """ascending s_e, equal sums by ascending entry id, cut, Score = -s_e / 2.0"""
    order = sorted(scores, key=lambda e: (scores[e], e))[:max_results]
    return [(e, -scores[e] / 2.0) for e in order]


def loop_decision(R, frame_index):
    """L on the query's results R = [(id, score)]"""
    find = len(R) >= 1 and R[0][1] > LOOP_MIN_FIRST and any(R[i][1] > LOOP_MIN_OTHER for i in range(1, len(R)))
    if not (find and frame_index > LOOP_GAP):
        return -1
    m = -1
    for rid, score in R:
        if m == -1 or (rid < m and score > LOOP_MIN_OTHER):
            m = rid
    return m


class Database:
    def __init__(self, voc):
        self.voc, self.entries = voc, []

    def add(self, descs):
        self.entries.append(self.voc.vector(descs))
        return len(self.entries) - 1

    def scores(self, descs, max_id):
        return raw_scores(self.voc.vector(descs), self.entries, max_id)

    def query(self, descs, max_results, max_id):
        return ranked(self.scores(descs, max_id), max_results)

    def detect_loop(self, descs, frame_index):
        R = self.query(descs, LOOP_RESULTS, frame_index - LOOP_GAP)
        self.add(descs)
        return loop_decision(R, frame_index), R


# ---- inputs the device tests share ----------------------------------------------------------------------------------
def sum_desc(vals):
    s = 0.0
    for v in reversed(vals):
        s += v
    return s


def sum_pairwise(vals):
    vals = list(vals)
    while len(vals) > 1:
        vals = [vals[j] + vals[j + 1] if j + 1 < len(vals) else vals[j] for j in range(0, len(vals), 2)]
    return vals[0] if vals else 0.0


def sum_asc(vals):
    s = 0.0
    for v in vals:
        s += v
    return s


def node_descs(voc):
    """descriptor of every leaf, by word id"""
    by_word = {}
    for n in voc.nodes.values():
        if not n["children"] and n["word"] >= 0:
            by_word[n["word"]] = n["desc"]
    return by_word


def discriminating_norm_case(ks=(10, 10), n=40, first_seed=0):
    """(file bytes, descriptors, seed): a TF_IDF case whose norm — the ascending sum of the un-normalised values —
    differs in at least one bit from the same values summed in descending order AND from their pairwise sum; seeds are
    searched until it does.  The descriptors are leaves' own descriptors, some repeated."""
    for seed in range(first_seed, first_seed + 200):
        data = full_tree(ks, seed=seed)
        voc = Vocabulary(data)
        rng = np.random.default_rng(seed + 1000)
        leaves = node_descs(voc)
        picks = [leaves[int(w)] for w in rng.integers(0, len(leaves), n)]
        vals = {}
        for d in picks:
            wid, w = voc.word(d)
            vals[wid] = vals[wid] + w if wid in vals else w
        ordered = [vals[w] for w in sorted(vals)]
        a = sum_asc(ordered)
        if a != sum_desc(ordered) and a != sum_pairwise(ordered):
            return data, picks, seed
    raise AssertionError("no discriminating seed found")


def discriminating_weight(times, seed=0):
    """an idf-like weight w for which w added `times` times, one after another, is not times * w"""
    rng = np.random.default_rng(seed)
    while True:
        w = math.log(5000.0 / float(rng.integers(1, 4000)))
        if sum_asc([w] * times) != times * w:
            return w


def discriminating_score_case(ks=(10, 10), n=30, first_seed=0):
    """(file bytes, entry descriptors, query descriptors, seed): the query shares several words with the entry and the
    sum of the shared words' terms differs in at least one bit when the words are taken in descending order"""
    for seed in range(first_seed, first_seed + 200):
        data = full_tree(ks, seed=seed)
        voc = Vocabulary(data)
        rng = np.random.default_rng(seed + 2000)
        leaves = node_descs(voc)
        entry = [leaves[int(w)] for w in rng.integers(0, len(leaves), n)]
        query = entry[: n // 2] + [leaves[int(w)] for w in rng.integers(0, len(leaves), n)]
        q, e = voc.vector(query), dict(voc.vector(entry))
        terms = [abs(qv - e[w]) - abs(qv) - abs(e[w]) for w, qv in q if w in e]
        if len(terms) >= 5:
            fwd = terms[0]
            for t in terms[1:]:
                fwd += t
            rev = terms[-1]
            for t in reversed(terms[:-1]):
                rev += t
            if fwd != rev:
                return data, entry, query, seed
    raise AssertionError("no discriminating seed found")
