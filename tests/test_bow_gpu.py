"""GPU: loop detection (esvio_fe_bow_*) against tests/bow_ref.py, the sequential reading of the rules in
include/esvio_fe.h "loop detection" — word for word, index for index, doubles bit for bit; nothing here has a tolerance:
every operation is an integer one or an IEEE double addition, subtraction or division in a stated order.  Every vocabulary
is synthetic (tests/bow_ref.py builds and serialises it).  The sizes are the smallest that reach each edge: the lanes of
a walk group, a wave, the query words the score kernel keeps in LDS (all read from esvio_fe_bow_limits), the pools'
first capacity."""
import ctypes as C
import os

import numpy as np
import pytest

import bow_ref as B
import kf_ref as K
from esvio_amd import frontend as FE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIM = FE.bow_limits()
G = LIM["group_lanes"]
ALL = (1 << 256) - 1


class Dev:
    """device memory of the library's runtime: upload, download"""

    def __init__(self, nbytes, data=None):
        self.L, self.hip, self.p, self.n = FE.load_library(), C.CDLL("libamdhip64.so"), C.c_void_p(), int(nbytes)
        assert self.L.esvio_fe_mem_alloc(FE.DEVICE, max(self.n, 16), C.byref(self.p)) == 0
        if data is not None:
            a = np.ascontiguousarray(data)
            assert a.nbytes == self.n and (self.n == 0 or self.L.esvio_fe_mem_upload(self.p, FE._p(a), a.nbytes) == 0)

    @property
    def ptr(self):
        return self.p.value

    def free(self):
        self.L.esvio_fe_mem_free(FE.DEVICE, self.p)


@pytest.fixture(scope="module")
def ft():
    t = FE.FeatureTracker(FE.make_config(67, 45, device=0, max_cnt=40, min_dist=5))
    yield t
    t.close()


def use(ft, data):
    """the vocabulary `data` on an empty database; -> its sequential reading"""
    if ft.bow_entries():
        ft.bow_clear()
    ft.bow_set_vocabulary(data)
    return B.Vocabulary(data)


def bits(vals):
    return np.array(vals, np.float64).tobytes()


def block_tree(ks, weighting=B.TF_IDF, seed=0, weights=None):
    """a full tree whose leaves' own descriptors walk to themselves: the child j of a node at level l has its parent's
    bits and block (l, j) of 240 / (levels * k) bits more, so the right child is two blocks nearer than any other.
    weights: {word id: weight} in place of the random idf.  -> (file bytes, the leaves' descriptors by word id)"""
    levels, k = len(ks), max(ks)
    width = 240 // (levels * k)
    t = B.TreeBuilder(seed)
    leaves = []

    def grow(parent, desc, level):
        for j in range(ks[level]):
            d = desc | (((1 << width) - 1) << (width * (level * k + j)))
            last = level + 1 == levels
            nid = t.add(parent, d, (weights or {}).get(len(leaves)) if last else None)
            if level + 1 < levels:
                grow(nid, d, level + 1)
            else:
                leaves.append(d)
    grow(0, 0, 0)
    return t.finish(k=k, L=levels, weighting=weighting), leaves


# ---- walk ------------------------------------------------------------------------------------------------------------
def walk_trees():
    out = {"k 3, L 2": B.full_tree((3, 3), seed=1), "k 10, L 3": B.full_tree((10, 10, 10), seed=2),
           "one child more than a group's lanes": B.full_tree((G + 1, 2), seed=3),
           "two rounds and one child more": B.full_tree((2 * G + 1,), seed=4),
           "records shuffled": B.full_tree((5, 4, 3), seed=5, shuffle=True)}
    t = B.TreeBuilder(6)  # a node with one child; leaves at depths 1 and 3
    a, b, c = t.add(0), t.add(0), t.add(0)
    t.add(a), t.add(a)
    d = t.add(c)
    t.add(d), t.add(d), t.add(d)
    out["one child, leaves at depths 1 and 3"] = t.finish(k=3, L=3, shuffle=True)
    t = B.TreeBuilder(7)  # duplicated child descriptors: the first wins
    same = t.rand_desc()
    for _ in range(G + 3):
        n = t.add(0, same)
        for _ in range(3):
            t.add(n, same ^ 1)
    out["duplicated child descriptors"] = t.finish(k=G + 3, L=2, shuffle=True)
    return out


WALK_TREES = walk_trees()
WALK_COUNTS = sorted({0, 1, G - 1, G, G + 1, 63, 64, 65, 257, 1000})


def walk_queries(voc, n, seed):
    """random descriptors, every node's own descriptor, and descriptors one bit off a node's"""
    rng = np.random.default_rng(seed)
    own = [nd["desc"] for i, nd in sorted(voc.nodes.items()) if i]
    qs = own[:n // 3] + [d ^ (1 << int(rng.integers(0, 256))) for d in own[:n // 3]]
    while len(qs) < n:
        qs.append(B.desc_int(rng.integers(0, 1 << 32, 8, dtype=np.uint64)))
    return [qs[j] for j in rng.permutation(n)]


@pytest.mark.parametrize("name", sorted(WALK_TREES))
def test_walk_equals_the_rule(ft, name):
    voc = use(ft, WALK_TREES[name])
    qs = walk_queries(voc, max(WALK_COUNTS), 11)
    want = [voc.word(d) for d in qs]
    arr = B.descs_array(qs)
    dev = Dev(arr.nbytes, arr)
    try:
        for n in WALK_COUNTS:
            for src in (arr[:n], dev.ptr):
                got = ft.bow_transform(src, n=n)
                assert got["word"].tolist() == [w for w, _ in want[:n]], (name, n)
                assert got["weight"].tobytes() == bits([w for _, w in want[:n]]), (name, n)
        ft.latency_stats(reset=True)
        for n in WALK_COUNTS:
            ft.bow_transform(arr[:n]), ft.bow_transform(dev.ptr, n=n)
        assert ft.latency_stats()["allocs"] == 0  # the second call of a size allocates nothing
    finally:
        dev.free()


@pytest.mark.parametrize("name", ["k 10, L 3", "k 3, L 2"])
def test_transform_sizes_big_small_big_on_one_handle(ft, name):
    """the sort between the walk and the vector runs in scratch of the group's own, of which a memset clears what THIS
    call's tile count and pass count use (two passes for 1000 words, one for 9; the digits are 8 bits wide always):
    4100 descriptors (three sort tiles), 5, one, and 4100 again on one handle — words, weights and the vector as the
    rule's.  With 9 words every tile holds hundreds of each digit."""
    voc = use(ft, WALK_TREES[name])
    qs = walk_queries(voc, 4100, 13)
    want = [voc.word(d) for d in qs]
    for n in (4100, 5, 4100, 1, 2049, 4100):
        got = ft.bow_transform(B.descs_array(qs[:n]))
        assert got["word"].tolist() == [w for w, _ in want[:n]], (name, n)
        vec = voc.vector(qs[:n])
        assert got["n_bow"] == len(vec) and got["bow_word"].tolist() == [w for w, _ in vec], (name, n)
        assert got["bow_value"].tobytes() == bits([v for _, v in vec]), (name, n)


# ---- vector ----------------------------------------------------------------------------------------------------------
def check_vector(ft, voc, qs, what):
    want = voc.vector(qs)
    got = ft.bow_transform(B.descs_array(qs))
    assert got["n_bow"] == len(want), (what, got["n_bow"], len(want))
    assert got["bow_word"].tolist() == [w for w, _ in want], what
    assert got["bow_value"].tobytes() == bits([v for _, v in want]), what
    return want


@pytest.mark.parametrize("weighting", [B.TF_IDF, B.TF, B.IDF, B.BINARY])
def test_vector_equals_the_rule(ft, weighting):
    w7 = B.discriminating_weight(7)
    # stopped words: weight 0 and a negative weight; one word with the discriminating weight
    data, leaves = block_tree((4, 5), weighting, seed=20 + weighting, weights={1: 0.0, 7: -1.5, 13: w7})
    voc = use(ft, data)
    assert [voc.word(d)[0] for d in leaves] == list(range(20)) and voc.word(leaves[13]) == (13, w7)
    rng = np.random.default_rng(5)
    qs = [B.desc_int(rng.integers(0, 1 << 32, 8, dtype=np.uint64)) for _ in range(400)] + leaves * 3
    want = check_vector(ft, voc, qs, "random and every leaf")
    assert len(want) == 18
    for n in (7, 300):  # all descriptors in one word
        want = check_vector(ft, voc, [leaves[13]] * n, "one word %d times" % n)
        assert want == [(13, 1.0)]
    stopped = [leaves[1], leaves[7]]
    assert check_vector(ft, voc, stopped * 5, "stopped words alone") == []
    check_vector(ft, voc, [leaves[13]] * 7 + stopped + qs[:50], "seven, the stopped and fifty")
    # bow_cap below the count: the first pairs, the full count
    full = voc.vector(qs)
    got = ft.bow_transform(B.descs_array(qs), bow_cap=3)
    assert got["n_bow"] == len(full) and got["bow_word"].tolist() == [w for w, _ in full[:3]]
    assert got["bow_value"].tobytes() == bits([v for _, v in full[:3]])
    got = ft.bow_transform(B.descs_array(qs), bow_cap=0)
    assert got["n_bow"] == len(full) and len(got["bow_word"]) == 0


def test_vector_of_weights_that_are_all_zero_is_empty(ft):
    t = B.TreeBuilder(30)
    for j in range(3):
        n = t.add(0)
        for i in range(3):
            t.add(n, weight=0.0)
    voc = use(ft, t.finish(k=3, L=2))
    qs = walk_queries(voc, 100, 3)
    assert check_vector(ft, voc, qs, "every weight 0") == []
    assert ft.bow_add(B.descs_array(qs)) == 0 and ft.bow_query(B.descs_array(qs), 4, -1) == []  # an empty entry, absent


def test_vector_keeps_the_order_of_the_norm_s_additions(ft):
    data, picks, seed = B.discriminating_norm_case()
    voc = use(ft, data)
    want = check_vector(ft, voc, picks, "the discriminating norm case")
    assert len(want) > 20


def test_vector_of_more_words_than_the_norm_chain_stages_at_a_time(ft):
    data, leaves = block_tree((10, 10, 10, 10))
    voc = use(ft, data)
    n = LIM["vector_block"] * 2 + 1
    rng = np.random.default_rng(8)
    qs = [leaves[int(j)] for j in rng.permutation(len(leaves))[:n]]
    want = check_vector(ft, voc, qs + qs[:40], "two chunks and one word")
    assert len(want) == n


# ---- add / query -----------------------------------------------------------------------------------------------------
def check_query(ft, db, qs, max_ids, what):
    arr = B.descs_array(qs)
    N = len(db.entries)
    assert ft.bow_entries() == N
    for max_id in max_ids:
        want = db.scores(qs, max_id)
        score, present = ft.bow_scores(arr, max_id)
        assert np.flatnonzero(present).tolist() == sorted(want), (what, N, max_id)
        assert score[present].tobytes() == bits([want[e] for e in sorted(want)]), (what, N, max_id)
        for max_results in (1, 4, 64):
            got = ft.bow_query(arr, max_results, max_id)
            ref = B.ranked(want, max_results)
            assert [g[0] for g in got] == [r[0] for r in ref], (what, N, max_id, max_results)
            assert bits([g[1] for g in got]) == bits([r[1] for r in ref]), (what, N, max_id, max_results)


def test_add_and_query_equal_the_rule_as_the_database_grows(ft):
    data, leaves = block_tree((10, 10))
    voc = use(ft, data)
    db = B.Database(voc)
    rng = np.random.default_rng(9)

    def frame(n):
        return [leaves[int(j)] for j in rng.integers(0, len(leaves), n)]
    special = {3: [], 5: leaves[:1], 6: [leaves[j] for j in range(0, 64)], 7: [leaves[j] for j in range(30, 95)]}  # 0, 1, 64, 65 words
    twice = frame(25)
    probe = frame(30)
    check_query(ft, db, probe, (-1, 0, 5), "no entries")
    checkpoints = {1, 2, 65, 300}
    for e in range(300):
        qs = special.get(e, twice if e in (10, 11, 40) else frame(int(rng.integers(5, 40))))
        assert ft.bow_add(B.descs_array(qs)) == db.add(qs) == e
        N = e + 1
        if N in checkpoints:
            max_ids = (-1, 0, -50, N - 1, N, N + 5)
            check_query(ft, db, probe, max_ids, "a probe")
            check_query(ft, db, db_last(db, leaves, qs), max_ids, "the last entry's own descriptors")
    # the entry added twice (and a third time): equal scores, the lower id first, also across the cut at max_results
    assert [r[0] for r in ft.bow_query(B.descs_array(twice), 4, -1)][:3] == [10, 11, 40]
    assert ft.bow_query(B.descs_array(twice), 1, -1)[0][0] == 10 and ft.bow_query(B.descs_array(twice), 2, 41)[1][0] == 11
    check_query(ft, db, twice, (-1, 11, 12), "the entry added twice")
    check_query(ft, db, special[6], (-1,), "64 words")
    check_query(ft, db, special[7] + special[5], (-1, 7), "65 words and one")
    check_query(ft, db, [], (-1,), "no descriptors")
    # fewer results than max_results
    few = ft.bow_query(B.descs_array(leaves[95:96]), 64, -1)
    assert 0 < len(few) < 64 and few == [(e, s) for e, s in db.query(leaves[95:96], 64, -1)]


def db_last(db, leaves, qs):
    return qs if qs else leaves[:3]


def test_pools_grow_with_earlier_entries_kept_and_a_reserve_ends_the_allocations():
    data, leaves = block_tree((10, 10))
    rng = np.random.default_rng(10)
    frames = [[leaves[int(j)] for j in rng.integers(0, len(leaves), 60)] for _ in range(80)]
    first = frames[0]
    ft = FE.FeatureTracker(FE.make_config(67, 45, device=0, max_cnt=40, min_dist=5))  # a handle of its own: pools at their first capacity
    try:
        voc = use(ft, data)
        db = B.Database(voc)
        ft.bow_add(B.descs_array(first)), db.add(first)  # the scratch of this descriptor count, the pools' first capacity
        ft.bow_query(B.descs_array(first), 4, -1)
        ft.latency_stats(reset=True)
        for qs in frames[1:40]:  # ~ 45 words each: past the pools' first 1024 words
            ft.bow_add(B.descs_array(qs)), db.add(qs)
        assert sum(len(v) for v in db.entries) > 1024 and ft.latency_stats()["allocs"] > 0
        check_query(ft, db, first, (-1, 20), "after the pools grew")
        ft.bow_clear()
        assert ft.bow_entries() == 0 and ft.bow_query(B.descs_array(first), 4, -1) == []
        db = B.Database(voc)
        ft.bow_reserve(81, 81 * 60)
        ft.latency_stats(reset=True)
        for qs in frames:
            ft.bow_query(B.descs_array(qs), 4, -1)
            ft.bow_add(B.descs_array(qs)), db.add(qs)
        ft.detect_loop(B.descs_array(first), 80), db.add(first)
        assert ft.latency_stats()["allocs"] == 0
        check_query(ft, db, first, (-1, 3, 81), "inside the reserve")
    finally:
        ft.close()


def test_a_query_vector_one_word_longer_than_fits_in_lds(ft):
    data, leaves = block_tree((10, 10, 10, 10))
    voc = use(ft, data)
    db = B.Database(voc)
    lds = LIM["lds_words"]
    assert len(leaves) == 10000 and lds + 1 <= len(leaves)
    rng = np.random.default_rng(12)
    order = [leaves[int(j)] for j in rng.permutation(len(leaves))]
    for qs in (order[:lds + 1], order[100:165], order[lds:lds + 1], order[:lds], order[5000:5064], []):
        assert ft.bow_add(B.descs_array(qs)) == db.add(qs)
    assert len(db.entries[0]) == lds + 1  # distinct words by construction
    check_query(ft, db, order[:lds + 1], (-1, 2), "one word more than fits")
    check_query(ft, db, order[:lds], (-1,), "exactly what fits")
    check_query(ft, db, order[50:lds + 300], (-1,), "longer still")


def test_scores_keep_the_order_of_their_additions(ft):
    data, entry, query, seed = B.discriminating_score_case()
    voc = use(ft, data)
    db = B.Database(voc)
    ft.bow_add(B.descs_array(entry)), db.add(entry)
    check_query(ft, db, query, (-1,), "the discriminating score case")


# ---- detect loop -----------------------------------------------------------------------------------------------------
def test_detect_loop_equals_the_rule_index_by_index(ft):
    data, leaves = block_tree((10, 10))
    voc = use(ft, data)
    db = B.Database(voc)
    rng = np.random.default_rng(13)
    frames = [[leaves[int(j)] for j in rng.integers(0, len(leaves), 12)] for _ in range(60)]
    frames[55] = frames[2]
    found = []
    for f, qs in enumerate(frames):
        want_m, want_R = db.detect_loop(qs, f)
        m, R = ft.detect_loop(B.descs_array(qs), f)
        assert m == want_m and [r[0] for r in R] == [r[0] for r in want_R], (f, m, want_m)
        assert bits([r[1] for r in R]) == bits([r[1] for r in want_R]), f
        assert ft.bow_entries() == f + 1
        found.append(m)
    # frame 55 is frame 2 again: entry 2 leads the results; the rule then prefers any lower id above 0.015
    assert found[55] == 0 and ft.bow_query(B.descs_array(frames[2]), 1, 5)[0][0] == 2 and all(m == -1 for m in found[:51])


# ---- chain -----------------------------------------------------------------------------------------------------------
def scene(shape, seed):
    """noise: corners everywhere, the first kp_capacity of them in raster order are the keyframe's"""
    return np.random.default_rng(100 + seed).integers(0, 256, (shape[1], shape[0]), dtype=np.uint8)


def test_describe_detect_loop_and_match_stay_on_the_device():
    shape, cap = (346, 260), 48
    data = B.full_tree((10, 10), seed=14)
    voc = B.Vocabulary(data)
    db = B.Database(voc)
    pattern = FE.load_brief_pattern(os.path.join(GOLDEN, "brief_pattern.yml"))
    rng = np.random.default_rng(15)
    window = np.stack([rng.uniform(30, 300, 20), rng.uniform(30, 220, 20)], 1).astype(np.float32)
    t = FE.FeatureTracker(FE.make_config(shape[0], shape[1], device=0, max_cnt=40, min_dist=5))
    bufs = []
    try:
        t.kf_set_pattern(*pattern)
        t.bow_set_vocabulary(data)
        host, found = [], []
        for f in range(56):
            img = scene(shape, 2 if f == 55 else f)
            h = t.keyframe_describe(img, window, kp_capacity=cap)
            k = len(h["kp_desc"])
            assert k > 10
            wd, kd = Dev(len(window) * 32), Dev(cap * 32)
            bufs += [wd, kd]
            d = t.keyframe_describe(img, window, kp_capacity=cap, device_desc=(wd.ptr, kd.ptr))
            assert np.array_equal(d["kp_xy"], h["kp_xy"])
            m, R = t.detect_loop(kd.ptr, f, n=k)  # the descriptors never leave the device
            want_m, want_R = db.detect_loop([B.desc_int(w) for w in h["kp_desc"]], f)
            assert m == want_m and [r[0] for r in R] == [r[0] for r in want_R] and bits([r[1] for r in R]) == bits([r[1] for r in want_R]), f
            host.append((h, k))
            found.append(m)
        assert found[55] >= 0 and R[0][0] == 2  # frame 2 again: entry 2 leads; the rule may prefer a lower id
        old, k_old = host[found[55]]
        got = t.kf_match(bufs[2 * 55].ptr, bufs[2 * found[55] + 1].ptr, nq=len(window), nt=k_old)
        via_host = t.kf_match(host[55][0]["window_desc"], old["kp_desc"])
        want = K.match(host[55][0]["window_desc"], old["kp_desc"])
        for a, b, c in zip(got, via_host, want):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    finally:
        for b in bufs:
            b.free()
        t.close()


# ---- isolation -------------------------------------------------------------------------------------------------------
def test_bow_calls_between_track_calls_with_batches_announced_change_no_later_result():
    from esvio_amd.events import event_times
    from esvio_amd.synth import SceneStream
    W, H = 346, 260
    s = SceneStream(W, H, rate=1e6, seed=3, n_rect=12, size=(30.0, 90.0))
    batches = [s.next_batch()[:2] for _ in range(6)]
    data, leaves = block_tree((10, 10))
    voc = B.Vocabulary(data)
    rng = np.random.default_rng(16)
    frames = [[leaves[int(j)] for j in rng.integers(0, len(leaves), 200)] for _ in range(6)]
    results = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
               "right_pts_velocity")

    def run(bow):
        t = FE.FeatureTracker(FE.make_config(W, H, device=0, max_cnt=60, min_dist=8, f_ransac=1))
        db = B.Database(voc)
        out = []
        try:
            if bow:
                t.bow_set_vocabulary(data)
            nxt = 1
            for k, (L, R) in enumerate(batches):
                while nxt < len(batches) and nxt <= k + 2:  # two batches ahead (the first call is a plain one)
                    t.set_next_batch(event_times(batches[nxt][0])[-1], batches[nxt][0], batches[nxt][1], True)
                    nxt += 1
                if bow:
                    arr = B.descs_array(frames[k])
                    assert t.bow_transform(arr)["bow_word"].tolist() == [w for w, _ in voc.vector(frames[k])]
                    got = t.bow_query(arr, 4, -1)
                    assert [g[0] for g in got] == [r[0] for r in db.query(frames[k], 4, -1)]
                    assert t.detect_loop(arr, k)[0] == db.detect_loop(frames[k], k)[0]
                t.trackEvent(event_times(L)[-1], L, R, True)
                out.append({n: np.array(getattr(t, n)) for n in results})
        finally:
            t.close()
        return out
    plain, mixed = run(False), run(True)
    assert len(plain[-1]["ids"]) > 10
    for k, (a, b) in enumerate(zip(plain, mixed)):
        for n in results:
            assert np.array_equal(a[n], b[n]), (k, n)


def test_reset_keeps_vocabulary_and_database_clear_empties_it_and_a_new_vocabulary_needs_it_empty(ft):
    data, leaves = block_tree((10, 10))
    voc = use(ft, data)
    db = B.Database(voc)
    for j in range(5):
        qs = leaves[10 * j:10 * j + 15]
        ft.bow_add(B.descs_array(qs)), db.add(qs)
    ft.reset()
    assert ft.bow_entries() == 5
    check_query(ft, db, leaves[5:30], (-1, 2), "after a reset")
    L, h = ft._hd.L, ft._hd.h
    other = B.full_tree((3, 3), seed=1)
    assert L.esvio_fe_bow_set_vocabulary(h, other, len(other)) == -1
    assert L.esvio_fe_last_error(h).decode().startswith("bow_set_vocabulary") and ft.bow_entries() == 5
    check_query(ft, db, leaves[5:30], (-1,), "after the refused vocabulary")
    ft.bow_clear()
    assert ft.bow_entries() == 0 and ft.bow_scores(B.descs_array(leaves[:5]))[0].size == 0
    ft.bow_set_vocabulary(other)
    v2 = B.Vocabulary(other)
    qs = walk_queries(v2, 20, 1)
    assert ft.bow_transform(B.descs_array(qs))["word"].tolist() == [v2.word(d)[0] for d in qs]


def test_every_argument_error_is_einval_with_a_message_and_leaves_the_handle_usable(ft):
    data, leaves = block_tree((10, 10))
    L, h, p = ft._hd.L, ft._hd.h, FE._p
    desc, n, m = B.descs_array(leaves[:4]), C.c_int32(0), C.c_int32(0)
    res, bw, bv = (FE.BowResult * 64)(), np.zeros(8, np.uint32), np.zeros(8, np.float64)
    sc, pr = np.zeros(8, np.float64), np.zeros(8, np.uint8)
    dev = Dev(256)
    # before a vocabulary: a fresh handle refuses every call but the three that need none
    t = FE.FeatureTracker(FE.make_config(67, 45, device=0, max_cnt=40, min_dist=5))
    try:
        h2 = t._hd.h
        assert L.esvio_fe_bow_entries(h2) == 0
        for call in (lambda: L.esvio_fe_bow_transform(h2, p(desc), 4, FE.HOST, None, None, None, None, 0, C.byref(n)),
                     lambda: L.esvio_fe_bow_add(h2, p(desc), 4, FE.HOST, None),
                     lambda: L.esvio_fe_bow_query(h2, p(desc), 4, FE.HOST, 4, -1, res, C.byref(n)),
                     lambda: L.esvio_fe_bow_detect_loop(h2, p(desc), 4, FE.HOST, 3, C.byref(m), None, None),
                     lambda: L.esvio_fe_bow_scores(h2, p(desc), 4, FE.HOST, -1, p(sc), p(pr)),
                     lambda: L.esvio_fe_bow_clear(h2), lambda: L.esvio_fe_bow_reserve(h2, 4, 4)):
            assert call() == -1 and "no vocabulary" in L.esvio_fe_last_error(h2).decode()
        bad = data[:-1]
        assert L.esvio_fe_bow_set_vocabulary(h2, bad, len(bad)) == -1 and "byte count" in L.esvio_fe_last_error(h2).decode()
        l2 = B.serialise(10, 2, 1, 0, [(1, 0, 1.0, 0)], [(1, 0)])
        assert L.esvio_fe_bow_set_vocabulary(h2, l2, len(l2)) == -4 and "scoring" in L.esvio_fe_last_error(h2).decode()
        assert L.esvio_fe_bow_set_vocabulary(h2, None, 10) == -1
    finally:
        t.close()
    voc = use(ft, data)
    calls = {
        "transform: bad space": lambda: L.esvio_fe_bow_transform(h, p(desc), 4, 5, None, None, None, None, 0, C.byref(n)),
        "transform: negative n": lambda: L.esvio_fe_bow_transform(h, p(desc), -1, FE.HOST, None, None, None, None, 0, C.byref(n)),
        "transform: n above the limit": lambda: L.esvio_fe_bow_transform(h, p(desc), (1 << 20) + 1, FE.HOST, None, None, None, None, 0, C.byref(n)),
        "transform: null desc": lambda: L.esvio_fe_bow_transform(h, None, 4, FE.HOST, None, None, None, None, 0, C.byref(n)),
        "transform: unaligned device desc": lambda: L.esvio_fe_bow_transform(h, C.c_void_p(dev.ptr + 8), 1, FE.DEVICE, None, None, None, None, 0, C.byref(n)),
        "transform: negative bow_cap": lambda: L.esvio_fe_bow_transform(h, p(desc), 4, FE.HOST, None, None, p(bw), p(bv), -1, C.byref(n)),
        "transform: bow_cap without bow_word": lambda: L.esvio_fe_bow_transform(h, p(desc), 4, FE.HOST, None, None, None, p(bv), 4, C.byref(n)),
        "transform: bow_cap without n_bow": lambda: L.esvio_fe_bow_transform(h, p(desc), 4, FE.HOST, None, None, p(bw), p(bv), 4, None),
        "add: bad space": lambda: L.esvio_fe_bow_add(h, p(desc), 4, -1, None),
        "add: null desc": lambda: L.esvio_fe_bow_add(h, None, 4, FE.HOST, None),
        "query: max_results 0": lambda: L.esvio_fe_bow_query(h, p(desc), 4, FE.HOST, 0, -1, res, C.byref(n)),
        "query: max_results -1": lambda: L.esvio_fe_bow_query(h, p(desc), 4, FE.HOST, -1, -1, res, C.byref(n)),
        "query: max_results 65": lambda: L.esvio_fe_bow_query(h, p(desc), 4, FE.HOST, 65, -1, res, C.byref(n)),
        "query: null results": lambda: L.esvio_fe_bow_query(h, p(desc), 4, FE.HOST, 4, -1, None, C.byref(n)),
        "query: null n_results": lambda: L.esvio_fe_bow_query(h, p(desc), 4, FE.HOST, 4, -1, res, None),
        "query: n above the limit": lambda: L.esvio_fe_bow_query(h, p(desc), (1 << 20) + 1, FE.HOST, 4, -1, res, C.byref(n)),
        "detect_loop: null loop_index": lambda: L.esvio_fe_bow_detect_loop(h, p(desc), 4, FE.HOST, 3, None, None, None),
        "detect_loop: negative frame_index": lambda: L.esvio_fe_bow_detect_loop(h, p(desc), 4, FE.HOST, -1, C.byref(m), None, None),
        "detect_loop: results without n_results": lambda: L.esvio_fe_bow_detect_loop(h, p(desc), 4, FE.HOST, 3, C.byref(m), res, None),
        "detect_loop: bad space": lambda: L.esvio_fe_bow_detect_loop(h, p(desc), 4, 2, 3, C.byref(m), None, None),
        "scores: null score": lambda: L.esvio_fe_bow_scores(h, p(desc), 4, FE.HOST, -1, None, p(pr)),
        "scores: negative n": lambda: L.esvio_fe_bow_scores(h, p(desc), -4, FE.HOST, -1, p(sc), p(pr)),
        "reserve: negative entries": lambda: L.esvio_fe_bow_reserve(h, -1, 10),
        "reserve: negative words": lambda: L.esvio_fe_bow_reserve(h, 10, -1),
    }
    try:
        db = B.Database(voc)
        ft.bow_add(desc), db.add(leaves[:4])
        ft.bow_query(desc, 4, -1), ft.detect_loop(desc, 1), db.add(leaves[:4])
        ft.latency_stats(reset=True)
        for name, call in calls.items():
            L.esvio_fe_reset(h)  # (clears nothing of the message: each refusal must write its own)
            assert call() == -1, name
            msg = L.esvio_fe_last_error(h).decode()
            assert msg.startswith("bow_" + name.split(":")[0]), (name, msg)
        assert ft.latency_stats()["allocs"] == 0 and ft.bow_entries() == 2  # refused before any device work
        check_query(ft, db, leaves[:9], (-1,), "after the refusals")
    finally:
        dev.free()


def test_the_group_s_kernels_are_booked_in_their_own_table(ft):
    data, leaves = block_tree((10, 10))
    use(ft, data)
    ft.set_profiling(True)
    ft.reset_kernel_stats()
    before = ft.bow_kernel_stats()
    ft.bow_add(B.descs_array(leaves[:20]))
    ft.bow_query(B.descs_array(leaves[:20]), 4, -1)
    after = ft.bow_kernel_stats()
    assert list(after) == ["k_bow_walk", "k_bow_vector", "k_bow_score", "k_bow_select"]
    assert [after[k]["launches"] - before[k]["launches"] for k in after] == [2, 2, 1, 1]
    assert all(after[k]["alg_bytes"] > before[k]["alg_bytes"] for k in after)
    ft.set_profiling(False)
