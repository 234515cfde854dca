"""CPU: tests/bow_create_ref.py, the sequential reading of rule C (include/esvio_fe.h "C, creating a vocabulary"), held to
answers worked out by hand on inputs of a few bits, its draws to splitmix64's published outputs, and its array form to its
loop form.  The traces are in the docstrings: a reader can check them with a pencil."""
import math

import numpy as np

import bow_create_ref as R
import bow_ref as B
from esvio_amd import frontend as FE

MAX = 2147483647  # the largest draw: RandomValue gives the whole sum


def index_draw(i, m):
    """a draw r with RandomInt(0, m - 1) == i"""
    r = (i * (1 << 31) + m - 1) // m
    assert R.random_int(r, m) == i
    return r


def first_then_whole(key, j, path):
    """draw 0 picks feature 0, every later draw makes cut_d the whole sum: the last feature with min_dist > 0"""
    return 0 if j == 0 else MAX


def accepted(data):
    B.parse(data)
    rc, hdr = FE.bow_vocabulary_header(data)
    assert rc == 0, hdr["message"]
    return hdr


def test_splitmix64_against_its_published_outputs():
    # the first outputs of Vigna's splitmix64.c for the states 1234567 and 0
    gamma = 0x9E3779B97F4A7C15
    want = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    assert [R.mix((1234567 + j * gamma) & R.M64) for j in range(5)] == want
    assert R.mix(0) == 0xE220A8397B1DCDAF
    key = R.root_key(5)
    assert R.child_key(key, 2) == R.mix(key ^ 3) and R.c5_draw(key, 1) == R.mix(key ^ (2 << 32)) >> 33 < 1 << 31
    assert R.random_int(MAX, 7) == 6 and R.random_int(0, 7) == 0 and R.random_value(MAX, 18) == 18.0 and R.random_value(0, 18) == 0.0


def test_ties_the_even_majority_a_shallow_leaf_a_redrawn_zero_and_a_cut_on_a_running_sum():
    """k = 2, L = 2, features 0000 0011 0001 0010 1111, documents {f0} {f1..f4}.
    Root: draw 0 -> f0.  min_dist 0 2 1 1 4, sum 8, cut 8.0: running 0 2 3 4 8 -> f4 (the cut equals a running sum).
    Pass 1, centres 0000 1111: 0011 is 2 from both -> cluster 0 (the lowest).  Groups {f0 f1 f2 f3} {f4}.
    Pass 2: cluster 0 has four features, bits 0 and 1 are set in two each: exactly half, clear -> 0000.  Same groups: 2 passes.
    Node 2 = 1111 has one feature: a leaf at depth 1.  Node 1 is split: draw 0 -> rank 1 (0011); min_dist 2 0 1 1, sum 4;
    draw 1 is 0 -> cut 0.0, drawn again; draw 2 -> cut 4.0: running 2 2 3 4 -> 0010.  Pass 1, centres 0011 0010: groups
    {0011 0001} {0000 0010}.  Pass 2: means 0001 (bit 1 in one of two: clear) and 0000; same groups.
    Walks: f0 -> node 4, f1 -> node 1 (tie) -> node 3, f2 -> node 3, f3 -> node 4, f4 -> node 2.  Ni = 1 1 2 of 2 documents."""
    feats = [0b0000, 0b0011, 0b0001, 0b0010, 0b1111]

    def draw(key, j, path):
        if path == ():
            return first_then_whole(key, j, path)
        assert path == (0,) and j < 3
        return (index_draw(1, 4), 0, MAX)[j]
    data, info = R.create_loops(feats, [0, 1, 5], 2, 2, draw=draw)
    ln2 = math.log(2.0 / 1.0)
    assert data == B.serialise(2, 2, 0, 0, [(1, 0, 0.0, 0b0000), (2, 0, ln2, 0b1111), (3, 1, ln2, 0b0001), (4, 1, math.log(2.0 / 2.0), 0b0000)],
                               [(2, 0), (3, 1), (4, 2)])
    assert info == dict(nodes=4, words=3, depth=2, max_children=2, kmeans_nodes=2, passes=2, empty_clusters=0, short_seedings=0, bytes=len(data))
    assert accepted(data)["leaves"] == 3
    assert R.create_numpy(B.descs_array(feats), [0, 1, 5], 2, 2, draw=draw) == (data, info)


def test_ids_are_the_depth_first_creation_order():
    """k = 2, L = 3, features a0 b0 a1 b1 a2 b2 with a = 0000 xxxx, b = 1111 xxxx and xxxx = 0000 0001 0110.
    Root: f0 = a0, min_dist 0 4 1 5 2 6, cut 18.0 -> b2.  Pass 1 splits a from b; pass 2's means are 00000000 (every low
    bit in one of three) and 11110000; same groups.  Node 1 (the a): a0, min_dist 0 1 2, cut 3.0 -> a2; groups {a0 a1} {a2},
    means 0000 (bit 0 in one of two) and 0110.  Node 3 = {a0 a1} has two features, m <= k: nodes 5 and 6 are the features.
    Node 2 (the b) likewise: nodes 7 8, then 9 10.  Breadth first would have numbered node 2's children 5 and 6."""
    a = [0b00000000, 0b00000001, 0b00000110]
    b = [0b11110000 | x for x in a]
    feats = [a[0], b[0], a[1], b[1], a[2], b[2]]
    data, info = R.create_loops(feats, [0, 2, 2, 6], 2, 3, draw=first_then_whole)
    w = math.log(3.0 / 1.0)
    nodes = [(1, 0, 0.0, 0), (2, 0, 0.0, 0b11110000), (3, 1, 0.0, 0), (4, 1, w, a[2]), (5, 3, w, a[0]), (6, 3, w, a[1]),
             (7, 2, 0.0, 0b11110000), (8, 2, w, b[2]), (9, 7, w, b[0]), (10, 7, w, b[1])]
    assert data == B.serialise(2, 3, 0, 0, nodes, [(4, 0), (5, 1), (6, 2), (8, 3), (9, 4), (10, 5)])
    assert (info["nodes"], info["words"], info["depth"], info["kmeans_nodes"], info["passes"]) == (10, 6, 3, 3, 2)
    accepted(data)
    assert R.create_numpy(B.descs_array(feats), [0, 2, 2, 6], 2, 3, draw=first_then_whole) == (data, info)


def test_an_empty_cluster_has_the_zero_centre_and_the_weight_zero():
    """k = 3, L = 1, features 0100 0011 0101 0010 1010; draw 0 -> f4, cut 10.0 of min_dist 3 2 4 1 0 -> f3 = 0010; min_dist
    2 1 3 0 0, sum 6, cut just below 3 -> f1 = 0011.  Pass 1 (1010 0010 0011): 1 2 2 1 0.  Pass 2 (1010 0000 0001): 1 2 2 0 0,
    f3 being 1 from clusters 0 and 1.  Pass 3 (0010 0100 0001): 1 0 1 0 0 — f1 ties clusters 0 and 2, f2 clusters 1 and 2.
    Pass 4 (0010 0100 and, for the empty group, 0000): 1 0 1 0 0 again.  Walks end in words 1 0 1 0 0: Ni = 1 2 0 of 3."""
    feats = [0b0100, 0b0011, 0b0101, 0b0010, 0b1010]
    draws = (index_draw(4, 5), MAX, MAX * 2 // 4)
    data, info = R.create_loops(feats, [0, 1, 1, 5], 3, 1, draw=lambda key, j, path: draws[j])
    assert data == B.serialise(3, 1, 0, 0, [(1, 0, math.log(3.0 / 1.0), 0b0010), (2, 0, math.log(3.0 / 2.0), 0b0100), (3, 0, 0.0, 0)],
                               [(1, 0), (2, 1), (3, 2)])
    assert (info["passes"], info["empty_clusters"], info["kmeans_nodes"], info["max_children"]) == (4, 1, 1, 3)
    accepted(data)
    assert R.create_numpy(B.descs_array(feats), [0, 1, 1, 5], 3, 1, draw=lambda key, j, path: draws[j]) == (data, info)


def test_duplicates_of_a_small_node_stay_and_the_later_one_is_never_walked_to():
    """k = 3, L = 2, features 0101 0101 0010: m <= k, one child each and no level below (one feature each).  Both 0101
    walk to node 1, the first of the equal distances: Ni = 1 0 1 of 3 documents."""
    data, info = R.create_loops([5, 5, 2], [0, 2, 3, 3], 3, 2)
    w = math.log(3.0 / 1.0)
    assert data == B.serialise(3, 2, 0, 0, [(1, 0, w, 5), (2, 0, 0.0, 5), (3, 0, w, 2)], [(1, 0), (2, 1), (3, 2)])
    assert info == dict(nodes=3, words=3, depth=1, max_children=3, kmeans_nodes=0, passes=0, empty_clusters=0, short_seedings=0, bytes=len(data))
    accepted(data)


def test_an_all_identical_input_is_a_chain_of_single_children_down_to_level_L():
    """every seeding stops at dist_sum == 0 with one centre; the one child holds every feature and is split again"""
    for weighting, w in ((B.TF_IDF, math.log(2.0 / 2.0)), (B.TF, 1.0), (B.IDF, 0.0), (B.BINARY, 1.0)):
        data, info = R.create_loops([0b101] * 3, [0, 1, 3], 2, 3, weighting=weighting)
        assert data == B.serialise(2, 3, 0, weighting, [(1, 0, 0.0, 5), (2, 1, 0.0, 5), (3, 2, w, 5)], [(3, 0)])
        assert info == dict(nodes=3, words=1, depth=3, max_children=1, kmeans_nodes=3, passes=2, empty_clusters=0, short_seedings=3, bytes=len(data))
        accepted(data)


def test_the_guard_and_the_default_draws():
    desc = R.uniform(300, 1)
    data, info = R.create_numpy(desc, [0, 300], 4, 2, seed=3)
    assert info["passes"] > 2 and R.create_numpy(desc, [0, 300], 4, 2, seed=3) == (data, info)
    assert R.create_numpy(desc, [0, 300], 4, 2, seed=4)[0] != data
    assert R.create_numpy(desc, [0, 300], 4, 2, seed=3, max_passes=info["passes"]) == (data, info)
    for form in (R.create_numpy, R.create_loops):
        try:
            form(desc, [0, 300], 4, 2, seed=3, max_passes=2)
            raise AssertionError("settled")
        except R.NotSettled as e:
            assert e.nodes >= 1


def test_the_array_form_equals_the_loop_form():
    empties = shorts = 0
    for s in range(220):
        rng = np.random.default_rng(s)
        n, k, L = int(rng.integers(1, 70)), int(rng.integers(2, 6)), int(rng.integers(1, 4))
        if s % 2:
            desc = R.low_entropy(n, s)
            desc[:, 0] &= 0x0f0f if s % 4 == 1 else 0xffff
        else:
            desc = R.prototypes(n, 3, 0.05, s)
        docs = sorted(int(x) for x in rng.integers(0, n + 1, int(rng.integers(0, 5))))
        docs = [0] + docs + [n]
        a = R.create_loops(desc, docs, k, L, weighting=s % 4, seed=s)
        assert a == R.create_numpy(desc, docs, k, L, weighting=s % 4, seed=s), s
        hdr = accepted(a[0])
        assert (hdr["nodes"], hdr["words"], hdr["depth"], hdr["max_children"]) == tuple(a[1][f] for f in ("nodes", "words", "depth", "max_children"))
        empties += a[1]["empty_clusters"]
        shorts += a[1]["short_seedings"]
    assert empties > 0 and shorts > 0
