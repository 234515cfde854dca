"""CPU: tests/bow_ref.py, the sequential reading of the rules in include/esvio_fe.h "loop detection", held to answers
worked out by hand on a k = 2, L = 2 tree, to what the reference's own BowVector.cpp (compiled unchanged, recorded in
tests/golden/bow_vector_ref.npz) leaves for seeded inputs, and to the quirks of the loop decision; and a check that the
inputs the device tests use can tell a wrong order of additions from the right one."""
import os

import numpy as np

import bow_ref as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL, LOW64 = (1 << 256) - 1, (1 << 64) - 1


def hand_tree(weighting=B.TF_IDF):
    """root -> A (all 0), B (all 1); A -> A1 (all 0; word 0, weight 1), A2 (low 64 bits; word 1, weight 2);
    B -> B1 (all 1; word 2, weight 0.5), B2 (all 1 but the low 64; word 3, weight 4)"""
    t = B.TreeBuilder()
    a, b = t.add(0, 0, 0.0), t.add(0, ALL, 0.0)
    t.add(a, 0, 1.0), t.add(a, LOW64, 2.0), t.add(b, ALL, 0.5), t.add(b, ALL ^ LOW64, 4.0)
    return B.Vocabulary(t.finish(k=2, L=2, weighting=weighting))


def test_the_file_round_trips_and_children_are_in_record_order():
    t = B.TreeBuilder(1)
    t.full([3, 2])
    plain, shuffled = B.Vocabulary(t.finish(k=3, L=2)), B.Vocabulary(t.finish(k=3, L=2, shuffle=True))
    assert plain.header == dict(k=3, L=2, scoring=0, weighting=0, nodes=9, words=6)
    assert plain.nodes[0]["children"] == [1, 4, 7] and plain.nodes[1]["children"] == [2, 3]
    assert sorted(shuffled.nodes[0]["children"]) == [1, 4, 7] and shuffled.nodes[0]["children"] != [1, 4, 7]
    assert [plain.nodes[i]["word"] for i in (2, 3, 5, 6, 8, 9)] == list(range(6))


def test_words_on_the_hand_made_tree():
    v = hand_tree()
    assert v.word(0) == (0, 1.0)
    assert v.word((1 << 60) - 1) == (1, 2.0)  # A: 60 against 196; A1: 60, A2: 4
    assert v.word(ALL) == (2, 0.5)
    assert v.word(ALL ^ ((1 << 32) - 1)) == (2, 0.5)  # B1 and B2 both at 32: the first
    assert v.word((1 << 128) - 1) == (1, 2.0)  # A and B both at 128: A; then A1: 128, A2: 64


def test_vectors_on_the_hand_made_tree():
    q = [0, 0, (1 << 60) - 1]
    assert hand_tree(B.TF_IDF).vector(q) == [(0, 0.5), (1, 0.5)]  # 1 + 1 and 2 over 4
    assert hand_tree(B.TF).vector(q) == [(0, 0.5), (1, 0.5)]
    assert hand_tree(B.IDF).vector(q) == [(0, 1.0 / 3.0), (1, 2.0 / 3.0)]  # 1 and 2 over 3
    assert hand_tree(B.BINARY).vector(q) == [(0, 1.0 / 3.0), (1, 2.0 / 3.0)]
    assert hand_tree().vector([]) == []
    t = B.TreeBuilder()
    t.add(0, 0, 0.0), t.add(0, ALL, -1.0)
    assert B.Vocabulary(t.finish()).vector([0, ALL, ALL]) == []  # weight 0 and a negative weight: stopped


def test_scores_on_the_hand_made_tree():
    v = hand_tree()
    db = B.Database(v)
    q = [0, 0, (1 << 60) - 1]
    assert db.query(q, 4, -1) == []
    assert (db.add(q), db.add([ALL]), db.add([0, ALL]), db.add([])) == (0, 1, 2, 3)
    assert db.entries[1] == [(2, 1.0)] and db.entries[2] == [(0, 1.0 / 1.5), (2, 0.5 / 1.5)] and db.entries[3] == []
    s = db.scores(q, -1)
    s2 = abs(0.5 - 1.0 / 1.5) - 0.5 - 1.0 / 1.5
    assert s == {0: -2.0, 2: s2}  # identical vectors: (0 - 0.5 - 0.5) twice; the disjoint entry 1 is absent
    assert db.query(q, 4, -1) == [(0, 1.0), (2, -s2 / 2.0)]
    assert db.query(q, 1, -1) == [(0, 1.0)]
    assert db.scores(q, 0) == {} and db.scores(q, 1) == {0: -2.0} and db.scores(q, -50) == {}  # (the last entry is empty)
    assert db.scores([0, ALL], 0) == {} and db.scores([ALL], 2) == {1: -2.0}
    db.add([ALL])
    assert db.scores([ALL], 0) == {4: -2.0} and db.scores([ALL], -7) == {4: -2.0}  # the last entry always takes part
    assert db.query([ALL], 4, -1) == [(1, 1.0), (4, 1.0), (2, -(abs(1.0 - 0.5 / 1.5) - 1.0 - 0.5 / 1.5) / 2.0)]  # equal scores: by id


def test_the_vector_equals_the_reference_s_compiled_bowvector():
    z = np.load(os.path.join(GOLDEN, "bow_vector_ref.npz"))
    assert int(z["cases"]) == 16
    for c in range(int(z["cases"])):
        pairs = list(zip(z["in_ids_%d" % c].tolist(), z["in_vals_%d" % c].tolist()))
        got = B.bow_vector(pairs, int(z["mode_%d" % c]) == 0)
        want_ids, want_vals = z["out_ids_%d" % c], z["out_vals_%d" % c]
        assert [w for w, _ in got] == want_ids.tolist(), c
        assert np.array([v for _, v in got], np.float64).tobytes() == want_vals.tobytes(), c


def test_the_device_tests_inputs_discriminate():
    data, picks, seed = B.discriminating_norm_case()
    voc = B.Vocabulary(data)
    vals = {}
    for d in picks:
        wid, w = voc.word(d)
        vals[wid] = vals[wid] + w if wid in vals else w
    ordered = [vals[w] for w in sorted(vals)]
    assert B.sum_asc(ordered) != B.sum_desc(ordered) and B.sum_asc(ordered) != B.sum_pairwise(ordered)
    assert sum(v for _, v in voc.vector(picks)) > 0.99
    w = B.discriminating_weight(7)
    assert ((((((w + w) + w) + w) + w) + w) + w) != 7 * w
    data, entry, query, seed = B.discriminating_score_case()
    voc = B.Vocabulary(data)
    q, e = voc.vector(query), dict(voc.vector(entry))
    terms = [abs(qv - e[wd]) - abs(qv) - abs(e[wd]) for wd, qv in q if wd in e]
    fwd, rev = terms[0], terms[-1]
    for t in terms[1:]:
        fwd += t
    for t in reversed(terms[:-1]):
        rev += t
    assert fwd != rev and B.raw_scores(q, [voc.vector(entry)], -1) == {0: fwd}


def test_the_loop_decision_s_quirks():
    R = [(3, 0.3), (1, 0.02)]
    assert [B.loop_decision(R, f) for f in (49, 50, 51)] == [-1, -1, 1]
    assert B.loop_decision([(5, 0.01), (2, 0.2)], 60) == -1      # R[0] at or below 0.05: nothing found
    assert B.loop_decision([(3, 0.9)], 60) == -1                 # |R| = 1: no second result above 0.015
    assert B.loop_decision([(7, 0.3), (2, 0.01), (5, 0.02)], 60) == 5  # a lower id counts only above 0.015
    assert B.loop_decision([(2, 0.3), (7, 0.2)], 60) == 2        # R[0] is taken first, a higher id never replaces it
    assert B.loop_decision([], 60) == -1


def test_detect_loop_queries_then_adds_and_max_id_follows_the_frame_index():
    v = hand_tree()
    db = B.Database(v)
    for f in range(49):
        db.add([0] if f % 2 else [ALL])
    m, R = db.detect_loop([0], 49)  # max_id -1: every entry takes part
    assert m == -1 and len(R) == 4 and [r[0] for r in R] == [1, 3, 5, 7] and len(db.entries) == 50
    m, R = db.detect_loop([ALL], 50)  # max_id 0: the last entry alone, and it holds word 0
    assert (m, R) == (-1, [])
    m, R = db.detect_loop([ALL], 51)  # max_id 1: entry 0 and the last one
    assert m == 0 and R == [(0, 1.0), (50, 1.0)]
