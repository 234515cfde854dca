"""GPU: esvio_fe_bow_create_vocabulary against tests/bow_create_ref.py, the sequential reading of rule C in
include/esvio_fe.h — the file image byte for byte, the counters value for value.  Nothing has a tolerance: the rule is
integer arithmetic, one double division and product per draw, and the host's log.  The sizes are the smallest that reach
each edge: m <= k against m = k + 1, one wave, one workgroup, one scan tile, the size at which a node's bit counts go
through memory (4096 features), many small nodes in one workgroup, the deepest and the widest tree the rule allows."""
import ctypes as C
import os

import numpy as np
import pytest

import bow_create_ref as R
import bow_ref as B
from esvio_amd import frontend as FE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INFO = ("nodes", "words", "depth", "max_children", "kmeans_nodes", "passes", "empty_clusters", "short_seedings", "bytes")


@pytest.fixture(scope="module")
def ft():
    t = FE.FeatureTracker(FE.make_config(67, 45, device=0, max_cnt=40, min_dist=5))
    yield t
    t.close()


class Dev:
    """device memory of the library's runtime"""

    def __init__(self, data):
        a = np.ascontiguousarray(data)
        self.L, self.p = FE.load_library(), C.c_void_p()
        assert self.L.esvio_fe_mem_alloc(FE.DEVICE, max(a.nbytes, 16), C.byref(self.p)) == 0
        assert self.L.esvio_fe_mem_upload(self.p, FE._p(a), a.nbytes) == 0

    def free(self):
        self.L.esvio_fe_mem_free(FE.DEVICE, self.p)


_REF = {}


def reference(name, desc, docs, k, L, **kw):
    """the restatement's answer, computed once per case"""
    if name not in _REF:
        _REF[name] = R.create_numpy(desc, docs, k, L, **kw)
    return _REF[name]


def check(ft, name, desc, docs, k, L, **kw):
    want, want_info = reference(name, desc, docs, k, L, **kw)
    rc, info = ft.bow_create_vocabulary(desc, docs, k, L, **kw)
    assert rc == 0 and info["message"] == ""
    print(name, info)
    assert {f: info[f] for f in INFO} == {f: want_info[f] for f in INFO}, name
    got = ft.bow_get_created(info["bytes"])
    assert got == want, name
    hrc, hdr = FE.bow_vocabulary_header(got)
    assert hrc == 0 and (hdr["k"], hdr["L"], hdr["nodes"], hdr["words"]) == (k, L, info["nodes"], info["words"])
    return got, want_info


@pytest.mark.parametrize("n", (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025))
def test_one_segment_at_the_wave_and_workgroup_edges_and_the_switch_to_kmeans(ft, n):
    desc = R.uniform(n, 100 + n)
    _, info = check(ft, "edges %d" % n, desc, R.even_docs(n, min(n, 5)), 3, 2, seed=n)
    assert (info["kmeans_nodes"] == 0) == (n <= 3)
    assert info["passes"] < 50


def test_many_small_nodes_share_a_workgroup_with_duplicates_short_seedings_and_ties(ft):
    desc = R.low_entropy(700, 5)
    desc[:, 0] &= 0x0f0f  # 8 variable bits: 256 distinct descriptors at the most
    _, info = check(ft, "low entropy", desc, R.even_docs(700, 9), 3, 3, seed=21)
    assert info["kmeans_nodes"] > 5 and 2 <= info["passes"] < 50
    rare = np.zeros((40, 8), np.uint32)  # three distinct descriptors, k = 4: every k-means node's seeding stops short
    rare[:, 0] = np.random.default_rng(8).integers(0, 3, 40)
    _, info = check(ft, "three distinct", rare, R.even_docs(40, 4), 4, 3, seed=3)
    assert info["short_seedings"] >= 1


def test_prototypes_with_flips_leave_empty_clusters_and_a_big_root(ft):
    desc = R.prototypes(20000, 40, 0.08, 1)
    _, info = check(ft, "prototypes", desc, R.even_docs(20000, 50), 10, 3, seed=11)
    assert info["empty_clusters"] > 0 and info["kmeans_nodes"] > 10 and info["passes"] < 50


def test_uniform_descriptors_need_many_passes(ft):
    desc = R.uniform(3000, 2)
    _, info = check(ft, "uniform", desc, R.even_docs(3000, 7), 10, 2, seed=11)
    assert 8 <= info["passes"] < 60


def test_the_widest_node_and_a_node_at_the_size_where_counts_go_through_memory(ft):
    desc = R.uniform(4096, 3)
    _, info = check(ft, "k 32", desc, R.even_docs(4096, 7), 32, 1, seed=11)
    assert info["max_children"] == 32 and info["passes"] < 100
    for n in (4095, 4097, 4096 + 2048 + 5):  # below, above, and a big node whose last tile it shares with nobody
        check(ft, "big edge %d" % n, R.prototypes(n, 6, 0.1, n), R.even_docs(n, 3), 4, 2, seed=n)


def test_create_sizes_big_small_big_on_one_handle(ft):
    """both regroupings (the features by node after every level, the words by document at the end) sort in scratch of
    the stage's own, of which a memset clears what each sort's tile and pass count use: 6149 descriptors (four sort
    tiles), 300 (one), 3 (no k-means at all) and 6149 again on one handle, the file image byte for byte each time.
    The digits are 8 bits wide always; the pass count follows the node and word counts of the level."""
    big = dict(desc=R.prototypes(6149, 6, 0.1, 6149), docs=R.even_docs(6149, 3), k=4, L=2, seed=6149)
    small = dict(desc=np.tile(R.uniform(1, 9), (300, 1)), docs=R.even_docs(300, 3), k=4, L=5, seed=2)
    tiny = dict(desc=R.uniform(3, 103), docs=R.even_docs(3, 3), k=3, L=2, seed=3)
    for name, kw in (("big edge 6149", big), ("identical", small), ("big edge 6149", big), ("edges 3", tiny), ("big edge 6149", big)):
        check(ft, name, **kw)


def test_the_deepest_tree(ft):
    desc = R.uniform(2048, 4)
    _, info = check(ft, "k 2 L 10", desc, R.even_docs(2048, 7), 2, 10, seed=11)
    assert info["depth"] == 10 and info["passes"] < 100


def test_an_all_identical_input_gives_a_chain_of_single_children(ft):
    desc = np.tile(R.uniform(1, 9), (300, 1))
    got, info = check(ft, "identical", desc, R.even_docs(300, 3), 4, 5, seed=2)
    assert (info["nodes"], info["words"], info["depth"], info["max_children"], info["short_seedings"]) == (5, 1, 5, 1, 5)


@pytest.mark.parametrize("weighting", (0, 1, 2, 3))
def test_the_four_weightings_with_empty_documents(ft, weighting):
    desc = R.prototypes(900, 12, 0.06, 7)
    docs = [0, 0, 100, 100, 100, 350, 900, 900]
    got, _ = check(ft, "weighting %d" % weighting, desc, docs, 5, 3, weighting=weighting, seed=5)
    _, nodes = B.parse(got)
    w = [nd["weight"] for nd in nodes.values() if not nd["children"]]
    assert all(x == 1.0 for x in w) if weighting in (1, 3) else len(set(w)) > 1


def test_descriptors_in_device_memory_are_read_in_place(ft):
    desc = R.prototypes(1500, 10, 0.08, 3)
    docs = R.even_docs(1500, 6)
    want, want_info = reference("device space", desc, docs, 6, 3, seed=9)
    d = Dev(desc)
    try:
        rc, info = ft.bow_create_vocabulary(d.p.value, docs, 6, 3, seed=9, n=1500)
        assert rc == 0 and ft.bow_get_created(info["bytes"]) == want and info["passes"] == want_info["passes"]
        rc, info = ft.bow_create_vocabulary(d.p.value + 4, docs[:-1] + [1499], 6, 3, seed=9, n=1499, check=False)
        assert rc == -1 and "aligned" in info["message"]
    finally:
        d.free()


# ---- the pick --------------------------------------------------------------------------------------------------------
def test_the_seeding_pick_at_its_boundaries(ft):
    rng = np.random.default_rng(4)
    edges = [0, 1, 63, 64, 255, 256, 257, 300, 300, 2047, 2048, 2049, 4096, 4100, 5000]
    md = rng.integers(0, 257, edges[-1]).astype(np.uint32)
    md[64:80] = 0      # a leading zero run of segment [64, 255)
    md[240:255] = 0    # ... and its trailing one
    md[2049:2100] = 0
    seg_off = np.array(edges, np.uint32)
    sums = [int(md[a:b].sum()) for a, b in zip(edges, edges[1:])]
    for kind in ("whole sum", "first non-zero", "below first non-zero", "on a running sum", "between", "beyond"):
        cut = []
        for (a, b), total in zip(zip(edges, edges[1:]), sums):
            seg = md[a:b].astype(np.int64)
            nz = seg[seg > 0]
            if kind == "whole sum" or not len(nz):
                cut.append(float(total))
            elif kind == "first non-zero":
                cut.append(float(nz[0]))
            elif kind == "below first non-zero":
                cut.append(float(nz[0]) - 0.5)
            elif kind == "on a running sum":
                cut.append(float(np.cumsum(seg)[len(seg) // 2]))
            elif kind == "between":
                cut.append(float(np.cumsum(seg)[len(seg) // 3]) + 0.25)
            else:
                cut.append(float(total) + 1.0)  # none reaches it: the last feature
        cut = np.array(cut)
        want = R.pick_ref(md, seg_off, cut)
        assert np.array_equal(ft.bow_create_pick(md, seg_off, cut), want), kind
    assert want[7] == 0xffffffff and want[0] == 0  # the empty segment, the segment of one


# ---- the guard -------------------------------------------------------------------------------------------------------
def test_max_passes_is_a_guard_and_a_failed_create_keeps_the_previous_image(ft):
    small = R.uniform(40, 1)
    rc, first = ft.bow_create_vocabulary(small, [0, 40], 3, 2, seed=1)
    kept = ft.bow_get_created(first["bytes"])
    desc = R.uniform(3000, 2)
    docs = R.even_docs(3000, 7)
    assert reference("uniform", desc, docs, 10, 2, seed=11)[1]["passes"] > 2
    with pytest.raises(R.NotSettled):
        R.create_numpy(desc, docs, 10, 2, seed=11, max_passes=2)
    rc, info = ft.bow_create_vocabulary(desc, docs, 10, 2, seed=11, max_passes=2, check=False)
    assert rc == -1 and "not settled" in info["message"] and info["bytes"] == 0 and info["nodes"] == 0
    assert ft.bow_get_created(first["bytes"]) == kept
    ft.reset()
    assert ft.bow_get_created(first["bytes"]) == kept


# ---- round trip ------------------------------------------------------------------------------------------------------
def test_created_words_are_the_restatements_walk(ft):
    desc = R.prototypes(2500, 30, 0.08, 12)
    docs = R.even_docs(2500, 20)
    got, _ = check(ft, "round trip", desc, docs, 6, 3, seed=4)
    if ft.bow_entries():
        ft.bow_clear()
    ft.bow_set_vocabulary(got)
    voc = B.Vocabulary(got)
    out = ft.bow_transform(desc)
    want = [voc.word(B.desc_int(r)) for r in desc]
    assert out["word"].tolist() == [w for w, _ in want]
    assert out["weight"].tobytes() == np.array([w for _, w in want], np.float64).tobytes()


def noise(shape, seed):
    """corners everywhere: the first kp_capacity in raster order are the keyframe's"""
    return np.random.default_rng(500 + seed).integers(0, 256, (shape[1], shape[0]), dtype=np.uint8)


def test_loop_detection_over_a_vocabulary_trained_on_the_librarys_own_descriptors():
    shape, cap, frames = (346, 260), 64, 56
    pattern = FE.load_brief_pattern(os.path.join(GOLDEN, "brief_pattern.yml"))
    window = np.zeros((0, 2), np.float32)
    t = FE.FeatureTracker(FE.make_config(shape[0], shape[1], device=0, max_cnt=40, min_dist=5))
    try:
        t.kf_set_pattern(*pattern)
        descs = []
        for f in range(frames):
            h = t.keyframe_describe(noise(shape, 2 if f == 55 else f), window, kp_capacity=cap)
            assert len(h["kp_desc"]) > 10
            descs.append(np.array(h["kp_desc"], np.uint32).reshape(-1, 8))
        train = np.concatenate(descs[:40])
        docs = np.concatenate([[0], np.cumsum([len(d) for d in descs[:40]])])
        want, _ = R.create_numpy(train, docs, 5, 3, seed=6)
        rc, info = t.bow_create_vocabulary(train, docs, 5, 3, seed=6)
        got = t.bow_get_created(info["bytes"])
        assert got == want
        t.bow_set_vocabulary(got)
        db = B.Database(B.Vocabulary(got))
        found = []
        for f in range(frames):
            m, res = t.detect_loop(descs[f], f)
            want_m, want_res = db.detect_loop([B.desc_int(w) for w in descs[f]], f)
            assert m == want_m and [r[0] for r in res] == [r[0] for r in want_res], f
            assert np.array([r[1] for r in res]).tobytes() == np.array([r[1] for r in want_res]).tobytes(), f
            found.append(m)
        assert res[0][0] == 2  # frame 55 is frame 2 again
    finally:
        t.close()


def test_make_vocabulary_turns_a_directory_of_descriptor_arrays_into_the_file(tmp_path, capsys):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_vocabulary", os.path.join(os.path.dirname(GOLDEN), "..", "tools", "make_vocabulary.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    desc = R.prototypes(400, 8, 0.08, 5)
    cuts = [0, 90, 90, 250, 400]  # the second keyframe has no descriptors
    for j, (a, b) in enumerate(zip(cuts, cuts[1:])):
        np.save(tmp_path / ("kf_%03d.npy" % j), desc[a:b])
    out = tmp_path / "voc.bin"
    assert tool.main([str(tmp_path), str(out), "--k", "4", "--L", "3", "--seed", "7"]) == 0
    want, want_info = R.create_numpy(desc, cuts, 4, 3, seed=7)
    assert out.read_bytes() == want
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (said["nodes"], said["words"], said["documents"], said["descriptors"]) == (want_info["nodes"], want_info["words"], 4, 400)


# ---- isolation -------------------------------------------------------------------------------------------------------
def test_a_create_between_track_calls_with_batches_announced_changes_no_later_result():
    from esvio_amd.events import event_times
    from esvio_amd.synth import SceneStream
    W, H = 346, 260
    s = SceneStream(W, H, rate=1e6, seed=3, n_rect=12, size=(30.0, 90.0))
    batches = [s.next_batch()[:2] for _ in range(5)]
    data = B.full_tree((4, 4), seed=3)
    voc = B.Vocabulary(data)
    qs = R.uniform(60, 77)
    train = R.prototypes(600, 8, 0.08, 2)
    results = ("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity", "ids_right", "cur_right_pts", "cur_un_right_pts",
               "right_pts_velocity")

    def run(create):
        t = FE.FeatureTracker(FE.make_config(W, H, device=0, max_cnt=60, min_dist=8, f_ransac=1))
        out = []
        try:
            t.bow_set_vocabulary(data)
            t.bow_add(qs[:30])
            before = t.bow_scores(qs)[0].tobytes()
            nxt = 1
            for k, (L, Rt) in enumerate(batches):
                while nxt < len(batches) and nxt <= k + 2:
                    t.set_next_batch(event_times(batches[nxt][0])[-1], batches[nxt][0], batches[nxt][1], True)
                    nxt += 1
                if create:
                    rc, info = t.bow_create_vocabulary(train, [0, 200, 600], 4, 3, seed=k)
                    assert rc == 0 and info["words"] > 4
                t.trackEvent(event_times(L)[-1], L, Rt, True)
                out.append({n: np.array(getattr(t, n)) for n in results})
            assert t.bow_entries() == 1 and t.bow_scores(qs)[0].tobytes() == before
            assert t.bow_transform(qs)["word"].tolist() == [voc.word(B.desc_int(r))[0] for r in qs]
        finally:
            t.close()
        return out
    plain, mixed = run(False), run(True)
    assert len(plain[-1]["ids"]) > 10
    for k, (a, b) in enumerate(zip(plain, mixed)):
        for n in results:
            assert np.array_equal(a[n], b[n]), (k, n)


# ---- the tables ------------------------------------------------------------------------------------------------------
def test_the_new_kernels_have_a_table_of_their_own(ft):
    L = FE.load_library()
    names = [L.esvio_fe_bow_create_kernel_name(j).decode() for j in range(L.esvio_fe_bow_create_kernel_count())]
    assert names == ["k_voc_first", "k_voc_mindist", "k_voc_scan_reduce", "k_voc_scan_top", "k_voc_scan_down", "k_voc_draw",
                     "k_voc_pick", "k_voc_assign", "k_voc_count_big", "k_voc_mean_big", "k_voc_mean_small", "k_voc_child_count",
                     "k_voc_regroup_keys", "k_voc_doc_count"]
    assert [L.esvio_fe_bow_kernel_name(j).decode() for j in range(L.esvio_fe_bow_kernel_count())] == ["k_bow_walk", "k_bow_vector", "k_bow_score", "k_bow_select"]
    assert (L.esvio_fe_kernel_count(), L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count(), L.esvio_fe_kf_kernel_count()) == (29, 48, 53, 3)
    ft.set_profiling(True)
    try:
        ft.reset_kernel_stats()
        before = ft.bow_create_kernel_stats()
        desc = R.prototypes(5000, 8, 0.08, 1)
        ft.bow_create_vocabulary(desc, R.even_docs(5000, 4), 4, 2, seed=1)
        after = ft.bow_create_kernel_stats()
        for name in names:
            assert after[name]["launches"] > before[name]["launches"], name
    finally:
        ft.set_profiling(False)
