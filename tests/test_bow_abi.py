"""CPU: the boundary of loop detection (esvio_fe_bow_*) that needs no device: the library exports the entry points and
the lists name them, a null handle is refused before anything else, the structs are laid out by the C compiler as their
ctypes mirrors say, the kernel tables that tests and recorded launch traces pin return what they returned, the group's
own table lists its four kernels, and esvio_fe_bow_vocabulary_header accepts the synthetic files and refuses every item
of rule V's list by name."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bow_ref as B
from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("esvio_fe_bow_vocabulary_header", "esvio_fe_bow_set_vocabulary", "esvio_fe_bow_transform", "esvio_fe_bow_add",
                "esvio_fe_bow_query", "esvio_fe_bow_detect_loop", "esvio_fe_bow_clear", "esvio_fe_bow_entries", "esvio_fe_bow_reserve")
TAPS = ("esvio_fe_bow_kernel_count", "esvio_fe_bow_kernel_name", "esvio_fe_bow_kernel_stats", "esvio_fe_bow_limits", "esvio_fe_bow_scores")
STRUCTS = {"esvio_fe_bow_vocabulary_info": (FE.BowVocabularyInfo, "esvio_fe.h"), "esvio_fe_bow_result": (FE.BowResult, "esvio_fe.h"),
           "esvio_fe_bow_limits_info": (FE.BowLimits, "esvio_fe_test.h")}
# the tables as they stood before the group existed
TRACK_KERNELS, STAGE_KERNELS, INGEST_KERNELS, KF_KERNELS = 29, 48, 53, 3


def test_entry_points_are_exported_and_listed():
    L = FE.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS, name
    for name in TAPS:
        assert hasattr(L, name) and name in FE.TEST_SYMBOLS, name
    hdr = open(os.path.join(ROOT, "include", "esvio_fe.h")).read()
    tst = open(os.path.join(ROOT, "include", "esvio_fe_test.h")).read()
    assert all("int %s(" % n in hdr for n in ENTRY_POINTS) and all("%s(" % n in tst for n in TAPS)
    for text, value in (("#define ESVIO_FE_BOW_MAX_RESULTS 64", FE.BOW_MAX_RESULTS), ("#define ESVIO_FE_BOW_LOOP_RESULTS 4", FE.BOW_LOOP_RESULTS),
                        ("#define ESVIO_FE_BOW_LOOP_GAP 50", FE.BOW_LOOP_GAP), ("#define ESVIO_FE_BOW_LOOP_MIN_FIRST 0.05", FE.BOW_LOOP_MIN_FIRST),
                        ("#define ESVIO_FE_BOW_LOOP_MIN_OTHER 0.015", FE.BOW_LOOP_MIN_OTHER)):
        assert text in hdr and float(text.split()[-1]) == value
    assert (B.LOOP_RESULTS, B.LOOP_GAP, B.LOOP_MIN_FIRST, B.LOOP_MIN_OTHER) == (4, 50, 0.05, 0.015)


def test_a_null_handle_is_refused_before_the_device():
    L = FE.load_library()
    w, n, res = np.zeros(8, np.uint32), C.c_int32(7), (FE.BowResult * 4)()
    p = FE._p
    assert L.esvio_fe_bow_set_vocabulary(None, b"x", 1) == -1
    assert L.esvio_fe_bow_transform(None, p(w), 1, FE.HOST, None, None, None, None, 0, C.byref(n)) == -1
    assert L.esvio_fe_bow_add(None, p(w), 1, FE.HOST, None) == -1
    assert L.esvio_fe_bow_query(None, p(w), 1, FE.HOST, 4, -1, res, C.byref(n)) == -1
    assert L.esvio_fe_bow_detect_loop(None, p(w), 1, FE.HOST, 3, C.byref(n), None, None) == -1
    assert L.esvio_fe_bow_clear(None) == -1 and L.esvio_fe_bow_entries(None) == -1 and L.esvio_fe_bow_reserve(None, 1, 1) == -1
    assert L.esvio_fe_bow_kernel_stats(None, 0, None, None, None) == -1
    assert L.esvio_fe_bow_scores(None, p(w), 1, FE.HOST, -1, None, None) == -1
    assert L.esvio_fe_bow_limits(None) == -1 and L.esvio_fe_bow_vocabulary_header(b"x", 1, None) == -1


def test_the_structs_are_laid_out_as_the_c_compiler_lays_them_out(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', '#include "esvio_fe_test.h"', "int main(void) {"]
    want = []
    for name, (cls, _) in STRUCTS.items():
        members = [m for m, _ in cls._fields_]
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        want += [C.sizeof(cls)] + [getattr(cls, m).offset for m in members]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert (C.sizeof(FE.BowVocabularyInfo), C.sizeof(FE.BowResult), C.sizeof(FE.BowLimits)) == (224, 16, 16)


def test_the_existing_kernel_tables_are_as_they_were():
    L = FE.load_library()
    assert (L.esvio_fe_kernel_count(), L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count(), L.esvio_fe_kf_kernel_count()) == \
        (TRACK_KERNELS, STAGE_KERNELS, INGEST_KERNELS, KF_KERNELS)
    names = [L.esvio_fe_kernel_name(k).decode() for k in range(INGEST_KERNELS)]
    assert len(set(names)) == INGEST_KERNELS and not any(n.startswith("k_bow_") for n in names)
    for k in range(INGEST_KERNELS, INGEST_KERNELS + 12):
        assert L.esvio_fe_kernel_name(k) == b""
    assert [L.esvio_fe_kf_kernel_name(k) for k in range(-1, 5)] == [b"", b"k_kf_blur", b"k_kf_brief", b"k_kf_match", b"", b""]


def test_the_group_has_a_table_of_its_own_and_limits():
    L = FE.load_library()
    assert L.esvio_fe_bow_kernel_count() == 4
    assert [L.esvio_fe_bow_kernel_name(k) for k in range(-1, 5)] == [b"", b"k_bow_walk", b"k_bow_vector", b"k_bow_score", b"k_bow_select", b""]
    lim = FE.bow_limits()
    assert lim["group_lanes"] in (8, 16, 32, 64) and lim["lds_words"] >= 64 and lim["vector_block"] >= 64 and lim["max_results"] == 64


# ---- rule V: esvio_fe_bow_vocabulary_header ---------------------------------------------------------------------------
def small_tree():
    """root -> 1, 2, 3; 1 -> 4, 5; 3 -> 6 -> 7 (leaves 2, 4, 5, 7 at depths 1, 2, 2, 3; node 3 and 6 have one child)"""
    t = B.TreeBuilder(3)
    a, b, c = t.add(0), t.add(0), t.add(0)
    t.add(a), t.add(a)
    t.add(t.add(c))
    return t


def test_the_header_call_accepts_the_synthetic_files():
    rc, info = FE.bow_vocabulary_header(small_tree().finish(k=3, L=3, weighting=B.IDF))
    assert rc == 0 and info == dict(k=3, L=3, scoring=0, weighting=2, nodes=7, words=4, leaves=4, max_children=3, depth=3, message="")
    rc, info = FE.bow_vocabulary_header(small_tree().finish(k=3, L=3, shuffle=True))
    assert rc == 0 and (info["nodes"], info["leaves"], info["depth"]) == (7, 4, 3)
    rc, info = FE.bow_vocabulary_header(B.full_tree((10, 10, 10), seed=1))
    assert rc == 0 and info == dict(k=10, L=3, scoring=0, weighting=0, nodes=1110, words=1000, leaves=1000, max_children=10, depth=3, message="")
    t = B.TreeBuilder(4)
    t.full([17])
    rc, info = FE.bow_vocabulary_header(t.finish(k=17, L=1, weighting=B.BINARY))
    assert rc == 0 and (info["max_children"], info["depth"], info["weighting"]) == (17, 1, 3)


def records():
    """the small tree's records, to be spoilt one at a time"""
    hdr, nodes = B.parse(small_tree().finish(k=3, L=3))
    recs = [(i, nodes[i]["parent"], nodes[i]["weight"], nodes[i]["desc"]) for i in range(1, 8)]
    words = [(i, nodes[i]["word"]) for i in (2, 4, 5, 7)]
    return recs, words


def spoilt(node=None, word=None, **hdr):
    recs, words = records()
    if node:
        recs[node[0]] = node[1](recs[node[0]])
    if word:
        words[word[0]] = word[1](words[word[0]])
    h = dict(k=3, L=3, scoring=0, weighting=0)
    h.update(hdr)
    return B.serialise(h["k"], h["L"], h["scoring"], h["weighting"], recs, words)


def set_counts(data, nodes=None, words=None):
    b = bytearray(data)
    if nodes is not None:
        struct.pack_into("<i", b, 16, nodes)
    if words is not None:
        struct.pack_into("<i", b, 20, words)
    return bytes(b)


REFUSALS = {
    "a byte too many": (lambda: spoilt() + b"\0", "byte count"),
    "a byte too few": (lambda: spoilt()[:-1], "byte count"),
    "half a header": (lambda: spoilt()[:12], "byte count"),
    "one node fewer than the bytes hold": (lambda: set_counts(spoilt(), nodes=6), "byte count"),
    "a negative word count": (lambda: set_counts(spoilt(), words=-6), "byte count"),
    "nNodes 0": (lambda: set_counts(spoilt()[:24 + 32], nodes=0), "nNodes"),
    "nNodes -1": (lambda: set_counts(spoilt(), nodes=-1), "nNodes"),
    "nodeId 0": (lambda: spoilt(node=(3, lambda r: (0,) + r[1:])), "nodeId"),
    "nodeId nNodes + 1": (lambda: spoilt(node=(3, lambda r: (8,) + r[1:])), "nodeId"),
    "nodeId duplicated": (lambda: spoilt(node=(3, lambda r: (2,) + r[1:])), "duplicated"),
    "parentId -1": (lambda: spoilt(node=(3, lambda r: (r[0], -1) + r[2:])), "parentId"),
    "parentId nNodes + 1": (lambda: spoilt(node=(3, lambda r: (r[0], 8) + r[2:])), "parentId"),
    "parentId its own node": (lambda: spoilt(node=(3, lambda r: (r[0], r[0]) + r[2:])), "parentId"),
    "two nodes that are each other's parents": (lambda: B.serialise(2, 2, 0, 0, [(1, 0, 1.0, 0), (2, 3, 1.0, 0), (3, 2, 1.0, 0)], [(1, 0)]), "not reachable"),
    "a root without children": (lambda: B.serialise(2, 2, 0, 0, [(1, 2, 1.0, 0), (2, 1, 1.0, 0)], []), "root"),
    "wordId -1": (lambda: spoilt(word=(1, lambda w: (w[0], -1))), "wordId"),
    "wordId nWords": (lambda: spoilt(word=(1, lambda w: (w[0], 4))), "wordId"),
    "wordId duplicated": (lambda: spoilt(word=(1, lambda w: (w[0], 0))), "duplicated"),
    "a word on a node that has children": (lambda: spoilt(word=(1, lambda w: (1, w[1]))), "has children"),
    "a word on node 0": (lambda: spoilt(word=(1, lambda w: (0, w[1]))), "nodeId"),
    "a word on node nNodes + 1": (lambda: spoilt(word=(1, lambda w: (8, w[1]))), "nodeId"),
    "a leaf without a word": (lambda: spoilt(word=(1, lambda w: (2, w[1]))), "leaf"),
    "weighting 4": (lambda: spoilt(weighting=4), "weighting"),
    "weighting -1": (lambda: spoilt(weighting=-1), "weighting"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_the_header_call_refuses_by_name(name):
    make, keyword = REFUSALS[name]
    rc, info = FE.bow_vocabulary_header(make())
    assert rc == -1 and keyword in info["message"], (name, rc, info["message"])


def test_other_scorings_are_not_built_and_a_null_image_is_refused():
    for scoring in (1, 2, 5, -1):
        rc, info = FE.bow_vocabulary_header(spoilt(scoring=scoring))
        assert rc == -4 and "scoring" in info["message"], (scoring, info)
    info = FE.BowVocabularyInfo()
    assert FE.load_library().esvio_fe_bow_vocabulary_header(None, 100, C.byref(info)) == -1 and b"null" in info.message
    assert FE.bow_vocabulary_header(spoilt())[0] == 0
