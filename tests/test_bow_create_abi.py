"""CPU: the boundary of esvio_fe_bow_create_vocabulary that needs no device: the entry points are exported, listed and
declared, the structs are laid out as the C compiler lays them out, the group's kernel table names its kernels and every
other table is as it was, and rule C7's refusals come by name before a handle or a device is looked at."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("esvio_fe_bow_create_vocabulary", "esvio_fe_bow_get_created")
TAPS = ("esvio_fe_bow_create_kernel_count", "esvio_fe_bow_create_kernel_name", "esvio_fe_bow_create_kernel_stats", "esvio_fe_bow_create_pick")
STRUCTS = {"esvio_fe_bow_create_params": FE.BowCreateParams, "esvio_fe_bow_create_info": FE.BowCreateInfo}
KERNELS = ["k_voc_first", "k_voc_mindist", "k_voc_scan_reduce", "k_voc_scan_top", "k_voc_scan_down", "k_voc_draw", "k_voc_pick",
           "k_voc_assign", "k_voc_count_big", "k_voc_mean_big", "k_voc_mean_small", "k_voc_child_count", "k_voc_regroup_keys",
           "k_voc_doc_count"]


def test_entry_points_are_exported_listed_and_declared():
    L = FE.load_library()
    hdr = open(os.path.join(ROOT, "include", "esvio_fe.h")).read()
    tst = open(os.path.join(ROOT, "include", "esvio_fe_test.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(L, name) and name in FE.ABI_SYMBOLS and "int %s(" % name in hdr, name
    for name in TAPS:
        assert hasattr(L, name) and name in FE.TEST_SYMBOLS and "%s(" % name in tst, name
    assert "C, creating a vocabulary" in hdr


def test_the_structs_are_laid_out_as_the_c_compiler_lays_them_out(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "esvio_fe.h"', '#include "esvio_fe_test.h"', "int main(void) {"]
    want = []
    for name, cls in STRUCTS.items():
        members = [m for m, _ in cls._fields_]
        lines.append('  printf("%%zu ", sizeof(%s));' % name)
        lines += ['  printf("%%zu ", offsetof(%s, %s));' % (name, m) for m in members]
        want += [C.sizeof(cls)] + [getattr(cls, m).offset for m in members]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert C.sizeof(FE.BowCreateParams) == 32 and C.sizeof(FE.BowCreateInfo) == 232


def test_the_groups_table_and_the_tables_that_were_there():
    L = FE.load_library()
    assert [L.esvio_fe_bow_create_kernel_name(j).decode() for j in range(L.esvio_fe_bow_create_kernel_count())] == KERNELS
    assert L.esvio_fe_bow_create_kernel_name(-1) == b"" and L.esvio_fe_bow_create_kernel_name(len(KERNELS)) == b""
    assert (L.esvio_fe_kernel_count(), L.esvio_fe_stage_kernel_count(), L.esvio_fe_ingest_kernel_count(), L.esvio_fe_kf_kernel_count(),
            L.esvio_fe_bow_kernel_count()) == (29, 48, 53, 3, 4)
    assert [L.esvio_fe_bow_kernel_name(j).decode() for j in range(4)] == ["k_bow_walk", "k_bow_vector", "k_bow_score", "k_bow_select"]
    assert L.esvio_fe_bow_create_kernel_stats(None, 0, None, None, None) == -1
    assert L.esvio_fe_bow_get_created(None, None, 0) == -1
    assert L.esvio_fe_bow_create_pick(None, None, 1, None, 1, None, None) == -1


def refuse(n=10, k=3, L=2, weighting=0, scoring=0, max_passes=0, docs=(0, 4, 10), space=None, desc=True, off=True, params=True):
    """the call without a handle: C7's checks come first -> (return code, message)"""
    lib = FE.load_library()
    d = np.zeros((max(int(min(n, 16)), 1), 8), np.uint32)
    o = np.array(docs, np.int64)
    par = FE.BowCreateParams(k, L, weighting, scoring, max_passes, 0, 1)
    info = FE.BowCreateInfo()
    rc = lib.esvio_fe_bow_create_vocabulary(None, FE._p(d) if desc else None, n, FE.HOST if space is None else space,
                                            FE._p(o) if off else None, len(o) - 1, C.byref(par) if params else None, C.byref(info))
    assert (info.nodes, info.words, info.bytes) == (0, 0, 0)
    return rc, info.message.decode()


@pytest.mark.parametrize("kw, code, word", [
    (dict(n=0, docs=(0, 0)), -1, "n must be"), (dict(n=(1 << 24) + 1, docs=(0, (1 << 24) + 1)), -1, "n must be"),
    (dict(k=1), -1, "k must be"), (dict(k=33), -1, "k must be"), (dict(L=0), -1, "L must be"), (dict(L=11), -1, "L must be"),
    (dict(weighting=-1), -1, "weighting"), (dict(weighting=4), -1, "weighting"), (dict(scoring=1), -4, "scoring"),
    (dict(max_passes=-1), -1, "max_passes"), (dict(docs=(1, 4, 10)), -1, "doc_offsets[0]"), (dict(docs=(0, 5, 4, 10)), -1, "lies below"),
    (dict(docs=(0, 4, 9)), -1, "doc_offsets[n_docs]"), (dict(docs=(0, 4, 11)), -1, "doc_offsets[n_docs]"), (dict(docs=(0,)), -1, "n_docs"),
    (dict(space=7), -1, "memory space"), (dict(desc=False), -1, "null"), (dict(off=False), -1, "null"), (dict(params=False), -1, "params"),
])
def test_c7_is_refused_by_name_before_a_handle_or_a_device(kw, code, word):
    rc, msg = refuse(**kw)
    assert rc == code and word in msg, (rc, msg)


def test_good_arguments_reach_the_handle_check_and_a_misaligned_device_pointer_does_not():
    assert refuse() == (-1, "the handle is null")
    assert refuse(docs=(0, 0, 10, 10)) == (-1, "the handle is null")  # empty documents are allowed
    lib = FE.load_library()
    o, par, info = np.array((0, 10), np.int64), FE.BowCreateParams(3, 2, 0, 0, 0, 0, 1), FE.BowCreateInfo()
    rc = lib.esvio_fe_bow_create_vocabulary(None, C.c_void_p(0x1004), 10, FE.DEVICE, FE._p(o), 1, C.byref(par), C.byref(info))
    assert rc == -1 and "16-byte aligned" in info.message.decode()
    assert lib.esvio_fe_bow_create_vocabulary(None, C.c_void_p(0x1000), 10, FE.DEVICE, FE._p(o), 1, C.byref(par), None) == -1
