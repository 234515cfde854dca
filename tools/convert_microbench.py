"""esvio_fe_convert_events micro-benchmark: per-launch time of k_events_from_fields (esvio_fe_get_kernel_stats) and
the whole call's wall time, for the layouts of tests/event_fields_ref.py at C3's batch (~167 k events per camera) and
C5's (3.3 M), from device memory, from page-locked memory read in place, from page-locked memory copied first
(ESVIO_FE_CONVERT_PINNED_COPY=1) and from pageable memory, into device memory; with the bytes read + written and
the share of the HBM rate (device sources) or of the PCIe rate (host sources: the bytes that cross the link) they
amount to.  Beside it the path without the call: esvio_amd.events.make_events on one core + esvio_fe_mem_upload of
the records, timed on the same box.  Per figure: the median of BLOCKS blocks of REPS launches after a warm-up block,
and the blocks' min - max.  One process, one pass, no retries; run it under a time limit:

    timeout -k 10 600 python tools/convert_microbench.py [--json out.json]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import event_fields_ref as R  # noqa: E402
from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.events import EventFields, make_events  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (8 TB/s spec)
PCIE_GBS = 52.0   # what k_stage_pull reaches from pinned memory on this stack (tools/h2d_probe.hip)
BLOCKS, REPS = 5, 20
SIZES = (("C3", 167_000), ("C5", 3_300_000))


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    L = FE.load_library()
    os.environ["ESVIO_FE_CONVERT_PINNED_COPY"] = "0"  # (unset: the library picks per layout and size)
    ft = FE.FeatureTracker(FE.make_config(640, 480))
    os.environ["ESVIO_FE_CONVERT_PINNED_COPY"] = "1"
    ft_copy = FE.FeatureTracker(FE.make_config(640, 480))
    del os.environ["ESVIO_FE_CONVERT_PINNED_COPY"]
    nmax = max(n for _, n in SIZES)
    arena = R.raw_bytes("", nmax)
    pin, dsrc, ddst = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.esvio_fe_mem_alloc(FE.HOST, arena, C.byref(pin)) == 0
    assert L.esvio_fe_mem_alloc(FE.DEVICE, arena, C.byref(dsrc)) == 0
    assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * nmax, C.byref(ddst)) == 0
    pinned = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), shape=(arena,))
    rows = []
    for tag, n in SIZES:
        for layout in R.LAYOUTS:
            case = R.make_case(layout, n, seed=5)
            f = case.fields
            nb = len(case.raw)
            pinned[:nb] = case.raw
            assert L.esvio_fe_mem_upload(dsrc, C.c_void_p(case.raw.ctypes.data), nb) == 0
            dev_fields = EventFields.at_pointers([dsrc.value + (p - case.raw.ctypes.data) for p in f.ptrs], f.strides, n,
                                                 f.t_bits, f.p_bits, f.t_unit_ns, f.t_offset)
            src_bytes = sum(sorted(s for _, s in f.spans())[-1:]) if layout.startswith(("aos", "packed")) else sum(s for _, s in f.spans())
            moved = src_bytes + 16 * n
            print("%s %-16s n %8d: %.1f B/event read, 16 written" % (tag, layout, n, src_bytes / n))
            for src, tr, fields, space in (("device", ft, dev_fields, FE.DEVICE), ("pinned, in place", ft, case.relocate(pinned[:nb]), FE.HOST),
                                           ("pinned, copy first", ft_copy, case.relocate(pinned[:nb]), FE.HOST),
                                           ("pageable", ft, f, FE.HOST)):
                desc, bad = FE.fields_desc(fields), C.c_uint64(0)

                def call():
                    assert L.esvio_fe_convert_events(tr._hd.h, C.byref(desc), n, space, ddst, FE.DEVICE, C.byref(bad)) == 0

                reps = REPS if n < 1_000_000 or src == "device" else 5
                for _ in range(reps):
                    call()  # warm-up block (and the first call's allocations)
                k_us, call_us = [], []
                for _ in range(BLOCKS):
                    tr.set_profiling(True)
                    tr.reset_kernel_stats()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        call()
                    call_us.append((time.perf_counter() - t0) / reps * 1e6)
                    st = tr.kernel_stats()["k_events_from_fields"]
                    tr.set_profiling(False)
                    assert st["launches"] == reps
                    k_us.append(st["ms"] / reps * 1e3)
                k, c = med(k_us), med(call_us)
                link = src_bytes if space == FE.HOST else 0
                gbs = moved / (k[0] * 1e-6) / 1e9
                row = dict(batch=tag, n=n, layout=layout, source=src, kernel_us=k, call_us=c, bytes=moved, kernel_gbs=gbs,
                           hbm_frac=gbs / HBM_GBS, mev_s_call=n / c[0])
                line = "    %-18s kernel %8.1f us (%.1f - %.1f) = %6.0f GB/s" % (src, k[0], k[1], k[2], gbs)
                if space == FE.DEVICE:
                    line += " = %4.1f %% of HBM" % (100 * gbs / HBM_GBS)
                else:
                    lg = link / (c[0] * 1e-6) / 1e9
                    row.update(link_bytes=link, link_gbs_call=lg, pcie_frac_call=lg / PCIE_GBS)
                    line += "; link %5.1f GB/s of the call = %4.1f %% of PCIe" % (lg, 100 * lg / PCIE_GBS)
                print(line + " | call %8.1f us (%.1f - %.1f) = %7.1f Mev/s" % (c[0], c[1], c[2], n / c[0]))
                rows.append(row)
            if layout == "soa_u32_us":  # the path without the call, for the same arrays: numpy on one core + upload of the records
                t_us = case.t.astype(np.int64) + case.t_offset
                mk, up = [], []
                for _ in range(BLOCKS):
                    t0 = time.perf_counter()
                    ev = make_events(case.x, case.y, t_us, case.p)
                    t1 = time.perf_counter()
                    assert L.esvio_fe_mem_upload(ddst, C.c_void_p(ev.ctypes.data), ev.nbytes) == 0
                    up.append((time.perf_counter() - t1) * 1e6)
                    mk.append((t1 - t0) * 1e6)
                m, u = med(mk), med(up)
                print("    make_events on one core %.0f us (%.0f - %.0f) + esvio_fe_mem_upload %.0f us (%.0f - %.0f) = %.1f Mev/s"
                      % (m[0], m[1], m[2], u[0], u[1], u[2], n / (m[0] + u[0])))
                rows.append(dict(batch=tag, n=n, layout=layout, source="make_events + esvio_fe_mem_upload", make_events_us=m,
                                 upload_us=u, mev_s_call=n / (m[0] + u[0])))
    L.esvio_fe_mem_free(FE.HOST, pin)
    L.esvio_fe_mem_free(FE.DEVICE, dsrc)
    L.esvio_fe_mem_free(FE.DEVICE, ddst)
    ft.close()
    ft_copy.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    main()
