"""esvio_fe_filter_events micro-benchmark: per-launch times of the filter's chain (esvio_fe_get_kernel_stats: k_sae_keys,
k_radix_pass x passes, k_baf_heads, k_baf_filter, k_baf_count, k_baf_scan, k_baf_emit) and the whole call's wall time,
at C3's batch (640 x 480, ~167 k events) and C5's (1280 x 720, ~3.3 M), on the scene stream and on the uniform stream,
from device memory into device memory, with the bytes each launch is booked with.  Beside it, measured in the same
run on the same events: the SAE update chain (k_tile_hist, k_tile_scan, k_tile_scatter, k_tile_apply) of
esvio_fe_create_sae, the existing event-proportional pass of a batch.  The filter runs with the reference driver's
20 ms window and support 1, every call on fresh planes (esvio_fe_filter_reset between the calls, not timed).  Per
figure: the median of BLOCKS blocks of REPS calls after a warm-up block, and the blocks' min - max.  One process, one
pass, no retries; run it under a time limit:

    timeout -k 10 600 python tools/filter_microbench.py [--json out.json]

--fields runs another pass instead: the same events as separate arrays in device memory (x[], y[] uint16, t[] uint32
microseconds behind an offset, p[] uint8: event_fields_ref's soa_u32_us) through esvio_fe_filter_batch on the fields,
against the two-call form it replaces — esvio_fe_convert_events into device memory, then esvio_fe_filter_events —
block after block in turn, in one process, the library's kernel timers off: call wall times, the median of BLOCKS
blocks of REPS calls after a warm-up block, min - max.  Behind the timed blocks, with the timers on, the per-launch
times of the fields form's chain.

    timeout -k 10 600 python tools/filter_microbench.py --fields [--json out.json]

--address: the address stage (esvio_fe_set_address_filter).  esvio_fe_filter_batch on records and on the separate
arrays above, device memory into device memory, call wall times, block after block in turn in one process: without a
stage, with a stage that rejects nothing (the whole sensor as ROI, use_mask with an empty mask) and with the stream's
eight most active pixels learned, installed and masked — and, with --other LIB, the same calls without a stage through
another build of the library (the parent commit's, say) in the same turn.  Behind the timed blocks, with the timers on,
the per-launch times of the chain with the stage that rejects nothing.

--hot: esvio_fe_hot_learn's k_hot_count per launch beside k_sae_keys (the filter's keys kernel, which reads the same 16
bytes per event) on the same events: the scene stream, the uniform stream, and the uniform stream with 1 % of its
events on eight pixels (and one with every other event on one pixel); records and fields.  With --other LIB the same launch of another build beside it (a build
without the in-wave combining, say).

    timeout -k 10 600 python tools/filter_microbench.py --address [--other LIB] [--only C3] [--json out.json]
    timeout -k 10 600 python tools/filter_microbench.py --hot [--other LIB] [--only C3] [--json out.json]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402
from esvio_amd.synth import SceneStream, uniform_batch  # noqa: E402

BLOCKS, REPS = 5, 10
WINDOW_NS, MIN_SUPPORT = 20_000_000, 1
SIZES = (("C3", 640, 480, 167_000), ("C5", 1280, 720, 3_300_000))
FILTER_CHAIN = ("k_sae_keys", "k_radix_pass", "k_baf_heads", "k_baf_filter", "k_baf_count", "k_baf_scan", "k_baf_emit")
SAE_CHAIN = ("k_tile_hist", "k_tile_scan", "k_tile_scatter", "k_tile_apply")
FIELDS_CHAIN = ("k_baf_keys_fields", "k_radix_pass", "k_baf_heads", "k_baf_filter", "k_baf_count", "k_baf_scan", "k_baf_emit_fields")
TWO_CALL_CHAIN = ("k_events_from_fields",) + FILTER_CHAIN


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def streams(w, h, n):
    """~n left events of one 1/30 s batch: the bench scene (7 % uniform noise) and uniform noise alone"""
    scene = SceneStream(W=w, H=h, rate=n * 30.0, seed=11).next_batch()[0]
    uni = uniform_batch(w, h, n, 1_000_000_000, 33_333, np.random.default_rng(12))
    return (("scene", scene), ("uniform", uni))


def measure(tr, call, chain, between=None):
    """-> {kernel: (us per call: median, min, max), launches per call, booked bytes per call}, call wall us"""
    for _ in range(REPS):
        if between:
            between()
        call()
    per, wall = {k: [] for k in chain}, []
    info = {}
    for _ in range(BLOCKS):
        tr.set_profiling(True)
        tr.reset_kernel_stats()
        t = 0.0
        for _ in range(REPS):
            if between:
                between()
            t0 = time.perf_counter()
            call()
            t += time.perf_counter() - t0
        wall.append(t / REPS * 1e6)
        st = tr.kernel_stats(stages=True)
        tr.set_profiling(False)
        for k in chain:
            per[k].append(st[k]["ms"] / REPS * 1e3)
            info[k] = (st[k]["launches"] / REPS, st[k]["alg_bytes"] / REPS)
    return {k: (med(per[k]),) + info[k] for k in chain}, med(wall), [sum(per[k][b] for k in chain) for b in range(BLOCKS)]


def device_fields(L, ev):
    """the events as separate arrays in one block of device memory -> (EventFields of device pointers, the block)"""
    from esvio_amd.events import EventFields
    t_us = ev["sec"].astype(np.int64) * 1_000_000 + ev["nsec"].astype(np.int64) // 1000
    base = int(t_us.min())
    arrs = (ev["x"].astype(np.uint16), ev["y"].astype(np.uint16), (t_us - base).astype(np.uint32), ev["polarity"].astype(np.uint8))
    offs, o = [], 0
    for a in arrs:
        offs.append(o)
        o = (o + a.nbytes + 15) & ~15
    raw = np.zeros(o, np.uint8)
    for a, off in zip(arrs, offs):
        raw[off:off + a.nbytes] = a.view(np.uint8)
    blk = C.c_void_p()
    assert L.esvio_fe_mem_alloc(FE.DEVICE, o, C.byref(blk)) == 0
    assert L.esvio_fe_mem_upload(blk, C.c_void_p(raw.ctypes.data), o) == 0
    f = EventFields.at_pointers([blk.value + off for off in offs], (2, 2, 4, 1), len(ev), 32, 8, 1000, base)
    return f, blk


def timed_blocks(calls, between):
    """calls: {name: callable}, run block after block in turn -> {name: wall us per call (median, min, max)}"""
    wall = {k: [] for k in calls}
    for b in range(BLOCKS + 1):  # (block 0: the warm-up)
        for k, call in calls.items():
            t = 0.0
            for _ in range(REPS):
                between()
                t0 = time.perf_counter()
                call()
                t += time.perf_counter() - t0
            if b:
                wall[k].append(t / REPS * 1e6)
    return {k: med(v) for k, v in wall.items()}


def main_fields():
    L = FE.load_library()
    rows = []
    for tag, w, h, n_target in SIZES:
        tr = FE.FeatureTracker(FE.make_config(w, h))
        for name, ev in streams(w, h, n_target):
            n = len(ev)
            fields, blk = device_fields(L, ev)
            desc = FE.fields_desc(fields)
            prm = FE.FilterParams(WINDOW_NS, MIN_SUPPORT, 0)
            rec, dst = C.c_void_p(), C.c_void_p()
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(rec)) == 0 and L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(dst)) == 0
            nk, rej, bad, nk2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

            def one_call():
                assert L.esvio_fe_filter_batch(tr._hd.h, 0, None, C.byref(desc), n, FE.DEVICE, C.byref(prm), dst, FE.DEVICE,
                                               C.byref(nk), None, None, C.byref(rej), C.byref(bad)) == 0

            def two_calls():
                assert L.esvio_fe_convert_events(tr._hd.h, C.byref(desc), n, FE.DEVICE, rec, FE.DEVICE, C.byref(bad)) == 0
                assert L.esvio_fe_filter_events(tr._hd.h, 0, rec, n, FE.DEVICE, WINDOW_NS, MIN_SUPPORT, dst, FE.DEVICE,
                                                C.byref(nk2), None, None, C.byref(rej)) == 0

            wall = timed_blocks({"fields": one_call, "two-call": two_calls}, tr.filter_reset)
            assert nk.value == nk2.value
            fk, _, fsum = measure(tr, one_call, FIELDS_CHAIN, between=tr.filter_reset)
            tk, _, tsum = measure(tr, two_calls, TWO_CALL_CHAIN, between=tr.filter_reset)
            print("%s %dx%d %-8s n %8d, kept %.3f, rejected %d" % (tag, w, h, name, n, nk.value / n, rej.value))
            for k in ("fields", "two-call"):
                print("  %-9s call %9.1f us (%.1f - %.1f) = %7.1f Mev/s" % ((k,) + wall[k] + (n / wall[k][0],)))
            print("  fields / two-call = %.3f; the two-call form's own spread: %.1f us" %
                  (wall["fields"][0] / wall["two-call"][0], wall["two-call"][2] - wall["two-call"][1]))
            for title, ks, tot in (("fields form", fk, fsum), ("two-call form", tk, tsum)):
                for k, (us, launches, nbytes) in ks.items():
                    print("    %-20s %9.1f us (%.1f - %.1f)  %4.1f launches  %7.1f B/event booked" % (k, us[0], us[1], us[2], launches, nbytes / n))
                t = med(tot)
                print("  %-13s launches %9.1f us (%.1f - %.1f), timers on" % (title, t[0], t[1], t[2]))
            rows.append(dict(batch=tag, width=w, height=h, stream=name, n=n, kept=int(nk.value), rejected=int(rej.value),
                             window_ns=WINDOW_NS, min_support=MIN_SUPPORT, fields_call_us=wall["fields"], two_call_us=wall["two-call"],
                             fields={k: dict(us=v[0], launches=v[1], booked_bytes=v[2]) for k, v in fk.items()},
                             two_call={k: dict(us=v[0], launches=v[1], booked_bytes=v[2]) for k, v in tk.items()},
                             fields_launches_us=med(fsum), two_call_launches_us=med(tsum)))
            for p in (blk, rec, dst):
                L.esvio_fe_mem_free(FE.DEVICE, p)
        tr.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


def main():
    L = FE.load_library()
    rows = []
    for tag, w, h, n_target in SIZES:
        tr = FE.FeatureTracker(FE.make_config(w, h))
        for name, ev in streams(w, h, n_target):
            n = len(ev)
            src = FE.EventBuffer(ev, FE.DEVICE)
            dst = C.c_void_p()
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(dst)) == 0
            nk, rej = C.c_uint64(0), C.c_uint64(0)

            def filt():
                assert L.esvio_fe_filter_events(tr._hd.h, 0, C.c_void_p(src.arg[0]), n, FE.DEVICE, WINDOW_NS, MIN_SUPPORT, dst,
                                                FE.DEVICE, C.byref(nk), None, None, C.byref(rej)) == 0

            def sae():
                tr.detector.createSAE_left(src.arg)

            fk, fwall, fsum = measure(tr, filt, FILTER_CHAIN, between=tr.filter_reset)
            sk, swall, ssum = measure(tr, sae, SAE_CHAIN)
            print("%s %dx%d %-8s n %8d, kept %.3f, rejected %d" % (tag, w, h, name, n, nk.value / n, rej.value))
            for title, ks, wall, tot in (("filter", fk, fwall, fsum), ("SAE update", sk, swall, ssum)):
                for k, (us, launches, nbytes) in ks.items():
                    print("    %-16s %9.1f us (%.1f - %.1f)  %4.1f launches  %7.1f B/event booked = %6.0f GB/s"
                          % (k, us[0], us[1], us[2], launches, nbytes / n, nbytes / max(us[0], 1e-9) / 1e3))
                t = med(tot)
                print("  %-10s chain %9.1f us (%.1f - %.1f) = %7.1f Mev/s | call %9.1f us (%.1f - %.1f) = %7.1f Mev/s"
                      % (title, t[0], t[1], t[2], n / t[0], wall[0], wall[1], wall[2], n / wall[0]))
            f, s = med(fsum)[0], med(ssum)[0]
            print("  filter chain / SAE chain = %.2f" % (f / s))
            rows.append(dict(batch=tag, width=w, height=h, stream=name, n=n, kept=int(nk.value), rejected=int(rej.value),
                             window_ns=WINDOW_NS, min_support=MIN_SUPPORT,
                             filter={k: dict(us=v[0], launches=v[1], booked_bytes=v[2]) for k, v in fk.items()},
                             sae={k: dict(us=v[0], launches=v[1], booked_bytes=v[2]) for k, v in sk.items()},
                             filter_chain_us=med(fsum), sae_chain_us=med(ssum), filter_call_us=fwall, sae_call_us=swall,
                             ratio=f / s))
            src.free()
            L.esvio_fe_mem_free(FE.DEVICE, dst)
        tr.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


def other_tracker(path, cfg):
    """a handle of another build of the library in this process (its entry points called with this build's
    argument types; what it lacks is not called)"""
    cur = FE.load_library()
    other = C.CDLL(path)
    for name in FE.ABI_SYMBOLS + FE.TEST_SYMBOLS:
        fn = getattr(other, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = getattr(cur, name).argtypes, getattr(cur, name).restype
    FE._lib = other
    try:
        return FE.FeatureTracker(cfg)
    finally:
        FE._lib = cur


def sizes():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    return [s for s in SIZES if only in (None, s[0])]


def turns(calls):
    """calls: {name: (callable, what runs untimed in front of every call)}, block after block in turn ->
    {name: wall us per call (median, min, max)}"""
    wall = {k: [] for k in calls}
    for b in range(BLOCKS + 1):  # (block 0: the warm-up)
        for k, (call, between) in calls.items():
            t = 0.0
            for _ in range(REPS):
                between()
                t0 = time.perf_counter()
                call()
                t += time.perf_counter() - t0
            if b:
                wall[k].append(t / REPS * 1e6)
    return {k: med(v) for k, v in wall.items()}


def batch_caller(tr, n, dst, prm, ev=None, desc=None):
    L, nk, rej, bad = tr._hd.L, C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call():
        assert L.esvio_fe_filter_batch(tr._hd.h, 0, ev, C.byref(desc) if desc is not None else None, n, FE.DEVICE, C.byref(prm), dst,
                                       FE.DEVICE, C.byref(nk), None, None, C.byref(rej), C.byref(bad)) == 0
    return call, nk, rej


def main_address():
    L = FE.load_library()
    other_path = sys.argv[sys.argv.index("--other") + 1] if "--other" in sys.argv else None
    rows = []
    for tag, w, h, n_target in sizes():
        cfg = FE.make_config(w, h)
        tr = {"no stage": FE.FeatureTracker(cfg), "stage, rejects nothing": FE.FeatureTracker(cfg), "stage, 8 pixels masked": FE.FeatureTracker(cfg)}
        if other_path:
            tr = dict([("other build, no stage", other_tracker(other_path, cfg))] + list(tr.items()))
        full = FE.AddressFilter((0, 0, w - 1, h - 1), use_mask=1)
        tr["stage, rejects nothing"].set_pixel_mask(0, [])
        tr["stage, rejects nothing"].set_address_filter(0, full)
        tr["stage, 8 pixels masked"].set_address_filter(0, full)
        for name, ev in streams(w, h, n_target):
            n = len(ev)
            src = FE.EventBuffer(ev, FE.DEVICE)
            fields, blk = device_fields(L, ev)
            desc = FE.fields_desc(fields)
            dst = C.c_void_p()
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(dst)) == 0
            prm = FE.FilterParams(WINDOW_NS, MIN_SUPPORT, 0)
            hot = tr["stage, 8 pixels masked"]
            hot.hot_reset()
            hot.hot_learn(0, src.arg)
            xy, cnt, info = hot.hot_select(0, FE.HotParams(max_pixels=8, min_count=1, install=True))
            print("%s %dx%d %-8s n %8d; the 8 most active pixels hold %s" % (tag, w, h, name, n, cnt.tolist()))
            row = dict(batch=tag, width=w, height=h, stream=name, n=n, masked_counts=cnt.tolist())
            for form, kw in (("records", dict(ev=C.c_void_p(src.arg[0]))), ("fields", dict(desc=desc))):
                calls, outs = {}, {}
                for k, t in tr.items():
                    call, nk, rej = batch_caller(t, n, dst, prm, **kw)
                    calls[k], outs[k] = (call, t.filter_reset), (nk, rej)
                wall = turns(calls)
                base = wall.get("other build, no stage", wall["no stage"])
                for k in calls:
                    print("  %-7s %-24s call %9.1f us (%.1f - %.1f)  %.3f of the first row, whose own spread is %.1f us; kept %d, rejected %d"
                          % ((form, k) + wall[k] + (wall[k][0] / base[0], base[2] - base[1], outs[k][0].value, outs[k][1].value)))
                assert outs["no stage"][0].value == outs["stage, rejects nothing"][0].value
                chain = ("k_baf_keys_addr",) + FILTER_CHAIN[1:] if form == "records" else FIELDS_CHAIN
                per, _, tot = measure(tr["stage, rejects nothing"], calls["stage, rejects nothing"][0], chain, between=tr["stage, rejects nothing"].filter_reset)
                ref_chain = FILTER_CHAIN if form == "records" else FIELDS_CHAIN
                per0, _, tot0 = measure(tr["no stage"], calls["no stage"][0], ref_chain, between=tr["no stage"].filter_reset)
                for (k, (us, launches, nbytes)), (k0, (us0, _, _)) in zip(per.items(), per0.items()):
                    print("    %-18s %9.1f us (%.1f - %.1f) | no stage: %-18s %9.1f us (%.1f - %.1f)" % ((k,) + us + (k0,) + us0))
                row[form] = dict(call_us=wall, stage_launch_us={k: v[0] for k, v in per.items()}, no_stage_launch_us={k: v[0] for k, v in per0.items()})
            rows.append(row)
            src.free()
            for p in (blk, dst):
                L.esvio_fe_mem_free(FE.DEVICE, p)
        for t in tr.values():
            t.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


def main_hot():
    L = FE.load_library()
    other_path = sys.argv[sys.argv.index("--other") + 1] if "--other" in sys.argv else None
    rows = []
    for tag, w, h, n_target in sizes():
        cfg = FE.make_config(w, h)
        tr = {"this build": FE.FeatureTracker(cfg)}
        if other_path:
            tr["other build"] = other_tracker(other_path, cfg)
        sts = list(streams(w, h, n_target))
        piled = sts[1][1].copy()
        rng = np.random.default_rng(13)
        idx = rng.choice(len(piled), len(piled) // 100, replace=False)
        piled["x"][idx] = 17 + 40 * rng.integers(0, 8, len(idx))
        piled["y"][idx] = 23
        sts.append(("1% on 8", piled))
        pile = sts[1][1].copy()  # (beyond the three streams above: every other event on ONE pixel, a pile the combining is for)
        pile["x"][::2], pile["y"][::2] = 20, 20
        sts.append(("50% on 1", pile))
        for name, ev in sts:
            n = len(ev)
            src = FE.EventBuffer(ev, FE.DEVICE)
            fields, blk = device_fields(L, ev)
            dst = C.c_void_p()
            assert L.esvio_fe_mem_alloc(FE.DEVICE, 16 * n, C.byref(dst)) == 0
            print("%s %dx%d %-8s n %8d" % (tag, w, h, name, n))
            row = dict(batch=tag, width=w, height=h, stream=name, n=n)
            for k, t in tr.items():
                call, nk, rej = batch_caller(t, n, dst, FE.FilterParams(WINDOW_NS, MIN_SUPPORT, 0), ev=C.c_void_p(src.arg[0]))
                keys = measure(t, call, ("k_sae_keys",), between=t.filter_reset)[0]["k_sae_keys"][0]
                rec = measure(t, lambda: t.hot_learn(0, src.arg), ("k_hot_count",), between=t.hot_reset)[0]["k_hot_count"][0]
                fld = measure(t, lambda: t.hot_learn(0, fields, src_space=FE.DEVICE), ("k_hot_count",), between=t.hot_reset)[0]["k_hot_count"][0]
                print("  %-11s k_sae_keys %8.1f us (%.1f - %.1f) | k_hot_count records %8.1f us (%.1f - %.1f) = %6.0f Mev/s | fields %8.1f us (%.1f - %.1f)"
                      % ((k,) + keys + rec + (n / rec[0],) + fld))
                row[k] = dict(k_sae_keys_us=keys, k_hot_count_records_us=rec, k_hot_count_fields_us=fld)
            rows.append(row)
            src.free()
            for p in (blk, dst):
                L.esvio_fe_mem_free(FE.DEVICE, p)
        for t in tr.values():
            t.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fo:
            json.dump(rows, fo, indent=1)


if __name__ == "__main__":
    if "--address" in sys.argv:
        main_address()
    elif "--hot" in sys.argv:
        main_hot()
    else:
        main_fields() if "--fields" in sys.argv else main()
