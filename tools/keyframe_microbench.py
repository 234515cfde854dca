"""esvio_fe_kf_* micro-benchmark: the loop-closure keyframe's image passes at 346x260 (DAVIS) and 1440x1080 (DSEC) on a
seeded blocky scene with noise, 150 window points (MAX_CNT) and the corners cv::FAST's rule finds at threshold 20.
Per shape: every kernel of esvio_fe_kf_describe per launch from the LIBRARY'S OWN TIMERS (esvio_fe_kf_kernel_stats and
esvio_fe_get_kernel_stats: HIP events around the launch) — k_kf_blur also as a share of the measured device copy rate at
its 2 bytes per pixel —; the wall time of esvio_fe_kf_describe from device and from pageable host memory, descriptors
left on the device; esvio_fe_kf_match at 150 x 2000 from device and from host memory.  Beside them the bridge the calls
replace: tools/keyframe_seq.cpp, the same rules as scalar loops on one core (NOT OpenCV's vectorised code, which nobody
has measured here), plus esvio_fe_mem_upload of the frame.  Per figure: the median of BLOCKS blocks of REPS after a
warm-up block, and the blocks' min - max.  One process, one pass, no retries; run it under a time limit:

    g++ -O2 -std=c++17 tools/keyframe_seq.cpp -o tools/_bin/keyframe_seq
    timeout -k 10 600 python tools/keyframe_microbench.py > profiles/keyframe_microbench.txt
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from esvio_amd import frontend as FE  # noqa: E402

HBM_GBS = 6290.0  # measured float4 copy rate of an MI355X (KERNELS.md)
BLOCKS, REPS = 5, 20
SHAPES = (("DAVIS", 346, 260), ("DSEC", 1440, 1080))
N_WINDOW, NQ, NT = 150, 150, 2000
SEQ = os.path.join(ROOT, "tools", "_bin", "keyframe_seq")
PATTERN = os.path.join(ROOT, "tests", "golden", "brief_pattern.yml")


def med(v):
    v = sorted(v)
    return (v[len(v) // 2], v[0], v[-1])


def scene(W, H, seed):
    rng = np.random.default_rng(seed)
    cell = 24
    g = rng.integers(30, 226, ((H + cell - 1) // cell, (W + cell - 1) // cell)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.uint8))[:H, :W] // 2 + rng.integers(0, 24, (H, W), dtype=np.uint8))


def timed(fn):
    out = []
    for _ in range(BLOCKS + 1):
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        out.append((time.perf_counter() - t0) / REPS * 1e6)
    return med(out[1:])


def alloc(L, nbytes, data=None):
    p = C.c_void_p()
    assert L.esvio_fe_mem_alloc(FE.DEVICE, max(int(nbytes), 16), C.byref(p)) == 0
    if data is not None:
        assert L.esvio_fe_mem_upload(p, FE._p(data), data.nbytes) == 0
    return p


def main():
    L = FE.load_library()
    hip = C.CDLL("libamdhip64.so")
    pattern = FE.load_brief_pattern(PATTERN)
    rng = np.random.default_rng(1)
    T = rng.integers(0, 2 ** 32, (NT, 8), dtype=np.uint64).astype(np.uint32)
    Q = T[rng.integers(0, NT, NQ)] ^ rng.integers(0, 2 ** 32, (NQ, 8), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101)
    print("keyframe stage: %d window points, cv::FAST's rule at threshold 20, match %d x %d; medians of %d blocks of %d (min - max)" % (N_WINDOW, NQ, NT, BLOCKS, REPS))
    for tag, W, H in SHAPES:
        img = scene(W, H, 5)
        window = np.stack([rng.uniform(10, W - 10, N_WINDOW), rng.uniform(10, H - 10, N_WINDOW)], 1).astype(np.float32)
        ft = FE.FeatureTracker(FE.make_config(W, H, max_cnt=150, min_dist=10))
        ft.kf_set_pattern(*pattern)
        first = ft.keyframe_describe(img, window)
        n_kp = first["n_kp"]
        print("%s %dx%d: %d corners kept of %d detected, %d window points" % (tag, W, H, n_kp, first["n_detected"], N_WINDOW))
        d_img, d_wd, d_kd = alloc(L, img.nbytes, img), alloc(L, N_WINDOW * 32), alloc(L, max(n_kp, 1) * 32)
        o = FE.KfOut()
        kxy, ksc, knorm = np.zeros((n_kp, 2), np.float32), np.zeros(n_kp, np.int32), np.zeros((n_kp, 2), np.float32)
        o.window_desc, o.kp_desc, o.desc_space, o.kp_capacity = d_wd.value, d_kd.value, FE.DEVICE, n_kp
        o.kp_xy, o.kp_score, o.kp_norm = kxy.ctypes.data, ksc.ctypes.data, knorm.ctypes.data

        def describe_dev():
            assert L.esvio_fe_kf_describe(ft._hd.h, 0, d_img, FE.DEVICE, FE._p(window), N_WINDOW, 20, C.byref(o)) == 0

        def describe_host():
            assert L.esvio_fe_kf_describe(ft._hd.h, 0, FE._p(img), FE.HOST, FE._p(window), N_WINDOW, 20, C.byref(o)) == 0

        for _ in range(REPS):
            describe_dev()
        back = np.zeros((n_kp, 8), np.uint32)
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), d_kd, C.c_size_t(back.nbytes), 2) == 0
        assert o.n_kp == n_kp and np.array_equal(back, first["kp_desc"]) and np.array_equal(kxy, first["kp_xy"])
        # per kernel, by the library's timers
        per = {}
        for _ in range(BLOCKS):
            ft.set_profiling(True)
            ft.reset_kernel_stats()
            for _ in range(REPS):
                describe_dev()
            st = dict(ft.kf_kernel_stats(), **{k: v for k, v in ft.kernel_stats().items() if k in ("k_fast_score", "k_fast_collect", "k_compact")})
            ft.set_profiling(False)
            for k, v in st.items():
                if v["launches"]:
                    per.setdefault(k, []).append((v["ms"] / v["launches"] * 1e3, v["launches"] // REPS))
        for k in ("k_kf_blur", "k_fast_score", "k_fast_collect", "k_compact", "k_kf_brief"):
            us, n = med([p[0] for p in per[k]]), per[k][0][1]
            extra = ""
            if k == "k_kf_blur":
                extra = "; %d bytes at 2 per pixel = %.0f GB/s, %.1f %% of the %.0f GB/s copy rate" % (2 * W * H, 2 * W * H / us[0] / 1e3, 100 * 2 * W * H / us[0] / 1e3 / HBM_GBS, HBM_GBS)
            print("    %-14s %7.2f us per launch (%.2f - %.2f), %d per call%s" % ((k,) + us + (n, extra)))
        dv, hs = timed(describe_dev), timed(describe_host)
        print("    esvio_fe_kf_describe, image in device memory, descriptors left on the device: %.1f us (%.1f - %.1f)" % dv)
        print("    esvio_fe_kf_describe, image in pageable host memory:                        %.1f us (%.1f - %.1f)" % hs)
        # the bridge: the scalar loops on one core, then the frame's upload
        with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
            f.write(np.array([W, H, N_WINDOW, NQ, NT, 3], np.int32).tobytes() + img.tobytes() + window.tobytes())
            f.write(np.concatenate(pattern).astype(np.int32).tobytes() + Q.tobytes() + T.tobytes())
        try:
            seq = subprocess.check_output([SEQ, f.name]).decode().split()
        finally:
            os.unlink(f.name)
        seq = dict(zip(seq[::2], seq[1::2]))
        want_xor = int(np.bitwise_xor.reduce(np.concatenate([first["window_desc"].ravel(), first["kp_desc"].ravel()])))
        assert int(seq["n_kp"]) == n_kp and int(seq["desc_xor"], 16) == want_xor, (seq, n_kp, hex(want_xor))
        up = timed(lambda: L.esvio_fe_mem_upload(d_img, FE._p(img), img.nbytes))
        print("    one core (tools/keyframe_seq.cpp: blur + corners + %d descriptors, scalar): %.0f us; esvio_fe_mem_upload of the frame %.1f us (%.1f - %.1f)"
              % ((N_WINDOW + n_kp, float(seq["describe_us"])) + up))
        if tag == "DAVIS":
            dq, dt = alloc(L, Q.nbytes, Q), alloc(L, T.nbytes, T)
            idx, dist, st = np.zeros(NQ, np.int32), np.zeros(NQ, np.int32), np.zeros(NQ, np.uint8)

            def match_dev():
                assert L.esvio_fe_kf_match(ft._hd.h, dq, NQ, dt, NT, FE.DEVICE, FE._p(idx), FE._p(dist), FE._p(st)) == 0

            def match_host():
                assert L.esvio_fe_kf_match(ft._hd.h, FE._p(Q), NQ, FE._p(T), NT, FE.HOST, FE._p(idx), FE._p(dist), FE._p(st)) == 0

            match_dev()
            assert int(idx.sum() + dist.sum() + st.sum()) == int(seq["match_sum"])
            mk = []
            for _ in range(BLOCKS + 1):
                ft.set_profiling(True)
                ft.reset_kernel_stats()
                for _ in range(REPS):
                    match_dev()
                v = ft.kf_kernel_stats()["k_kf_match"]
                ft.set_profiling(False)
                mk.append(v["ms"] / v["launches"] * 1e3)
            print("match %d x %d:" % (NQ, NT))
            print("    k_kf_match     %7.2f us per launch (%.2f - %.2f)" % med(mk[1:]))
            print("    esvio_fe_kf_match, descriptors in device memory: %.1f us (%.1f - %.1f); in host memory: %.1f us (%.1f - %.1f)" % (timed(match_dev) + timed(match_host)))
            print("    one core (tools/keyframe_seq.cpp, popcount loop): %.0f us" % float(seq["match_us"]))
            L.esvio_fe_mem_free(FE.DEVICE, dq), L.esvio_fe_mem_free(FE.DEVICE, dt)
        for p in (d_img, d_wd, d_kd):
            L.esvio_fe_mem_free(FE.DEVICE, p)
        ft.close()


if __name__ == "__main__":
    main()
