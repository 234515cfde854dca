"""The launch trace of tests/test_launch_trace.py for the paths its matrix never reaches: everything that leaves
per-block candidate lists and has them compacted.  tests/hipstub/drive.cpp `trace_cand` walks, on one thread at
346 x 260: esvio_fe_fast_corners on the handle's time surface and on a host image (arc 9 and 10, non-max on and off);
a handle after esvio_fe_set_detector(ESVIO_FE_DETECT_FAST) through a plain call, an announced batch,
esvio_fe_features_to_track_fast, esvio_fe_reset and a call after it; two handles whose Arc* pass runs k_dedup
(max_cnt 600, ESVIO_FE_DEDUP=1); esvio_fe_good_features_to_track without and with a mask.

tests/golden/launch_trace_cand.txt was recorded from the library as it was BEFORE the FAST list pass and the
compaction of a candidate set were given one place each (KERNELS.md, "candidate lists"): a host-side refactoring
reproduces it byte for byte.  A change that is meant to launch something else records the file anew (the command is
in the assertion message) and says so."""
import os
import subprocess

from test_host_tsan import ROOT, build_driver

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace_cand.txt")


def test_candidate_paths_launch_sequence_streams_and_byte_accounting_are_the_recorded_ones(tmp_path):
    exe = build_driver(tmp_path, name="drive_trace_cand", sanitize=None)
    out = str(tmp_path / "trace_cand.txt")
    p = subprocess.run([exe, "trace_cand"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIPSTUB_TRACE=out))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    got, want = open(out).read().splitlines(), open(GOLDEN).read().splitlines()
    assert got[-1] == "live: device 0 pinned 0 events 0 streams 0", got[-1]
    section = call = ""
    for i, (g, w) in enumerate(zip(got, want)):
        section = w if w.startswith("== ") else section
        call = w if w.startswith("-- ") else call
        assert g == w, "line %d, handle '%s', call '%s': got '%s', recorded '%s' (HIPSTUB_TRACE=%s %s trace_cand)" % (
            i + 1, section[3:], call[3:], g, w, os.path.relpath(GOLDEN, ROOT), os.path.basename(exe))
    assert len(got) == len(want), "%d lines, recorded %d" % (len(got), len(want))
    assert open(out, "rb").read() == open(GOLDEN, "rb").read()
    # the paths are really walked: every kernel this file is about was booked by some handle
    for kernel in ("k_fast_score", "k_fast_collect", "k_dedup", "k_compact", "k_arc_ev"):
        assert any(l.startswith("profile %s launches " % kernel) and not l.startswith("profile %s launches 0 " % kernel)
                   for l in want), kernel
    for launcher in ("launch_gftt_collect", "launch_fast_keys", "launch_dedup"):
        assert any(l.startswith(launcher + " ") for l in want), launcher
