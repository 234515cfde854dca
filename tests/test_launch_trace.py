"""What the host side launches, in which order and on which stream, pinned without a GPU.  tests/hipstub/drive.cpp
`trace` walks a fixed matrix on one thread — event handles at 346 x 260 (default, equalize, median, ESVIO_FE_NO_FUSE
with and without equalize, ESVIO_FE_SAE_SORT, ESVIO_FE_NO_CAMSPLIT), one whose pyramid has fewer than three levels,
one at 1920 x 1080 (the selection bitmap in device memory), each through plain calls from device and host memory,
announced batches, an imported right image, the time-surface and featuresToTrack entry points; two image handles
through trackImage and goodFeaturesToTrack — and the stub runtime (HIPSTUB_TRACE) writes one line per launcher,
hipEventRecord, hipStreamWaitEvent, hipMemsetAsync and hipMemcpyAsync with its stream's ordinal, then per handle the
launches and bytes the profiling API counted for every kernel id.

tests/golden/launch_trace.txt was recorded from the library as it was BEFORE the image build, the radix sort and the
selection launch were given one place each (KERNELS.md): a host-side refactoring reproduces it byte for byte.  A change
that is meant to launch something else records the file anew (the command is in the assertion message) and says so."""
import os
import subprocess

from test_host_tsan import ROOT, build_driver

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.txt")


def test_launch_sequence_streams_and_byte_accounting_are_the_recorded_ones(tmp_path):
    exe = build_driver(tmp_path, name="drive_trace", sanitize=None)
    out = str(tmp_path / "trace.txt")
    p = subprocess.run([exe, "trace"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIPSTUB_TRACE=out))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    got, want = open(out).read().splitlines(), open(GOLDEN).read().splitlines()
    assert got[-1] == "live: device 0 pinned 0 events 0 streams 0", got[-1]
    section = call = ""
    for i, (g, w) in enumerate(zip(got, want)):
        section = w if w.startswith("== ") else section
        call = w if w.startswith("-- ") else call
        assert g == w, "line %d, handle '%s', call '%s': got '%s', recorded '%s' (HIPSTUB_TRACE=%s %s trace)" % (
            i + 1, section[3:], call[3:], g, w, os.path.relpath(GOLDEN, ROOT), os.path.basename(exe))
    assert len(got) == len(want), "%d lines, recorded %d" % (len(got), len(want))
