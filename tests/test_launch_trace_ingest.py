"""The launch trace of tests/test_launch_trace.py for the ingest entry points, which neither its matrix nor
test_launch_trace_cand.py's reaches.  tests/hipstub/drive.cpp `trace_ingest` walks, on one thread at 346 x 260:
esvio_fe_decode_raw (EVT2 / EVT3 / EVT2.1 x pageable / registered / device source x host / device dst; the argument
refusals; bad stamps, no room and the repeated emit, a plain success behind each) and esvio_fe_decode_triggers;
esvio_fe_track_raw (both cameras, one camera, a filter, motion, bad stamps on the right camera only, the repeated emit,
no left event, a filter body that fails, a batch announced); esvio_fe_decode_aedat and esvio_fe_track_aedat over the same
cells (ESVIO_FE_AEDAT_KEEP_INVALID off and on, a malformed header, a chunk that completes no polarity record);
esvio_fe_decode_bag; esvio_fe_feed_push_raw / _aedat / _bag / _events on a feed without and with a filter — on the
filtered one the bag push whose right camera fails behind the left camera's append, which is undone —; and
esvio_fe_decode_reset, esvio_fe_reset and esvio_fe_reserve on each of these handles.

The stub launchers do nothing, so the fake device (tests/hipstub/fake_device.cpp) has the emit launchers of the raw,
trigger, AEDAT and bag chains write a result block the driver sets beforehand — that is how refusals and the repeated
emit are walked — and has them and the raw reduce write what they were handed into the trace: the carried decoder
state as the seed, the chunk, the room.  A decoder state that moved when it should not have, or did not when it should
have, shows in the next call's lines.  Behind every call the trace holds its return code, the error text of a failed call
and every field of the info struct, so messages and info contents are pinned byte for byte.  A sixth override,
launch_baf_emit, reports every record kept and a last stamp unless the driver sets its error (hipstub_set_baf: the filter
body that fails under esvio_fe_track_raw / _aedat; hipstub_set_baf_err_at: only the right camera's chain of a bag push);
the older traces' matrices and the ThreadSanitizer driver run no filter and are as they were.

What the trace does NOT pin: the stub runtime writes no hipMalloc lines, so allocation sizes show only as the dst_cap a
launch is handed — min(scratch capacity, room) for raw words, the room itself for AEDAT and bags, whose growth of the
decode scratch behind a host dst is therefore unpinned — and the stub slicer closes no window, so the feed's window
queue and slicer state show only as `queued 0` and in the length the left camera's buffer is moved with.

tests/golden/launch_trace_ingest.txt was recorded from the library as it was BEFORE the decode step, the placements and
the decode-and-track tail were given one place each (KERNELS.md, "ingest host code"): only tests/hipstub/drive.cpp,
fake_device.cpp, gen_kernel_stubs.py's OVERRIDES and this file differed from that commit when it was recorded.  A
host-side refactoring reproduces it byte for byte.  A change that is meant to launch something else records the file
anew (the command is in the assertion message) and says so."""
import os
import subprocess

from test_host_tsan import ROOT, build_driver

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace_ingest.txt")

REFUSALS = (
    "decode_raw: dst is null", "decode_raw: a device dst must be 16-byte aligned", "decode_raw: bad memory space",
    "the camera's decoder state is as it was", "the camera's trigger-decoder state is as it was",
    "decode_raw: the chunk holds 3000 events, dst has room for 2999", "decode_triggers: the chunk holds 9 triggers, dst has room for 8",
    "both cameras' decoder states are as they were", "both cameras' states are as they were",
    "track_raw: batches are announced on this handle", "track_aedat: batches are announced on this handle",
    "track_raw: radix sort look-back spin expired", "track_aedat: radix sort look-back spin expired",
    "decode_aedat: the chunk holds 10 events, dst has room for 9; the camera's state is as it was",
    "decode_aedat: 1 of 10 events have a stamp outside [0, 2^32 s); the camera's state is as it was",
    "decode_aedat: malformed packet header", "track_aedat (right): malformed packet header",
    "decode_bag: 2 of 11 events have nsec >= 10^9; the walker's state is as it was",
    "decode_bag: the chunk holds 6 left and 5 right events, dst has room for 4000 and 4; the walker's state is as it was",
    "decode_bag: the chunk completes 2 event messages, msgs has room for 1; the walker's state is as it was",
    "decode_bag: malformed bag", "decode_bag: a device dst must be 16-byte aligned", "decode_bag: dst[1] is null",
    "feed_push_raw: 4 of 500 events have a stamp outside [0, 2^32 s); nothing was appended, the camera's decoder state is as it was",
    "feed_push_aedat: 1 of 10 events have a stamp outside [0, 2^32 s); nothing was appended, the camera's state is as it was",
    "feed_push_bag: 1 of 11 events have nsec >= 10^9; nothing was appended, the walker's state is as it was",
    "feed_push_bag: the origin is the first left record", "feed_push_raw: the origin is the first left record",
    "feed_push_bag: radix sort look-back spin expired",
)


def test_ingest_paths_launch_sequence_return_codes_messages_and_infos_are_the_recorded_ones(tmp_path):
    exe = build_driver(tmp_path, name="drive_trace_ingest", sanitize=None)
    out = str(tmp_path / "trace_ingest.txt")
    p = subprocess.run([exe, "trace_ingest"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIPSTUB_TRACE=out))
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    got, want = open(out).read().splitlines(), open(GOLDEN).read().splitlines()
    assert got[-1] == "live: device 0 pinned 0 events 0 streams 0", got[-1]
    section = call = ""
    for i, (g, w) in enumerate(zip(got, want)):
        section = w if w.startswith("== ") else section
        call = w if w.startswith("-- ") else call
        assert g == w, "line %d, handle '%s', call '%s': got '%s', recorded '%s' (HIPSTUB_TRACE=%s %s trace_ingest)" % (
            i + 1, section[3:], call[3:], g, w, os.path.relpath(GOLDEN, ROOT), os.path.basename(exe))
    assert len(got) == len(want), "%d lines, recorded %d" % (len(got), len(want))
    assert open(out, "rb").read() == open(GOLDEN, "rb").read()
    # the paths are really walked: every kernel of the raw, trigger, AEDAT and bag ranges was booked by some handle ...
    for kernel in ("k_raw_reduce", "k_raw_scan", "k_raw_emit", "k_trig_reduce", "k_trig_emit", "k_aedat_count", "k_aedat_scan",
                   "k_aedat_emit", "k_bag_emit"):
        assert any(l.startswith("profile %s launches " % kernel) and not l.startswith("profile %s launches 0 " % kernel)
                   for l in want), kernel
    # ... the emit launch was repeated in each of the four raw consumers, and every refusal occurs
    text = "\n".join(want)
    for again in ("launch_raw_emit 1\n  launch_raw_emit[0]", "launch_trig_emit 1\n  launch_trig_emit[0]"):
        assert text.count("hipMemsetAsync 1 8\nhipEventRecord 1\n" + again) >= 1, again
    assert text.count("hipMemsetAsync 1 8\nhipEventRecord 1\nlaunch_raw_emit 1") >= 5
    for refusal in REFUSALS:
        assert any(l.startswith("   rc -") and refusal in l for l in want), refusal
