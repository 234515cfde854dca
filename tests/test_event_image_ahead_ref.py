"""CPU: the designed sequences of tests/event_image_ahead_cases.py tell their frames apart — under the plain loop of
tests/event_image_ref.py the images of any two batches within four of each other differ, in both cameras and on the
canvas, and one batch has no right events — and the boundary of mode 2 that needs no device: the header's constant, the
entry point's signature, the value the Python mirror passes."""
import os
import subprocess
import types

import numpy as np

import event_image_ahead_cases as A
import event_image_ref as R
from esvio_amd import frontend as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sequence_is_eight_or_more_stereo_batches_each_in_rows_its_neighbours_avoid():
    seq = A.sequence()
    assert len(seq) >= 8 and len(A.PUB) == len(seq) and 0 < sum(A.PUB) < len(seq)
    rows = []
    for k, (L, Rt, t) in enumerate(seq):
        assert 100 <= len(L) <= 5000 and (len(Rt) == 0) == (k == A.NO_RIGHT)
        assert t > (L["sec"][-1] + L["nsec"][-1] * 1e-9)
        rows.append((set(L["y"].tolist()), set(Rt["y"].tolist())))
        assert len(rows[-1][0]) == A.BAND_ROWS  # the band is covered: every row of it has an event
    for i in range(len(seq)):
        for j in range(i + 1, min(i + 5, len(seq))):
            assert not rows[i][0] & rows[j][0] and not rows[i][1] & rows[j][1], (i, j)
    # more than one event per pixel of the cameras that have events in some batches, fewer in others: both forms of
    # the mark kernel
    dens = [(len(L) + len(Rt)) / (A.W * A.H * (2 if len(Rt) else 1)) for L, Rt, _ in seq]
    assert min(dens) < 1 < max(dens) and sum(d > 1 for d in dens) >= 2


def test_reference_images_of_batches_within_four_of_each_other_differ():
    ref = A.reference()
    for i in range(len(ref)):
        for j in range(i + 1, min(i + 5, len(ref))):
            for part, name in enumerate(("left", "right", "canvas")):
                assert not np.array_equal(ref[i][part], ref[j][part]), (i, j, name)
    # the batch without right events: a zero right image, the left half of its canvas is its left image
    a, b, c = ref[A.NO_RIGHT]
    assert a.any() and not b.any() and np.array_equal(c[:, :A.W], a) and not c[:, A.W:].any()
    # ... and a second sequence (the one tracked after esvio_fe_reset) differs from the first frame by frame
    other = A.reference(seed=1)
    assert all(not np.array_equal(x[0], y[0]) for x, y in zip(ref, other))


def test_an_image_is_rewritten_whole_nothing_of_an_earlier_batch_stays():
    seq, ref = A.sequence(), A.reference()
    for k in range(1, len(seq)):
        stale = R.event_image(seq[k][0], A.W, A.H, base=ref[k - 1][0])  # what accumulating would give
        assert not np.array_equal(stale, ref[k][0]), k


SIGNATURES = """
#include "esvio_fe.h"
int (*p_set)(esvio_fe_handle, int) = esvio_fe_set_event_images;
int (*p_next)(esvio_fe_handle, double, const esvio_fe_event*, size_t, const esvio_fe_event*, size_t, int, int) = esvio_fe_set_next_batch;
#if ESVIO_FE_EVENT_IMAGES_AHEAD != 2
#error "ESVIO_FE_EVENT_IMAGES_AHEAD must be 2"
#endif
"""


def test_the_header_has_the_mode_and_the_mirror_passes_it_through(tmp_path):
    src = tmp_path / "sig.c"
    src.write_text(SIGNATURES)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "sig.o")])
    hdr = open(os.path.join(ROOT, "include", "esvio_fe.h")).read()
    assert hdr.count("#define ESVIO_FE_EVENT_IMAGES_AHEAD 2") == 1
    assert "62 bytes per pixel" in hdr  # the header states what the mode costs
    assert FE.EVENT_IMAGES_AHEAD == 2
    # the value that reaches the library: 2 for 2, 1 / 0 for anything else by its truth
    seen = []
    fake = types.SimpleNamespace(_hd=types.SimpleNamespace(
        h=None, check=lambda rc: None, L=types.SimpleNamespace(esvio_fe_set_event_images=lambda h, on: seen.append(on) or 0)))
    for on in (2, True, False, 1, 0, FE.EVENT_IMAGES_AHEAD):
        FE.FeatureTracker.set_event_images(fake, on)
    assert seen == [2, 1, 0, 1, 0, 2] and all(type(x) is int for x in seen)
    assert FE.load_library().esvio_fe_set_event_images(None, 2) == -1  # a null handle is refused before the device
