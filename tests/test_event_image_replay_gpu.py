"""GPU: tools/replay_node show=1 against the Python node with show_track=True on the same log: every tracked frame's
canvas — published or not — has the same FNV-1a 64 hash, and a dump without show=1 is byte for byte what it was."""
import os
import subprocess

import numpy as np
import pytest

import event_image_ref as R
import test_replay_node_gpu as T
from esvio_amd import frontend as FE
from esvio_amd.node import StereoEventTrackerNode
from esvio_amd.synth import SceneStream

pytestmark = pytest.mark.gpu


def fnv1a64(b):
    h = 14695981039346656037
    for x in bytes(b):
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def messages():
    """seven stereo batches, a 1.5 s hole after the fourth (a restart: a frame that is not tracked)"""
    s = SceneStream(T.W, T.H, rate=3e5, seed=23, n_rect=12, size=(30.0, 90.0))
    msgs = []
    for b in range(7):
        if b == 4:
            s.t_us += 1_500_000
        L, Rt, t_end = s.next_batch()
        msgs += [(0, t_end * 1e-6, L), (1, t_end * 1e-6 + 0.001, Rt)]
    return msgs


def test_replay_node_show_hashes_equal_the_python_nodes(tmp_path):
    assert fnv1a64(b"") == 0xcbf29ce484222325 and fnv1a64(b"a") == 0xaf63dc4c8601ec8c  # the published test vectors
    msgs = messages()
    log = str(tmp_path / "log.esvb")
    T._write_log(log, msgs)
    from esvio_amd import build as B
    tool, dumps = B.build_tools(), {}
    for name, opts in (("plain", []), ("show", ["show=1"])):
        dump = str(tmp_path / (name + ".bin"))
        p = subprocess.run([tool, log, dump, "max_cnt=%d" % T.KW["max_cnt"], "min_dist=%d" % T.KW["min_dist"], "freq=%d" % T.FREQ,
                            "lk_accum=%d" % FE.DEFAULT_LK_ACCUM] + opts, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        dumps[name] = open(dump, "rb").read()
    assert dumps["show"].startswith(dumps["plain"])  # the frames are what they were; the lines follow them
    frames = T._read_dump(str(tmp_path / "show.bin"))
    lines = dumps["show"][len(dumps["plain"]):].decode().splitlines()
    got = [(int(l.split()[1]), int(l.split()[2], 16)) for l in lines]
    assert all(l.split()[0] == "show" and len(l.split()[2]) == 16 for l in lines)
    # the Python node over the same pairs (every left message has its partner 1 ms behind it)
    ft = FE.FeatureTracker(FE.make_config(T.W, T.H, device=0, **T.KW))
    try:
        node = StereoEventTrackerNode(ft, T.FREQ, show_track=True)
        want, k, unpublished = [], 0, 0
        for (_, stamp, L), (_, _, Rt) in zip(msgs[0::2], msgs[1::2]):
            out = node.handle(L, Rt, stamp)
            if out is not None:
                assert set(out) == {"points", "feature_img_base", "time_surface"}  # the plain overload: no event_loop
                assert np.array_equal(out["feature_img_base"], R.canvas(R.event_image(L, T.W, T.H), R.event_image(Rt, T.W, T.H)))
                assert np.array_equal(out["time_surface"], ft.gettimesurface(0))
                unpublished += out["points"] is None
                want.append((k, fnv1a64(out["feature_img_base"].tobytes())))
                k += 1
            elif node.restart_flag:
                k += 1  # a restart is a frame of the dump that carries no canvas
    finally:
        ft.close()
    assert len(frames) == k and sum(f[1] for f in frames) == 1
    assert len(want) >= 4 and unpublished >= 1  # frames that publish nothing are shown too (node:257 precedes :268)
    assert got == want
