"""GPU: tools/replay_node show=1 in replay mode (ahead=1, 2, 3, and 3 with lazy=1 threads=2) on the log of
tests/test_event_image_replay_gpu.py: the setting is ESVIO_FE_EVENT_IMAGES_AHEAD there, and the dump — the frames and
every tracked frame's `show` hash line — is byte for byte that of ahead=0 show=1."""
import re
import subprocess

import pytest

import test_event_image_replay_gpu as S
import test_replay_node_gpu as T
from esvio_amd import frontend as FE

pytestmark = pytest.mark.gpu


def test_show_hashes_in_replay_mode_equal_the_plain_schedules(tmp_path):
    log = str(tmp_path / "log.esvb")
    T._write_log(log, S.messages())
    from esvio_amd import build as B
    tool, dumps = B.build_tools(), {}
    runs = (("ahead0", ["ahead=0"]), ("ahead1", ["ahead=1"]), ("ahead2", ["ahead=2"]), ("ahead3", ["ahead=3"]),
            ("ahead3_lazy", ["ahead=3", "lazy=1", "threads=2"]))
    for name, opts in runs:
        dump = str(tmp_path / (name + ".bin"))
        p = subprocess.run([tool, log, dump, "max_cnt=%d" % T.KW["max_cnt"], "min_dist=%d" % T.KW["min_dist"], "freq=%d" % T.FREQ,
                            "lk_accum=%d" % FE.DEFAULT_LK_ACCUM, "show=1"] + opts, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (name, p.stdout + p.stderr)
        dumps[name] = open(dump, "rb").read()
    lines = re.findall(rb"show \d+ [0-9a-f]{16}\n", dumps["ahead0"])  # (they follow the last frame's bytes)
    assert dumps["ahead0"].endswith(b"".join(lines))
    assert len(lines) >= 4 and len(set(l.split()[2] for l in lines)) == len(lines)  # every frame's canvas has a hash of its own
    for name, _ in runs[1:]:
        assert dumps[name] == dumps["ahead0"], name
