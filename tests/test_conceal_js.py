"""SharedEngine({ resident: true, ragged: true, devicePlans: true, conceal: ... }) under Node (tests/js/test_conceal.js).  With a stub
addon (no GPU): the option reaches the pipeline's config, throws at construction without devicePlans, a result that carries the concealed
flag delivers its PCM and is counted, a refused frame without it still throws.  On a real MI355X: three streams, one frame cut to 9
bytes — readChunk() returns PCM for that frame, the same bits as the Python pipeline's for the same bytes, stats.concealedFrames is 1, and
without the option the same feed throws the reference's message."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_conceal.js")


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_conceal_option_with_a_stub_addon():
    r = subprocess.run([NODE, SCRIPT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "conceal cpu tests ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_behind_the_plugin_surface(tmp_path):
    import aacgpu
    from resident_kit import adts_frame_table, packed, rect_script, same_bits
    d, out = str(tmp_path / "streams"), str(tmp_path / "out")
    os.makedirs(d)
    os.makedirs(out)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "shape_cases.js"), d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([NODE, SCRIPT, "gpu", d, out], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "conceal gpu tests ok" in r.stdout, r.stdout + r.stderr
    # the same bytes through the Python pipeline, four frames a batch
    feeds = [np.fromfile(os.path.join(out, "feed_%d.aac" % i), np.uint8) for i in range(3)]
    tables = [adts_frame_table(f) for f in feeds]
    assert [len(t) for t in tables] == [12, 12, 12] and int(tables[1]["byte_length"][5]) == 9
    data, bases = np.concatenate(feeds), np.cumsum([0] + [len(f) for f in feeds])[:-1]
    p = aacgpu.Pipeline(channels=2, max_streams=3, max_frames=4, device_plans=True, conceal=True)
    want, flagged = [[] for _ in range(3)], []
    for live, counts, at in rect_script(3, 4, 12):
        pcm, res, refused = p.decode(data, packed(tables, bases, at, counts), np.array(live, np.uint32), np.array(counts, np.uint32))
        flagged += [(int(i) // 4, at[0] + int(i) % 4) for i in np.flatnonzero(res["flags"] & aacgpu.PARSE_CONCEALED)]
        for s in live:
            want[s].append(pcm[s * 4 * 2048:(s + 1) * 4 * 2048].copy())
    assert flagged == [(1, 5)] and p.concealed() == 1
    p.close()
    for s in range(3):
        got = np.fromfile(os.path.join(out, "js_%d.f32" % s), np.float32)
        assert same_bits(got, np.concatenate(want[s])), "stream %d: readChunk() and the Python pipeline give other bits" % s
