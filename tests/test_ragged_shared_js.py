"""SharedEngine({ resident: true, ragged: true }) under Node with a stub addon (no GPU): what a flush submits — per-stream counts,
frame tables packed stream after stream, per-stream PCM views — and, without `ragged`, the batch cut to the fewest frames as before;
the jittered-arrival driver reads every frame it feeds.  The GPU half is in tests/test_ragged_pipeline_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_ragged_flush_with_a_stub_addon():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_ragged_shared.js"), "cpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ragged shared cpu tests ok" in r.stdout, r.stdout + r.stderr
