"""SharedEngine({ resident: true, carryWindowShape: true }) under Node with a stub addon (no GPU): a decoder that carries its window
shape takes the resident route of an engine made with the option, the pipeline is created with stages 4 (7 with both spec modes), a
mismatch either way goes to the parsing route, int16 PCM goes with it.  The GPU half is in tests/test_resident_shape_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_carried_window_shape_takes_the_resident_route_with_a_stub_addon():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_resident_shape.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "resident shape cpu tests ok" in r.stdout, r.stdout + r.stderr
