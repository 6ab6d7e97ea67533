"""SharedEngine({ resident: true, ragged: true, devicePlans: true }) under Node with a stub addon (no GPU): the option reaches every
pipeline's config (planMode 1), it is off by default, a flush submits the same batches in either mode, and the counters are summed.
The GPU half is in tests/test_device_plans_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_device_plans_option_with_a_stub_addon():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_device_plans.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device plans cpu tests ok" in r.stdout, r.stdout + r.stderr
