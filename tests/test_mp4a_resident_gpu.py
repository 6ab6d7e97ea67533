"""'mp4a' decoders on the resident route (SharedEngine({ resident: true, residentPackets: true })): the blocks of MP4 chunks found
by the device walk (aacg_pipeline_walk_submit / _collect through the N-API addon), decoded by the resident pipeline.  CPU: the
option routes an 'mp4a' decoder there, and only the option does.  GPU: the committed streams as MP4 chunks give the PCM the same
streams give as ADTS on the resident route, bit for bit, with ADTS streams on the same engine, overlap on and off, a PCM ring and
packets longer than the look-ahead; errors come where the parsing route raises them."""
import os
import subprocess

import pytest

from resident_kit import NODE, ROOT

SCRIPT = os.path.join(ROOT, "tests", "js", "test_mp4a_resident.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / node_api.h not present on this machine")


@needs_node
def test_resident_packets_option_routes_mp4a():
    r = subprocess.run([NODE, SCRIPT, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mp4a resident cpu tests ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@needs_node
def test_mp4a_chunks_on_the_resident_route():
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, SCRIPT, "gpu"], capture_output=True, text=True, timeout=500)
    assert r.returncode == 0 and "mp4a resident gpu tests ok" in r.stdout, r.stdout + r.stderr
