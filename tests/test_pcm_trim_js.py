"""The trim's rule under Node (tests/js/test_trim.js): aac.js_amd/js/trim.js — aacg_trim_counts' and aacg_trim_design's arithmetic and the
per-stream slicing of chunks on the host, for decoders that do not take the resident route — against vectors the Python rule makes
(trim_kit, in Python integers and fractions; written into a temporary file, not committed); the addon's trimDesign against the same
vectors; and on a GPU SharedEngine({ resident: true, trim: true }) — two stereo streams, f32 and int16, with and without sampleRate: 16000,
and decoders forced onto the parsing route: readChunk() equals the same engine's untrimmed output sliced by trim.js, chunk lengths
included, and no chunk is delivered for frames inside the priming."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

import trim_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_trim.js")
needs_addon = pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present on this machine")


def make_vectors():
    pieces = [1024, 1024, 341, 342, 1, 0, 1024, 2048]
    vec = {"counts": [], "design": [], "streams": []}
    for position, (skip, keep) in itertools.product((0, 1, 2112, 2 ** 32 + 12345, 2 ** 45), ((0, None), (0, 0), (2112, None), (1, 5000), (1024, 1024), (1023, 2), (2389, 343), (5803, 1))):
        for s in (skip, position + skip):
            if s < kit.LIMIT:
                first, kept = kit.counts(position, s, keep, pieces)
                vec["counts"].append({"position": position, "skip": s, "keep": keep, "n_in": pieces, "first_of": first, "kept_of": kept})
    for (L, M), taps, skip_in, keep_in, limiter in itertools.product(((1, 3), (160, 441), (160, 147), (441, 160), (2, 1), (1, 1)), (0, 8, 32), (0, 1024, 2112, 2113, 2 ** 33 + 17),
                                                                      (None, 0, 5000, 2 ** 33 + 5), (False, True)):
        if taps == 0 and (L, M) != (1, 1):
            continue
        skip, keep, residual = kit.design(skip_in, keep_in, limiter, L, M, taps)
        vec["design"].append({"skip_in": skip_in, "keep_in": keep_in, "limiter": limiter, "L": L, "M": M, "taps": taps, "skip": skip, "keep": keep,
                              "residual": [residual.numerator, residual.denominator]})
    for channels, (skip, keep), chunks in itertools.product((1, 2, 6), ((0, None), (2112, None), (1, 5000), (0, 0), (2047, 2), (1024, 1024)), ([1024] * 7, [341, 342, 341, 1024, 2048, 3, 1024])):
        delivered, at = [], 0
        for n in chunks:
            first, kept = kit.span(at, skip, keep, n)
            if kept:
                delivered.append([kept, (((at + first) * channels) * 7 + 1) % 30000])      # the length and the first element of the chunk test_trim.js makes
            at += n
        vec["streams"].append({"channels": channels, "skip": skip, "keep": keep, "chunks": chunks, "delivered": delivered})
    return vec


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_trim_js_is_the_rule(tmp_path):
    vec = make_vectors()
    assert len(vec["counts"]) > 50 and len(vec["design"]) > 300 and any(not s["delivered"] for s in vec["streams"])
    path = str(tmp_path / "trim_vectors.json")
    with open(path, "w") as f:
        json.dump(vec, f)
    r = subprocess.run([NODE, SCRIPT, "cpu", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "trim cpu tests ok" in r.stdout, r.stdout + r.stderr


@needs_addon
def test_trim_design_through_the_addon(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = str(tmp_path / "trim_vectors.json")
    with open(path, "w") as f:
        json.dump(make_vectors(), f)
    r = subprocess.run([NODE, SCRIPT, "design", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "trim design tests ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@needs_addon
def test_shared_engine_trim_gpu():
    """two stereo streams on SharedEngine({ resident: true, trim: true }), f32 and int16, with and without sampleRate: 16000, and decoders
    forced onto the parsing route: readChunk() is the same engine's untrimmed output sliced by trim.js, chunk lengths included; no chunk
    for frames inside the priming; without the option, and with default windows, nothing differs"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, SCRIPT, "gpu"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "trim gpu tests ok" in r.stdout, r.stdout + r.stderr
