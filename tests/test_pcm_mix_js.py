"""The downmix under Node (tests/js/test_mix.js): aac.js_amd/js/mix.js — the rule of include/aacgpu.h on the host, for the decoders of a
SharedEngine({ downmix }) that do not take the resident route — against vectors written by the Python rule (mix_kit.mix_rule; the
committed tests/golden/mix/vectors.json, which this file can write again: python tests/test_pcm_mix_js.py), addon.mixStandard against
the table, and on a GPU SharedEngine({ resident: true, downmix: 'stereo' }) against mix.js over the same engine's unmixed output."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mix_kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
VECTORS = os.path.join(ROOT, "tests", "golden", "mix", "vectors.json")
needs_addon = pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present on this machine")
N = 24            # samples of a case


def bits(a):
    a = np.ascontiguousarray(a)
    return [int(v) for v in (a.view(np.uint32) if a.dtype == np.float32 else a).ravel()]


def make_vectors():
    """every C x O: float samples of mixed sign over 2^-20 .. 2^3 and int16 samples with the ends of the range and the largest sums
    either way through the hostile matrix, and small int16 samples through coefficients of 0.5 (exact halves); then the standard table"""
    cases = []
    for channels in range(1, 9):
        for out_channels in (1, 2):
            m = mix_kit.hostile_matrix(out_channels, channels)
            rng = np.random.default_rng(1000 + 10 * channels + out_channels)
            xf = (rng.choice([-1.0, 1.0], (N, channels)) * np.exp2(rng.uniform(-20.0, 3.0, (N, channels)))).astype(np.float32)
            xi = rng.integers(-32768, 32768, (N, channels)).astype(np.int16)
            xi[0, :], xi[1, :] = 32767, -32768
            for k, row in enumerate(m):
                xi[2 + 2 * k, :] = np.where(row >= 0, 32767, -32768)
                xi[3 + 2 * k, :] = np.where(row >= 0, -32768, 32767)
            half = np.full((out_channels, channels), 0.5, np.float32)
            xh = rng.integers(-5, 6, (N, channels)).astype(np.int16)
            xh[:6, 0] = [1, 3, 5, -1, -3, -5]
            xh[:6, 1:] = 0
            for name, x, mat in (("f32", xf, m), ("i16", xi, m), ("i16 halves", xh, half)):
                cases.append({"name": "%s %d -> %d" % (name, channels, out_channels), "channels": channels, "outChannels": out_channels,
                              "type": "f32" if x.dtype == np.float32 else "i16", "matrix": bits(mat), "x": bits(x), "want": bits(mix_kit.mix_rule(x, mat))})
    standard = []
    for channels in sorted(mix_kit.POSITIONS):
        for out_channels in (1, 2):
            for normalise in (0, 1):
                for gain in (2.0 ** -0.5, 0.5):
                    g = np.float32(gain)
                    standard.append({"channels": channels, "outChannels": out_channels, "normalise": normalise, "gain": bits(np.array([g]))[0],
                                     "matrix": bits(mix_kit.standard_table(channels, out_channels, g, normalise))})
    return {"cases": cases, "standard": standard}


def test_committed_vectors_are_the_python_rule():
    """the fixture is what the rule in mix_kit gives today: the JavaScript legs below are pinned to the same rule as the emulator and
    the GPU tests"""
    assert json.load(open(VECTORS)) == make_vectors()
    assert os.path.getsize(VECTORS) < 256 * 1024


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_mix_js_is_the_rule():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_mix.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mix cpu tests ok" in r.stdout, r.stdout + r.stderr


@needs_addon
def test_mix_standard_through_the_addon():
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_mix.js"), "standard"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mix standard tests ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@needs_addon
def test_shared_engine_downmix_gpu():
    """two 5.1 streams on SharedEngine({ resident: true, downmix }) — 'stereo' and a matrix of the caller's, f32 and int16 — and decoders
    forced onto the parsing route: readChunk() is mix.js over the same engine's unmixed output, bit for bit"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_mix.js"), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mix gpu tests ok" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    os.makedirs(os.path.dirname(VECTORS), exist_ok=True)
    with open(VECTORS, "w") as f:
        json.dump(make_vectors(), f, separators=(",", ":"))
    print("wrote", VECTORS, os.path.getsize(VECTORS), "bytes")
