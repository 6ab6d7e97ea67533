"""The resampler under Node (tests/js/test_resample.js): aac.js_amd/js/resample.js — the rule of include/aacgpu.h on the host, for the
decoders of a SharedEngine({ sampleRate }) that do not take the resident route, and the per-frame shares the engine slices a resident
batch's output by — against vectors the Python rule makes (resample_kit.resample_rule; written into a temporary file, not committed),
addon.resampleDesign, and on a GPU SharedEngine({ resident: true, sampleRate: 16000 }) against resample.js over the same engine's plain
output, chunk lengths included."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import resample_kit as kit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "test_resample.js")
needs_addon = pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present on this machine")
FRAME, FRAMES = 1024, 3


def bits(a):
    a = np.ascontiguousarray(a)
    return [int(v) for v in (a.view(np.uint32) if a.dtype == np.float32 else a).ravel()]


def make_vectors():
    """every ratio with 4 and 32 taps (441 / 160: 4 and 16) through a hostile table, 1..3 channels in turn: float samples of mixed sign
    over 2^-20 .. 2^3, int16 samples over the whole range (sums that saturate both ways), and small int16 samples through rows of
    (0.5, 0.5, 0, 0) — exact halves; three frames of 1024, so that the second and third begin in mid-phase with a history"""
    cases = []
    for k, (L, M) in enumerate(kit.RATIOS):
        for j, taps in enumerate((4, 32 if L * 32 <= 16384 else 16)):
            channels = 1 + (k + j) % 3
            table = kit.hostile_table(L, taps)
            rng = np.random.default_rng(1000 + 10 * k + j)
            xf = (rng.choice([-1.0, 1.0], (FRAME * FRAMES, channels)) * np.exp2(rng.uniform(-20.0, 3.0, (FRAME * FRAMES, channels)))).astype(np.float32)
            xi = rng.integers(-32768, 32768, (FRAME * FRAMES, channels)).astype(np.int16)
            xi[10:20], xi[30:40] = 32767, -32768
            sets = [("f32", xf, table), ("i16", xi, table)]
            if taps == 4:
                sets.append(("i16 halves", rng.integers(-6, 7, (FRAME * FRAMES, channels)).astype(np.int16), np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (L, 1))))
            for name, x, h in sets:
                want = kit.resample_rule(x, L, M, h)
                if name == "i16":
                    assert (want == 32767).any() and (want == -32768).any()
                cases.append({"name": "%s %d / %d, %d taps, %d channels" % (name, L, M, taps, channels), "L": L, "M": M, "taps": taps, "channels": channels,
                              "frame": FRAME, "type": "f32" if x.dtype == np.float32 else "i16", "table": bits(h), "x": bits(x), "want": bits(want),
                              "counts": [kit.n_out(f * FRAME, (f + 1) * FRAME, L, M) for f in range(FRAMES)]})
    return {"cases": cases, "expect": len(cases)}


@pytest.mark.skipif(NODE is None, reason="node not present on this machine")
def test_resample_js_is_the_rule(tmp_path):
    vectors = make_vectors()
    assert vectors["expect"] == 25
    path = str(tmp_path / "vectors.json")
    with open(path, "w") as f:
        json.dump(vectors, f, separators=(",", ":"))
    r = subprocess.run([NODE, SCRIPT, "cpu", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "resample cpu tests ok" in r.stdout, r.stdout + r.stderr


@needs_addon
def test_resample_design_through_the_addon():
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, SCRIPT, "design"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resample design tests ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@needs_addon
def test_shared_engine_sample_rate_gpu():
    """two stereo streams on SharedEngine({ resident: true, sampleRate: 16000 }), f32 and int16, and decoders forced onto the parsing
    route: readChunk() is resample.js over the same engine's plain output, bit for bit, each chunk its frame's share of the output"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "aac.js_amd", "napi")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([NODE, SCRIPT, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "resample gpu tests ok" in r.stdout, r.stdout + r.stderr
