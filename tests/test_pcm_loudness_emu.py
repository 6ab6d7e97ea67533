"""The loudness tap on a resident batch's transform PCM (aacg_pcm_loudness, aac.js_amd/csrc/aacg_pcm_loudness.h: loudness_body) against the
rule of include/aacgpu.h as a plain numpy-float32 loop (loudness_kit.rule), bit for bit — the records AND the state left behind — with
poisoned guards around the record buffer and the state block: the kernel's source run lane by lane on CPU threads
(tests/emu/loudness_emu.cpp with tests/emu/devport_emu.h).

The rule: per sample, section 0 then 1, y = (b0 v) + z1; z1 = ((b1 v) - (a1 y)) + z2; z2 = (b2 v) - (a2 y); v = y; then e = e + (v v),
peak = max(peak, |x|), every operation rounded to float32 on its own; after every `hop` samples {e, peak} leaves and both restart at +0.
Then conformance: BS.1770's filters over a 997 Hz sine at -23 dBFS integrate to -23.0 LUFS within 0.01 LU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import aacgpu
import emu_lib
import loudness_kit as kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 1024            # poisoned floats on either side of the records and of the state
REC = np.dtype([(n, np.uint32) for n in ("frame_first", "frames", "out_first", "n_out", "n0", "slot", "parity", "fresh")])
POISON = np.float32(-77.25)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("loudness_emu", ["tests/emu/loudness_emu.cpp"], tmp_path_factory.mktemp("loudness_emu"))
    L.emu_loudness.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 3 + [C.c_int]
    L.emu_loudness.restype = C.c_int
    sizes = (C.c_uint32 * 4)()
    L.emu_loudness_sizes(sizes)
    assert sizes[0] == 64 and sizes[1] == REC.itemsize == 32 and sizes[2] == 6
    return L


def guarded(n_floats):
    """n_floats at a 16-byte aligned address inside a block with GUARD poisoned floats on either side: (block, view)"""
    raw = np.full(GUARD + n_floats + GUARD + 4, POISON, np.float32)
    off = ((-(raw.ctypes.data + 4 * GUARD)) % 16) // 4
    block = raw[off:off + GUARD + n_floats + GUARD]
    return block, block[GUARD:GUARD + n_floats]


def guards_intact(block, n_floats):
    return (block[:GUARD] == POISON).all() and (block[GUARD + n_floats:] == POISON).all()


def source(n, channels, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        x = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
        x[:3] = [[32767] * channels, [-32768] * channels, [-32767] * channels]
        return x
    return (rng.choice([-1.0, 1.0], (n, channels)) * np.exp2(rng.uniform(-20.0, 1.0, (n, channels)))).astype(np.float32)


class Slots:
    """what the host keeps for `n` slots — clocks, parities, fresh flags —, the state block the device keeps, and the rule's own state"""

    def __init__(self, n, channels):
        self.C, self.n = channels, n
        self.block, raw = guarded(n * 2 * channels * 6)
        self.state = raw.reshape(n, 2, channels, 6)
        self.N, self.parity, self.fresh = [0] * n, [0] * n, [1] * n
        self.ref = [kit.State(channels) for _ in range(n)]

    def reset(self, slot):
        self.N[slot], self.fresh[slot], self.ref[slot] = 0, 1, kit.State(self.C)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert wrong.size == 0, "%s: the kernel differs from the rule at %d of %d values, first at %s: %r against %r" % (
        what, len(wrong), got.size, wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])])


def launch(lib, S, xs, slots, hop, coeffs, blocks=None, reverse=0, check=True):
    """one emulated launch: stream s brings xs[s] (frames * 1024, C) for slot slots[s].  Returns each stream's records (n_out, C, 2),
    compares them and the state left behind with the rule's, bit for bit, and advances S."""
    dtype, channels = xs[0].dtype, xs[0].shape[1]
    rec = np.zeros(len(xs), REC)
    first = out_first = 0
    for s, (x, slot) in enumerate(zip(xs, slots)):
        frames = len(x) // 1024
        n = (S.N[slot] % hop + len(x)) // hop
        rec[s] = (first, frames, out_first, n, S.N[slot] % hop, slot, S.parity[slot], S.fresh[slot])
        first, out_first = first + frames, out_first + n
    packed = np.concatenate(xs)
    raw = np.zeros(packed.nbytes + 16, np.uint8)
    src = raw[(-raw.ctypes.data) % 16:][:packed.nbytes]
    src.view(dtype)[:] = packed.reshape(-1)
    n_dst = out_first * channels * 2
    dst_block, dst = guarded(n_dst)
    before = S.state.copy()
    k = np.ascontiguousarray(coeffs, np.float32).reshape(10)
    groups = -(-len(xs) // (64 // channels))
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 8 == 0
    assert lib.emu_loudness(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), S.state.ctypes.data, hop, k.ctypes.data,
                            channels, xs[0].dtype.itemsize, groups + 1 if blocks is None else blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst), "a float outside the records was written"
    assert guards_intact(S.block, S.state.size), "a float outside the state was written"
    assert (src.view(dtype) == packed.reshape(-1)).all()
    flat = dst.reshape(out_first, channels, 2)
    outs = [flat[r["out_first"]:r["out_first"] + r["n_out"]].copy() for r in rec]
    assert not (flat.view(np.uint32) == POISON.view(np.uint32)).any(), "a record was not written"
    untouched = np.ones(S.state.shape[:2], bool)
    for s, (x, slot) in enumerate(zip(xs, slots)):
        new = S.parity[slot] ^ 1
        if check:
            want = kit.rule(x, hop, coeffs, S.ref[slot])
            same_bits(outs[s], want, "stream %d, records" % s)
            same_bits(S.state[slot, new], S.ref[slot].floats(), "stream %d, the state left behind" % s)
        untouched[slot, new] = False
        S.N[slot], S.parity[slot], S.fresh[slot] = S.N[slot] + len(x), new, 0
    assert (S.state.view(np.uint32)[untouched] == before.view(np.uint32)[untouched]).all(), "the other parity's state or another slot's was written"
    return outs


# (hop, channels, per batch the frames of each stream) — the smallest shapes that can go wrong: a hop far below a tile and one that is a
# frame; ragged streams in one group; six channels (ten streams a group, four lanes idle); a hop that spans batches, so that some emit
# nothing; eight channels with a hop that is no multiple of anything
SHAPES = [(7, 1, [[1]]),
          (1000, 2, [[1, 3, 2], [3, 1, 1]]),
          (1024, 6, [[2, 1]]),
          (4800, 2, [[1, 2], [3, 1], [2, 3]]),
          (5000, 8, [[1]] * 6)]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["hop7-c1", "hop1000-c2-ragged", "hop1024-c6", "hop4800-c2-3batches", "hop5000-c8-6batches"])
def test_loudness_is_the_rule(lib, shape, dtype):
    """fresh slots, then both parities batch after batch, hostile coefficients; one workgroup more than there are groups, then one
    workgroup that walks every group, in reverse"""
    hop, channels, batches = shape
    coeffs = kit.hostile_coeffs(hop + channels)
    n_streams = len(batches[0])
    S = Slots(n_streams + 2, channels)
    slots = [n_streams + 1 - s for s in range(n_streams)]                             # not in order, not from 0
    emitted, parities = [], set()
    for b, frames_of in enumerate(batches):
        xs = [source(f * 1024, channels, dtype, 1000 * b + 10 * s + channels) for s, f in enumerate(frames_of)]
        parities |= {S.parity[slot] for slot in slots}
        outs = launch(lib, S, xs, slots, hop, coeffs, None if b % 2 == 0 else 1, b % 2)
        emitted.append([len(o) for o in outs])
    for s, slot in enumerate(slots):
        assert sum(e[s] for e in emitted) == S.N[slot] // hop
    if len(batches) > 1:
        assert parities == {0, 1}
    if hop > 1024:
        assert any(0 in e for e in emitted) and any(max(e) > 0 for e in emitted), "a hop that spans batches: some emit nothing"


@pytest.mark.parametrize("channels,n_streams", [(8, 9), (3, 22), (1, 65)])
def test_more_streams_than_a_workgroup_takes(lib, channels, n_streams):
    """one stream more than a group of 64 / C: two groups, with two workgroups in reverse and with one that takes both in turn"""
    coeffs = kit.hostile_coeffs(channels)
    for blocks, dtype in ((2, np.float32), (1, np.int16)):
        S = Slots(n_streams, channels)
        xs = [source(1024, channels, dtype, 7 * s + channels) for s in range(n_streams)]
        outs = launch(lib, S, xs, list(range(n_streams))[::-1], 500, coeffs, blocks, 1)
        assert all(len(o) == 2 for o in outs)


def test_a_reset_between_batches(lib):
    """a slot that is reset starts from nothing — clock, filters, energy, peak — while its neighbour goes on"""
    hop, channels, coeffs = 1000, 2, kit.hostile_coeffs(5)
    S = Slots(2, channels)
    launch(lib, S, [source(2048, channels, np.float32, 1), source(1024, channels, np.float32, 2)], [0, 1], hop, coeffs)
    S.reset(0)
    x = source(1024, channels, np.float32, 3)
    outs = launch(lib, S, [x, source(1024, channels, np.float32, 4)], [0, 1], hop, coeffs)
    same_bits(outs[0], kit.rule(x, hop, coeffs, kit.State(channels)), "the reset slot against a new stream")
    assert len(outs[0]) == 1 and len(outs[1]) == 1 and S.N == [1024, 2048]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_any_split_into_batches_gives_the_same_bits(lib, dtype):
    """EVERY split of five frames into batches — all sixteen compositions of 5 — beside a second stream that is there in some batches
    only: the records concatenated are the rule's over the five frames, and the final state is the same"""
    hop, channels, coeffs = 1000, 2, kit.hostile_coeffs(17)
    x, other = source(5 * 1024, channels, dtype, 42), source(1024, channels, dtype, 43)
    whole = kit.State(channels)
    want = kit.rule(x, hop, coeffs, whole)
    assert len(want) == 5
    for cuts in itertools.product([0, 1], repeat=4):
        split, run = [], 1
        for c in cuts:
            if c:
                split.append(run)
                run = 0
            run += 1
        split.append(run)
        S, got, at = Slots(3, channels), [], 0
        for b, frames in enumerate(split):
            part = x[at * 1024:(at + frames) * 1024]
            xs, slots = ([other, part], [0, 2]) if b % 2 == 0 and len(split) > 1 else ([part], [2])
            got.append(launch(lib, S, xs, slots, hop, coeffs, None, b % 2, check=False)[-1])
            at += frames
        same_bits(np.concatenate(got), want, "split %s" % split)
        same_bits(S.state[2, S.parity[2]], whole.floats(), "split %s, the final state" % split)


def test_a_burst_dies_away_through_subnormals(lib):
    """a frame of noise, then 20 frames of zeros, a frame per batch, with poles of radius 0.995: the filters' z values decay by e^-5 a
    frame and pass through the subnormal range between the 17th and the 21st — a unit that flushed them would differ from the rule"""
    channels, hop = 2, 1000
    r = 0.995
    coeffs = np.array([[1.0, -0.5, 0.25, -2 * r * np.cos(0.3), r * r], [0.75, 0.5, -0.25, -2 * r * np.cos(1.1), r * r]], np.float32)
    S = Slots(1, channels)
    seen = False
    for b in range(21):
        x = source(1024, channels, np.float32, 9) if b == 0 else np.zeros((1024, channels), np.float32)
        launch(lib, S, [x], [0], hop, coeffs, 1, 0)
        z = np.abs(S.state[0, S.parity[0], :, :4])
        seen = seen or bool(((z > 0) & (z < np.finfo(np.float32).tiny)).any())
    assert seen, "no z value was subnormal at any batch's end: the case does not test what it is for"


def test_loudness_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: the ragged batch
    (1, 3 and 2 frames, one stream in mid-hop), 1, 2, 3 and 8 channels, both element sizes, over heap blocks of exactly the buffers'
    sizes.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "loudness_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DLOUDNESS_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "loudness_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "loudness_emu: ok" in r.stdout, r.stdout + r.stderr


def test_conformance_997_hz_at_minus_23(lib, engine_lib):
    """BS.1770 / EBU Tech 3341, case 1 in kind: a 2 s stereo 997 Hz sine of peak 10^(-23/20) measures -23.0 LUFS within 0.01 LU (the
    rule gives -23.0003 in float64; float32 hop energies differ from float64 by at most 3e-4 dB on this signal), with
    loudness_design(48000) and a hop of 4800; every record's peak is the hop's max |x|, exactly"""
    d = aacgpu.loudness_design(48000)
    assert d["hop"] == 4800
    n = 94 * 1024                                                         # 2 s and the rest of the last frame
    t = np.arange(n, dtype=np.float64) / 48000.0
    x = np.repeat((10.0 ** (-23.0 / 20.0) * np.sin(2 * np.pi * 997.0 * t)).astype(np.float32)[:, None], 2, axis=1)
    S = Slots(1, 2)
    rec = launch(lib, S, [x], [0], 4800, d["coeffs"], 1, 0, check=False)[0]
    assert rec.shape == (20, 2, 2)
    lufs = aacgpu.loudness_integrate(rec, 4800)
    print("integrated: %.6f LUFS" % lufs)
    assert abs(lufs - (-23.0)) <= 0.01
    want_peak = np.abs(x[:20 * 4800]).reshape(20, 4800, 2).max(axis=1)
    assert (rec[:, :, 1].view(np.uint32) == want_peak.view(np.uint32)).all()
