"""A resident batch's one-channel PCM framed and transformed to (log-)mel features (aacg_pcm_features, aac.js_amd/csrc/aacg_pcm_features.h:
features_body) against the rule of include/aacgpu.h as a straight C loop of fmaf (emu_features_rule in the same driver, which shares no
code with the body), BIT FOR BIT, with a poisoned guard on both sides of the destination and of the history block: the kernel's source
run lane by lane on CPU threads (tests/emu/features_emu.cpp with tests/emu/devport_emu.h; the matrix-core primitive is the twin of
tests/emu/devport_mfma_emu.h).

The tables are hostile, not Hann: random entries with |v| in [0.5, 2) and mixed signs, and an x that never repeats, so that any
mis-indexed sample, row or bin shows grossly.  A stream in mid-flight is checked against the rule over a WHOLE stream — made-up earlier
input, then the batch's samples — so the kernel's history and the records' arithmetic are what is tested."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import features_kit as kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096            # poisoned bytes on either side of the destination and of the history
FLOOR = 1e-3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return kit.driver(tmp_path_factory.mktemp("features_emu"))


def guarded(n_bytes, fill):
    """n_bytes at a 16-byte aligned address inside a block with GUARD poisoned bytes on either side: (block, view)"""
    raw = np.full(GUARD + n_bytes + GUARD + 16, fill, np.uint8)
    off = (-(raw.ctypes.data + GUARD)) % 16
    block = raw[off:off + GUARD + n_bytes + GUARD]
    return block, block[GUARD:GUARD + n_bytes]


def guards_intact(block, n_bytes, fill):
    return (block[:GUARD] == fill).all() and (block[GUARD + n_bytes:] == fill).all()


class Slots:
    """the state the host keeps and the history block the device keeps, for `n` slots: clocks, parities, fresh flags"""

    def __init__(self, n, K):
        self.K, self.n = K, n
        self.bytes = n * 2 * (K - 1) * 4
        self.block, raw = guarded(self.bytes, 0x5A)
        self.hist = raw.view(np.float32).reshape(n, 2, K - 1)
        self.hist[:] = np.float32(-77.25)                # what nobody has written yet: any read of it shows
        self.N, self.parity, self.fresh = [0] * n, [0] * n, [1] * n
        self.tail = [np.zeros(K - 1, np.float32) for _ in range(n)]      # the last K - 1 samples of (zeros, everything consumed)

    def seed(self, slot, pre, parity):
        """the slot has consumed `pre` (float32) already: the clock, and its last K - 1 samples in the buffer its next launch reads"""
        self.N[slot], self.fresh[slot], self.parity[slot] = len(pre), 0, parity
        self.tail[slot] = np.concatenate([self.tail[slot], pre])[-(self.K - 1):]
        self.hist[slot, parity] = self.tail[slot]


def launch(lib, state, xs, slots, shape, basis, fb, log, row_extra, blocks, reverse):
    """one emulated launch: stream s brings xs[s] (samples,) for slot slots[s]; row_extra: None packed, else planar with that many frames
    more per row than the longest stream has.  Returns each stream's frames (n_out, n_mels) and advances `state`."""
    K, H, P, B, NM = shape
    dtype = xs[0].dtype
    rec = np.zeros(len(xs), kit.REC)
    first = out_first = items = 0
    for s, (x, slot) in enumerate(zip(xs, slots)):
        N = state.N[slot]
        j0 = kit.count(N, K, H, P)
        n = kit.count(N + len(x), K, H, P) - j0
        off0 = j0 * H - P - N
        assert -(K - 1) <= off0 <= 0
        rec[s] = (first, len(x), out_first, n, items, off0, slot, state.parity[slot] | (state.fresh[slot] << 1))
        first, out_first, items = first + len(x), out_first + n, items + max(1, -(-n // kit.TILE))
    row = None if row_extra is None else max(1, int(rec["n_out"].max()) + row_extra)
    packed = np.concatenate(xs)
    src_block, src = guarded(packed.nbytes, 0)
    src.view(dtype)[:] = packed
    n_dst = (len(xs) * NM * row if row else out_first * NM) * 4
    dst_block, dst = guarded(n_dst, 0xC3)
    before = state.hist.copy()
    blocks = items + 2 if blocks is None else blocks
    assert lib.emu_features(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), items, basis.ctypes.data, fb.ctypes.data, state.hist.ctypes.data,
                            K, H, 2 * B, NM, FLOOR, 1 if log else 0, row or 0, dtype.itemsize, blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst, 0xC3), "a byte outside the destination was written"
    assert guards_intact(state.block, state.bytes, 0x5A), "a byte outside the history was written"
    assert (src.view(dtype) == packed).all()
    outs = []
    if row:
        whole = dst.view(np.float32).reshape(len(xs), NM, row)
        pad = np.float32(np.log10(np.float64(np.float32(FLOOR)))) if log else np.float32(0.0)
        for s in range(len(xs)):
            n = int(rec[s]["n_out"])
            outs.append(whole[s, :, :n].T.copy())
            padding = whole[s, :, n:]
            assert padding.size == NM * (row - n)
            if log:
                assert (kit.ulps(padding, np.full_like(padding, pad)) <= 4).all() and (padding == padding.flat[0]).all(), "the planar padding is not log10f(floor)"
            else:
                assert (padding.view(np.uint32) == 0).all(), "the planar padding is not +0"
    else:
        flat = dst.view(np.float32).reshape(out_first, NM)
        for s in range(len(xs)):
            outs.append(flat[rec[s]["out_first"]:rec[s]["out_first"] + rec[s]["n_out"]].copy())
    # the history: the streams' new parity holds the last K - 1 of everything consumed, everything else is as it was
    untouched = np.ones(state.hist.shape[:2], bool)
    for x, slot in zip(xs, slots):
        new = state.parity[slot] ^ 1
        state.tail[slot] = np.concatenate([state.tail[slot], kit.as_float(x)])[-(K - 1):]
        assert np.array_equal(state.hist[slot, new].view(np.uint32), state.tail[slot].view(np.uint32)), "the new history is not the last K - 1 samples"
        untouched[slot, new] = False
        state.N[slot], state.parity[slot], state.fresh[slot] = state.N[slot] + len(x), new, 0
    assert (state.hist.view(np.uint32)[untouched] == before.view(np.uint32)[untouched]).all(), "the other parity's buffer or another slot's was written"
    return outs


def frames_for(shape):
    """AAC frames (1024 samples) of the three streams: 1..3, fewer where a hop of 1 makes a frame a thousand feature frames"""
    return (1, 1, 1) if shape[1] == 1 else (3, 1, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("shape", kit.SHAPES, ids=["K%d-H%d-P%d-B%d-M%d" % s for s in kit.SHAPES])
def test_features_are_the_rule(lib, shape, dtype):
    """three streams in one launch — a fresh one, one with history at parity 0 and one at parity 1 (clocks that are no multiple of
    anything) — linear, packed with one workgroup (it walks every item) and planar with every padding element checked, four
    workgroups in reverse; the third way has two more workgroups than items"""
    K, H, P, B, NM = shape
    basis, fb = kit.hostile_tables(K, B, NM)
    counts = frames_for(shape)
    for way, (row_extra, blocks, reverse) in enumerate([(None, 1, 0), (3, 4, 1), (None, None, 0)]):
        if way == 2 and (dtype == np.int16 or H == 1):   # (the third way once per shape, and not where a frame is a thousand feature frames)
            continue
        state = Slots(5, K)
        pres = {3: kit.as_float(kit.source(K + 3 * H + 5, dtype, 11)), 1: kit.as_float(kit.source(K // 2 + 1, dtype, 12))}
        state.seed(3, pres[3], 0)
        state.seed(1, pres[1], 1)
        xs = [kit.source(1024 * f, dtype, 100 + 10 * way + s) for s, f in enumerate(counts)]
        slots = [4, 3, 1]
        outs = launch(lib, state, xs, slots, shape, basis, fb, False, row_extra, blocks, reverse)
        for s, pre in enumerate([np.zeros(0, np.float32), pres[3], pres[1]]):
            want = kit.rule(lib, np.concatenate([pre, kit.as_float(xs[s])]), K, H, P, basis, fb)[kit.count(len(pre), K, H, P):]
            assert len(want) > 0 or K == 1024
            kit.same_bits(outs[s], want, "%s, stream %d, way %d" % (shape, s, way))


@pytest.mark.parametrize("case", [((400, 160, 200, 201, 80), np.float32, None), ((32, 7, 31, 3, 1), np.int16, 2), ((1024, 1024, 0, 16, 128), np.float32, 0)],
                         ids=["whisper-f32-packed", "small-i16-planar", "long-f32-planar"])
def test_any_split_into_batches_gives_the_same_bits(lib, case):
    """the same stream as 3 frames, as 1 + 2 and as 1 + 1 + 1 — beside a second stream that is there in some of the batches only, and cut
    raggedly as a resampler's output is — gives the same bits concatenated, and they are the rule's over the whole stream"""
    shape, dtype, row_extra = case
    K, H, P, B, NM = shape
    basis, fb = kit.hostile_tables(K, B, NM)
    x = kit.source(3 * 1024, dtype, 42)
    other = kit.source(2 * 1024, dtype, 43)
    want = kit.rule(lib, kit.as_float(x), K, H, P, basis, fb)
    assert len(want) == kit.count(3 * 1024, K, H, P)
    for split in ([3072], [1024, 2048], [1024, 1024, 1024], [341, 342, 341, 1000, 1048]):
        state = Slots(3, K)
        got, at = [], 0
        for b, n in enumerate(split):
            part = x[at:at + n]
            xs, slots = ([other[:1024] if b == 0 else other[1024:], part], [0, 2]) if b in (0, 2) and len(split) > 1 else ([part], [2])
            got.append(launch(lib, state, xs, slots, shape, basis, fb, False, row_extra, 2 if b % 2 else None, b % 2)[-1])
            at += n
        kit.same_bits(np.concatenate(got), want, "split %s" % split)


@pytest.mark.parametrize("shape", [kit.SHAPES[1], kit.SHAPES[0]], ids=["whisper", "small"])
def test_log_output_is_log10_of_the_floored_mel(lib, shape):
    """with log: float32(np.log10 in float64 of max(the rule's mel, floor)) to 4 ulp — OpenCL's 3-ulp bound for log10, which the device
    library follows, plus the reference's own rounding; the hostile filterbank's negative sums sit on the floor"""
    K, H, P, B, NM = shape
    basis, fb = kit.hostile_tables(K, B, NM)
    state = Slots(2, K)
    pre = kit.as_float(kit.source(K + 17, np.float32, 5))
    state.seed(1, pre, 1)
    xs = [kit.source(2048, np.float32, 6), kit.source(1024, np.float32, 7)]
    outs = launch(lib, state, xs, [0, 1], shape, basis, fb, True, 2, 3, 1)
    floored = 0
    for s, p in enumerate([np.zeros(0, np.float32), pre]):
        mel = kit.rule(lib, np.concatenate([p, xs[s]]), K, H, P, basis, fb)[kit.count(len(p), K, H, P):]
        floored += int((mel < FLOOR).sum())
        assert outs[s].shape == mel.shape and (kit.ulps(outs[s], kit.log_reference(mel, FLOOR)) <= 4).all()
    assert floored > 0


def test_limits(lib):
    """the limits of include/aacgpu.h as the launch's host part checks them"""
    for good in ((32, 1, 0, 2, 1), (400, 160, 200, 402, 80), (1024, 1024, 1023, 1026, 128), (64, 64, 63, 66, 5)):
        assert lib.emu_features_check(*good) == 0, good
    for bad in ((28, 7, 0, 2, 1), (1028, 7, 0, 2, 1), (402, 160, 0, 2, 1), (400, 0, 0, 2, 1), (400, 401, 0, 2, 1), (400, 160, 400, 2, 1), (400, 160, 0, 0, 1),
                (400, 160, 0, 3, 1), (400, 160, 0, 1028, 1), (400, 160, 0, 402, 0), (400, 160, 0, 402, 129)):
        assert lib.emu_features_check(*bad) != 0, bad


def test_features_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: both element
    sizes, both layouts, linear and log, over heap blocks of exactly the buffers' sizes — the ragged output's and the history's
    included.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "features_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DFEATURES_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "features_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "features_emu: ok" in r.stdout, r.stdout + r.stderr
