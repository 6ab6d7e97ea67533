"""A resident batch's packed PCM resampled by L / M (aacg_pcm_resample, aac.js_amd/csrc/aacg_pcm_resample.h: resample_body) against the rule
of include/aacgpu.h in numpy float32 (resample_kit.resample_rule), bit for bit, with a poisoned guard on both sides of the destination and
of the history block: the kernel's source run lane by lane on CPU threads (tests/emu/resample_emu.cpp with tests/emu/devport_emu.h).

The rule: output m of a stream's channel is acc = h[p][0] * x[i], then acc = acc + h[p][t] * x[i - t] for t = 1 .. T-1, i = floor(m M / L),
p = (m M) mod L, x[j] = 0 for j < 0, every product and every sum rounded to float32, never fused; int16 in = the sample as float, out = acc
rounded to nearest even and saturated.  A stream in mid-phase is checked against the rule over a WHOLE stream — made-up earlier input of
a length congruent to its clock modulo M, then the batch's frames — so the kernel's clock modulo M and its history are what is tested."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import resample_kit as kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096            # poisoned bytes on either side of the destination and of the history
REC = np.dtype([(n, np.uint32) for n in ("frame_first", "frames", "out_first", "n_out", "n0", "slot", "parity", "fresh")])
TAPS = [4, 32, 64]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("resample_emu", ["tests/emu/resample_emu.cpp"], tmp_path_factory.mktemp("resample_emu"))
    L.emu_resample.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 2 + [C.c_uint32] * 7 + [C.c_int]
    L.emu_resample.restype = C.c_int
    L.emu_resample_check.argtypes = [C.c_uint32] * 3
    sizes = (C.c_uint32 * 3)()
    L.emu_resample_sizes(sizes)
    assert sizes[1] == REC.itemsize == 32 and sizes[2] == 64
    L.threads = int(sizes[0])
    return L


def guarded(n_bytes, fill):
    """n_bytes at a 16-byte aligned address inside a block with GUARD poisoned bytes on either side: (block, view)"""
    raw = np.full(GUARD + n_bytes + GUARD + 16, fill, np.uint8)
    off = (-(raw.ctypes.data + GUARD)) % 16
    block = raw[off:off + GUARD + n_bytes + GUARD]
    return block, block[GUARD:GUARD + n_bytes]


def guards_intact(block, n_bytes, fill):
    return (block[:GUARD] == fill).all() and (block[GUARD + n_bytes:] == fill).all()


def source(n, channels, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        x = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
        x[:3] = [[32767] * channels, [-32768] * channels, [-32767] * channels]
        return x
    return (rng.choice([-1.0, 1.0], (n, channels)) * np.exp2(rng.uniform(-20.0, 3.0, (n, channels)))).astype(np.float32)


class Slots:
    """the state the host keeps and the history block the device keeps, for `n` slots: clocks modulo M, parities, fresh flags"""

    def __init__(self, n, taps, channels, M):
        self.T, self.C, self.M, self.n = taps, channels, M, n
        self.bytes = n * 2 * (taps - 1) * channels * 4
        self.block, raw = guarded(self.bytes, 0x5A)
        self.hist = raw.view(np.float32).reshape(n, 2, taps - 1, channels)
        self.hist[:] = np.float32(-77.25)                # what nobody has written yet: any read of it shows
        self.n0, self.parity, self.fresh = [0] * n, [0] * n, [1] * n

    def seed(self, slot, pre):
        """the slot has consumed `pre` (N, C) already: the clock, and the last T - 1 samples in the buffer its next launch reads"""
        assert len(pre) >= self.T - 1
        self.n0[slot], self.fresh[slot] = len(pre) % self.M, 0
        self.hist[slot, self.parity[slot]] = pre[len(pre) - (self.T - 1):].astype(np.float32)


def launch(lib, state, xs, slots, L, M, table, row, blocks, reverse):
    """one emulated launch: stream s brings xs[s] (frames * 1024, C) for slot slots[s]; row: None packed, else the planar row's length.
    Returns each stream's output (n_out, C) — planar: the whole block (n_streams, C, row) as well — and advances `state`."""
    dtype, channels, T = xs[0].dtype, xs[0].shape[1], table.shape[1]
    rec = np.zeros(len(xs), REC)
    first = out_first = 0
    for s, (x, slot) in enumerate(zip(xs, slots)):
        frames = len(x) // 1024
        n = kit.n_out(state.n0[slot], state.n0[slot] + len(x), L, M)
        rec[s] = (first, frames, out_first, n, state.n0[slot], slot, state.parity[slot], state.fresh[slot])
        first, out_first = first + frames, out_first + n
    packed = np.concatenate(xs)
    src_block, src = guarded(packed.nbytes, 0)
    src.view(dtype)[:] = packed.reshape(-1)
    n_dst = (len(xs) * channels * row if row else out_first * channels) * xs[0].dtype.itemsize
    dst_block, dst = guarded(n_dst, 0xC3)
    tab_block, tab = guarded(table.nbytes, 0)
    tab.view(np.float32)[:] = table.reshape(-1)
    before = state.hist.copy()
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0 and tab.ctypes.data % 16 == 0
    blocks = first + 2 if blocks is None else blocks
    assert lib.emu_resample(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), first, tab.ctypes.data, state.hist.ctypes.data,
                            L, M, T, row or 0, channels, xs[0].dtype.itemsize, blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst, 0xC3), "a byte outside the destination was written"
    assert guards_intact(state.block, state.bytes, 0x5A), "a byte outside the history was written"
    assert (src.view(dtype) == packed.reshape(-1)).all()
    outs, whole = [], None
    if row:
        whole = dst.view(dtype).reshape(len(xs), channels, row).copy()
        for s in range(len(xs)):
            outs.append(whole[s, :, :rec[s]["n_out"]].T.copy())
            assert (whole[s, :, rec[s]["n_out"]:] == 0).all(), "the planar padding is not zeros"
    else:
        flat = dst.view(dtype).reshape(out_first, channels)
        for s in range(len(xs)):
            outs.append(flat[rec[s]["out_first"]:rec[s]["out_first"] + rec[s]["n_out"]].copy())
    # the history: the streams' new parity holds their last T - 1 inputs, everything else is as it was
    untouched = np.ones(state.hist.shape[:2], bool)
    for x, slot in zip(xs, slots):
        new = state.parity[slot] ^ 1
        tail = x[len(x) - (T - 1):].astype(np.float32)
        assert state.hist[slot, new].view(np.uint32).tolist() == tail.view(np.uint32).tolist(), "the new history is not the last T - 1 inputs"
        untouched[slot, new] = False
        state.n0[slot], state.parity[slot], state.fresh[slot] = (state.n0[slot] + len(x)) % M, new, 0
    assert (state.hist.view(np.uint32)[untouched] == before.view(np.uint32)[untouched]).all(), "the other parity's buffer or another slot's was written"
    return outs


def same_bits(got, want, what):
    view = np.uint32 if got.dtype == np.float32 else np.uint16
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = np.argwhere(np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view))
    assert wrong.size == 0, "%s: the kernel differs from the rule at %d of %d elements, first at (sample, channel) %s: %r against %r" % (
        what, len(wrong), got.size, wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])])


def taps_for(L, k):
    """the tap counts in turn, among those whose table fits (441 x 64 does not)"""
    fit = [t for t in TAPS if L * t <= 16384]
    return fit[k % len(fit)]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("channels", range(1, 9))
def test_resample_is_the_rule(lib, channels, dtype):
    """every C x element type with a hostile table, every ratio, the tap counts in turn: a fresh stream of 3 frames, a stream in
    mid-phase with 1 and one with 2 (clocks that are no multiple of M, histories that are not zero), packed and planar, with one
    workgroup (it walks every frame), four in reverse, and two more than there are frames"""
    seen = set()
    for k, (L, M) in enumerate(kit.RATIOS):
        T = taps_for(L, k + channels)
        seen.add(T)
        assert lib.emu_resample_check(L, M, T) == 0
        table = kit.hostile_table(L, T)
        assert (table < 0).any() and (np.abs(table) > 1).any()
        for way, (row_frames, blocks, reverse) in enumerate([(None, 1, 0), (True, 4, 1), (None, None, 0)]):
            state = Slots(5, T, channels, M)
            pres = {3: source(M * 70 + M // 2, channels, dtype, 11 * k + 1),
                    1: source(M * 64 + (M - 1), channels, dtype, 11 * k + 2)}
            for slot, pre in pres.items():
                state.seed(slot, pre)
            if M > 1:
                assert state.n0[3] != 0 and state.n0[1] != 0
            xs = [source(3 * 1024, channels, dtype, 100 * channels + k), source(1024, channels, dtype, 200 * channels + k), source(2048, channels, dtype, 300 * channels + k)]
            slots = [4, 3, 1]
            full = [xs[0], np.concatenate([pres[3], xs[1]]), np.concatenate([pres[1], xs[2]])]
            skip = [0, kit.ceil_div(len(pres[3]) * L, M), kit.ceil_div(len(pres[1]) * L, M)]
            row = None
            if row_frames:
                longest = max(kit.n_out(0, len(f), L, M) - s for f, s in zip(full, skip))
                row = (longest + 1023) // 1024 * 1024 + (1024 if way else 0)
            outs = launch(lib, state, xs, slots, L, M, table, row, blocks, reverse)
            for s in range(3):
                same_bits(outs[s], kit.resample_rule(full[s], L, M, table)[skip[s]:], "%d / %d, %d taps, stream %d, way %d" % (L, M, T, s, way))
    assert len(seen) >= 2


@pytest.mark.parametrize("taps", TAPS)
def test_every_tap_count_at_every_ratio(lib, taps):
    """stereo f32 and mono int16 at every ratio whose table fits, fresh and in mid-phase in one launch, one frame each"""
    for k, (L, M) in enumerate(kit.RATIOS):
        if L * taps > 16384:
            assert lib.emu_resample_check(L, M, taps) != 0
            continue
        for channels, dtype in ((2, np.float32), (1, np.int16)):
            table = kit.hostile_table(L, taps)
            state = Slots(2, taps, channels, M)
            pre = source(M * 64 + M // 3, channels, dtype, k)
            state.seed(1, pre)
            xs = [source(1024, channels, dtype, 7 + k), source(1024, channels, dtype, 9 + k)]
            outs = launch(lib, state, xs, [0, 1], L, M, table, None, 2, 1)
            same_bits(outs[0], kit.resample_rule(xs[0], L, M, table), "fresh")
            same_bits(outs[1], kit.resample_rule(np.concatenate([pre, xs[1]]), L, M, table)[kit.ceil_div(len(pre) * L, M):], "mid-phase")


@pytest.mark.parametrize("layout", ["packed", "planar"])
@pytest.mark.parametrize("case", [(np.float32, 2, 160, 441, 32), (np.int16, 3, 441, 160, 4), (np.float32, 1, 160, 147, 64), (np.int16, 6, 1, 3, 32), (np.float32, 5, 2, 1, 4)],
                         ids=["f32-c2-160/441", "i16-c3-441/160", "f32-c1-160/147", "i16-c6-1/3", "f32-c5-2/1"])
def test_any_split_into_batches_gives_the_same_bits(lib, case, layout):
    """six frames of a stream as one batch, as 2 + 1 + 3 and as six batches of one — beside a second stream that is there in some of the
    batches only — give the same bits concatenated, and they are the rule's over the six frames"""
    dtype, channels, L, M, T = case
    table = kit.hostile_table(L, T)
    x = source(6 * 1024, channels, dtype, 42)
    other = source(2 * 1024, channels, dtype, 43)
    want = kit.resample_rule(x, L, M, table)
    assert len(want) == kit.ceil_div(6 * 1024 * L, M)
    for split in ([6], [2, 1, 3], [1] * 6):
        state = Slots(3, T, channels, M)
        got, at = [], 0
        for b, frames in enumerate(split):
            part = x[at * 1024:(at + frames) * 1024]
            xs, slots = ([other[:1024] if b == 0 else other[1024:], part], [0, 2]) if b in (0, 2) and len(split) > 1 else ([part], [2])
            row = None
            if layout == "planar":
                row = (max(kit.n_out(state.n0[s], state.n0[s] + len(v), L, M) for v, s in zip(xs, slots)) + 1023) // 1024 * 1024
            got.append(launch(lib, state, xs, slots, L, M, table, row, 2 if b % 2 else None, b % 2)[-1])
            at += frames
        same_bits(np.concatenate(got), want, "split %s" % split)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_int16_rounds_halves_to_even_and_saturates(lib, channels):
    """rows of (0.5, 0.5, 0, 0) over small int16 samples: every sum is exact in float and an odd sum of two neighbours is an exact half,
    which goes to the even neighbour; rows of (1, 1, 1, 1) over samples at the ends of the range saturate both ways"""
    for L, M in ((1, 3), (2, 1)):
        rng = np.random.default_rng(3 + channels)
        x = rng.integers(-6, 7, (1024, channels)).astype(np.int16)
        half = np.tile(np.array([0.5, 0.5, 0, 0], np.float32), (L, 1))
        want = kit.resample_rule(x, L, M, half)
        exact = 0.5 * x.astype(np.float64)[:-1] + 0.5 * x.astype(np.float64)[1:]
        assert (np.abs(exact % 1.0 - 0.5) < 1e-12).sum() > 100, "exact halves"
        assert (want % 2 == 0)[np.abs(kit.resample_rule(x.astype(np.float32), L, M, half) % 1.0) == 0.5].all()
        same_bits(launch(lib, Slots(1, 4, channels, M), [x], [0], L, M, half, None, 1, 0)[0], want, "halves")
        x = rng.integers(-32768, 32768, (1024, channels)).astype(np.int16)
        x[100:110], x[200:210] = 32767, -32768
        ones = np.ones((L, 4), np.float32)
        want = kit.resample_rule(x, L, M, ones)
        assert (want == 32767).any() and (want == -32768).any()
        unclamped = kit.resample_rule(x.astype(np.float32), L, M, ones)
        assert unclamped.max() > 40000 and unclamped.min() < -40000, "sums beyond the int16 range in both directions"
        same_bits(launch(lib, Slots(1, 4, channels, M), [x], [0], L, M, ones, 1024 * (2 if L > M else 1), 2, 1)[0], want, "saturation")


def test_limits(lib):
    """the limits of include/aacgpu.h as the launch's host part checks them"""
    assert lib.emu_resample_check(160, 441, 32) == 0 and lib.emu_resample_check(1, 8, 4) == 0 and lib.emu_resample_check(8, 1, 64) == 0 and lib.emu_resample_check(256, 255, 64) == 0
    for bad in ((160, 441, 0), (160, 441, 6), (160, 441, 68), (1025, 1024, 4), (1024, 1025, 4), (0, 1, 4), (1, 0, 4), (441, 160, 64), (257, 256, 64), (1, 9, 4), (9, 1, 4)):
        assert lib.emu_resample_check(*bad) != 0, bad


def test_resample_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: 1, 2, 3 and 8
    channels, both element sizes, both layouts, over heap blocks of exactly the buffers' sizes — the ragged output's and the
    history's included.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "resample_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DRESAMPLE_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "resample_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "resample_emu: ok" in r.stdout, r.stdout + r.stderr
