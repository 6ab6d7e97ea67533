"""The limiter with a true-peak detector on a resident batch's PCM (aacg_pcm_limit_tp_detect and aacg_pcm_limit_tp,
aac.js_amd/csrc/aacg_pcm_limit_tp.h) against the rule of include/aacgpu.h (aacg_pipeline_set_limiter_true_peak) in numpy float32
(limiter_tp_kit), bit for bit — what leaves AND both sides of the state left behind, the plain limiter's block and the history — with
poisoned guards around the destination, the two state blocks and the scratch: the kernels' source run lane by lane on CPU threads
(tests/emu/limiter_tp_emu.cpp with tests/emu/devport_emu.h and tests/emu/devport_limit_emu.h).

Inputs are noise with bursts above full scale (limiter_kit.bursts, burst 1.4); every case asserts ON THE KIT'S RESULT that some block
had tk < G and some tk = G, and, where the input is finite, that |out| <= c (1 + 2^-21).

The property the stage is for, on the kit alone: a full-scale sine at fs / 4 with 45 degrees of phase and c = 10^(-1/20) leaves the plain
limiter with a true peak of at least 1.09 c (4 x 24 table) and this one with at most c (1 + 2^-20)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import limiter_kit
import limiter_tp_kit as kit
import truepeak_kit

F = np.float32
GUARD = 1024
REC = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("slot", "<u4"), ("parity", "<u4"), ("fresh", "<u4"), ("gain", "<f4"), ("unused", "<u4", (2,))])
POISON = F(-77.25)
HEAD = 4
RELEASE = F(0.0625)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table_of(name):
    """(1, 4) and (8, 64): the limits' corners; (4, 24): the default; mixed: not a filter, every rounding shows"""
    if name == "mixed":
        return truepeak_kit.mixed_table(3, 12)
    L, T = name
    return truepeak_kit.design(L, T)


def ceiling_of(table):
    """between the quiet noise's detector values and the bursts': 0.3 for a filter whose rows sum to 1, more for a table with gain"""
    return F(0.3 * max(1.0, float(np.abs(np.asarray(table, np.float64)).sum(axis=1).max()) / 2.0))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("limiter_tp_emu", ["tests/emu/limiter_tp_emu.cpp"], tmp_path_factory.mktemp("limiter_tp_emu"))
    L.emu_limit_tp.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_float, C.c_float] + [C.c_uint32] * 4 + [C.c_int]
    L.emu_limit_tp.restype = C.c_int
    sizes = (C.c_uint32 * 16)()
    L.emu_limit_tp_sizes(sizes)
    assert list(sizes)[:7] == [256, 256, 4, REC.itemsize, HEAD, kit.B, 16] and REC.itemsize == 32
    assert list(sizes)[7:] == [(64 + 1024) * 4 * c + 4096 + 2048 for c in range(9)]
    return L


def guarded(n_floats):
    raw = np.full(GUARD + n_floats + GUARD + 4, POISON, F)
    off = ((-(raw.ctypes.data + 4 * GUARD)) % 16) // 4
    block = raw[off:off + GUARD + n_floats + GUARD]
    return block, block[GUARD:GUARD + n_floats]


def guards_intact(block, n_floats):
    return (block[:GUARD] == POISON).all() and (block[GUARD + n_floats:] == POISON).all()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = np.uint32 if got.dtype == F else np.uint16
    assert np.array_equal(got.view(view), want.view(view)), "%s: the kernel differs from the rule at %d of %d values, first at %s" % (
        what, int((got.view(view) != want.view(view)).sum()), got.size, np.argwhere(got.view(view) != want.view(view))[0])


class Slots:
    """what the host keeps for `n` slots — gains, parities, fresh flags —, the two state blocks the device keeps, and the rule's own state"""

    def __init__(self, n, channels, table):
        self.C, self.n, self.table = channels, n, np.ascontiguousarray(table, F)
        self.T = self.table.shape[1]
        self.SF, self.H = HEAD + kit.B * channels, (self.T - 1) * channels
        self.block, raw = guarded(n * 2 * self.SF)
        self.state = raw.reshape(n, 2, self.SF)
        self.hblock, raw = guarded(n * 2 * self.H)
        self.hist = raw.reshape(n, 2, self.H)
        self.gain, self.parity, self.fresh = [F(1.0)] * n, [0] * n, [1] * n
        self.ref = [kit.State(channels, self.T) for _ in range(n)]

    def reset(self, slot):
        self.fresh[slot], self.ref[slot] = 1, kit.State(self.C, self.T)

    def engaged(self):
        under, at = zip(*[r.engaged() for r in self.ref])
        return sum(under), sum(at)


def launch(lib, S, xs, slots, c, r=RELEASE, detect_blocks=None, walk_blocks=None, reverse=0, check=True):
    """one emulated pair of launches: stream s brings xs[s] (frames * 1024, C) for slot slots[s].  Returns what leaves per stream,
    compares it, the scratch and both states left behind with the rule's, bit for bit, and advances S."""
    dtype, channels = xs[0].dtype, xs[0].shape[1]
    rec = np.zeros(len(xs), REC)
    first = 0
    for s, (x, slot) in enumerate(zip(xs, slots)):
        rec[s] = (first, len(x) // 1024, slot, S.parity[slot], S.fresh[slot], S.gain[slot], (0, 0))
        first += len(x) // 1024
    packed = np.concatenate(xs)
    raw = np.zeros(packed.nbytes + 16, np.uint8)
    src = raw[(-raw.ctypes.data) % 16:][:packed.nbytes]
    src.view(dtype)[:] = packed.reshape(-1)
    n_dst = packed.nbytes // 4
    dst_block, dst = guarded(n_dst)
    peak_block, peak = guarded(first * 16)
    tab_block, tab = guarded(S.table.size)
    tab[:] = S.table.reshape(-1)
    before, hbefore = S.state.copy(), S.hist.copy()
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0 and tab.ctypes.data % 16 == 0
    assert lib.emu_limit_tp(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), S.state.ctypes.data, S.hist.ctypes.data, peak.ctypes.data, tab.ctypes.data,
                            S.table.shape[0], S.T, c, r, channels, dtype.itemsize, first + 1 if detect_blocks is None else detect_blocks,
                            -(-len(xs) // 4) + 1 if walk_blocks is None else walk_blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst), "an element outside the destination was written"
    assert guards_intact(S.block, S.state.size) and guards_intact(S.hblock, S.hist.size), "a float outside the state was written"
    assert guards_intact(peak_block, first * 16), "a float outside the scratch was written"
    assert guards_intact(tab_block, S.table.size) and (tab.view(np.uint32) == S.table.reshape(-1).view(np.uint32)).all()
    flat = dst.view(dtype).reshape(len(packed), channels)
    outs = [flat[1024 * q["frame_first"]:1024 * (q["frame_first"] + q["frames"])].copy() for q in rec]
    untouched, huntouched = np.ones(S.state.shape, bool), np.ones(S.hist.shape, bool)
    untouched[:, :, 2:HEAD] = False
    for s, (x, slot) in enumerate(zip(xs, slots)):
        new = S.parity[slot] ^ 1
        seen = len(S.ref[slot].targets)
        want = kit.rule(x, S.gain[slot], c, r, S.table, S.ref[slot])
        if check:
            same_bits(outs[s], want, "stream %d, what leaves" % s)
            p = np.array([t[2] for t in S.ref[slot].targets[seen:]], F)
            same_bits(peak[16 * rec[s]["frame_first"]:16 * (rec[s]["frame_first"] + rec[s]["frames"])], p, "stream %d, the detector's float per block" % s)
            left, ref = S.state[slot, new], S.ref[slot].floats()
            same_bits(left[:2], ref[:2], "stream %d, a0 and th left behind" % s)
            same_bits(left[HEAD:], ref[HEAD:], "stream %d, the block left behind" % s)
            same_bits(S.hist[slot, new], S.ref[slot].history(), "stream %d, the history left behind" % s)
        untouched[slot, new] = huntouched[slot, new] = False
        S.parity[slot], S.fresh[slot] = new, 0
    assert (S.state.view(np.uint32)[untouched] == before.view(np.uint32)[untouched]).all(), "the other parity's state or another slot's was written"
    assert (S.hist.view(np.uint32)[huntouched] == hbefore.view(np.uint32)[huntouched]).all(), "the other parity's history or another slot's was written"
    return outs


def within_the_bound(outs, c):
    lim = float(c) * (1.0 + 2.0 ** -21)
    for o in outs:
        v = o.astype(np.float64) / (32768.0 if o.dtype == np.int16 else 1.0)
        assert np.abs(v).max() <= lim, (np.abs(v).max(), lim)


def test_the_kit_agrees_with_itself():
    """the rule over a whole history at once and block after block from a carried state, any split, a gain per batch, every table: the
    same bits, the same detector values"""
    for dtype, channels, name in ((F, 2, (4, 24)), (np.int16, 3, (1, 4)), (F, 1, (8, 64)), (F, 2, "mixed")):
        table = table_of(name)
        c = ceiling_of(table)
        x = kit.bursts(6 * 1024, channels, dtype, 5 + channels, burst=1.4)
        gains = [F(1.0), F(3.5), F(0.25), F(0.0), F(2.0), F(2.0)]                 # per frame
        want, t, G, p = kit.whole(x, np.repeat(np.array(gains, F), 16), c, RELEASE, table)
        assert (t < G).any() and (t == G).any()
        st = kit.State(channels, table.shape[1])
        got = [kit.rule(x[f * 1024:(f + 1) * 1024], gains[f], c, RELEASE, table, st) for f in range(6)]
        same_bits(np.concatenate(got), want, "a gain per frame")
        same_bits(np.array([q[2] for q in st.targets], F), p, "the detector's values")
        assert st.engaged() == (int((t < G).sum()), int((t == G).sum()))
        want = kit.whole(x, 2.0, c, RELEASE, table)[0]
        for split in ([6], [1, 2, 3], [4, 2]):
            st, got, at = kit.State(channels, table.shape[1]), [], 0
            for frames in split:
                got.append(kit.rule(x[at * 1024:(at + frames) * 1024], 2.0, c, RELEASE, table, st))
                at += frames
            same_bits(np.concatenate(got), want, "split %s" % split)
    # a detector that is the delayed path itself (acc = x[j - 2] exactly, so pt = ps) is the plain limiter, T / 2 later: one phase (0, 0, 1, 0)
    x = kit.bursts(3 * 1024, 2, F, 3, burst=1.4)
    ident = np.array([[0, 0, 1, 0]], F)
    got = kit.whole(x, 1.5, 0.3, RELEASE, ident)[0]
    plain = limiter_kit.whole(np.concatenate([np.zeros((2, 2), F), x[:-2]]), 1.5, 0.3, RELEASE)[0]
    same_bits(got, plain, "the identity table against the plain rule on the delayed input")


@pytest.mark.parametrize("name", [(1, 4), (4, 24), (8, 64), "mixed"], ids=["1x4", "4x24", "8x64", "mixed"])
@pytest.mark.parametrize("channels,dtype", [(1, F), (2, F), (6, F), (2, np.int16)], ids=["c1-f32", "c2-f32", "c6-f32", "c2-i16"])
def test_limiter_tp_is_the_rule(lib, channels, dtype, name):
    """a ragged batch of five streams of 1..3 frames on fresh slots (two walk workgroups of four waves and one more that finds nothing, a
    detector workgroup per frame and one more), then a second one of another shape on the other parity — every stream's history crosses
    the cut — with gains changed up, down and to 0, by one walk workgroup that takes both groups and three detector workgroups"""
    dtype, table = np.dtype(dtype), table_of(name)
    c = ceiling_of(table)
    S = Slots(7, channels, table)
    slots = [6, 4, 5, 1, 2]
    for slot, g in zip(slots, (1.0, 4.0, 0.5, 1.0, 2.5)):
        S.gain[slot] = F(g)
    outs = []
    for b, frames_of in enumerate(([1, 3, 2, 1, 2], [2, 1, 3, 2, 1])):
        xs = [kit.bursts(f * 1024, channels, dtype, 100 * b + 10 * s + channels, burst=1.4) for s, f in enumerate(frames_of)]
        outs += launch(lib, S, xs, slots, c, detect_blocks=None if b == 0 else 3, walk_blocks=None if b == 0 else 1, reverse=b)
        S.gain[6], S.gain[4], S.gain[5] = F(3.0), F(0.75), F(0.0)
    under, at = S.engaged()
    assert under > 0 and at > 0, "the kit never limited, or always: the case does not test what it is for"
    within_the_bound(outs, c)
    assert all(S.parity[slot] == 0 and not S.fresh[slot] for slot in slots)


@pytest.mark.parametrize("dtype", [F, np.int16], ids=["f32", "i16"])
def test_any_split_into_batches_gives_the_same_bits(lib, dtype):
    """the same two streams in three splits, beside a third that is there in some batches only: what leaves, concatenated, is the rule's
    over the whole history, and both states left behind are the same"""
    dtype, channels, table = np.dtype(dtype), 2, table_of((4, 24))
    c = ceiling_of(table)
    xa, xb, other = (kit.bursts(n * 1024, channels, dtype, seed, burst=1.4) for n, seed in ((5, 42), (5, 43), (1, 44)))
    want = [kit.whole(x, g, c, RELEASE, table) for x, g in ((xa, 1.0), (xb, 4.0))]
    for w, t, G, p in want:
        assert (t < G).any() and (t == G).any()
    final = []
    for split in ([5], [2, 3], [1, 1, 2, 1]):
        S, got, at = Slots(4, channels, table), ([], []), 0
        S.gain[1], S.gain[3] = F(1.0), F(4.0)
        for b, frames in enumerate(split):
            xs, slots = [xa[at * 1024:(at + frames) * 1024], xb[at * 1024:(at + frames) * 1024]], [1, 3]
            if b % 2 == 0:
                xs, slots = [xs[0], other, xs[1]], [1, 0, 3]
            outs = launch(lib, S, xs, slots, c, reverse=b % 2, check=False)
            got[0].append(outs[0])
            got[1].append(outs[-1])
            at += frames
        for k in (0, 1):
            same_bits(np.concatenate(got[k]), want[k][0], "split %s, stream %d" % (split, k))
        final.append(np.concatenate([np.concatenate([S.state[slot, S.parity[slot]][[0, 1] + list(range(HEAD, S.SF))], S.hist[slot, S.parity[slot]]]) for slot in (1, 3)]))
        within_the_bound(got[0] + got[1], c)
    for f in final[1:]:
        same_bits(f, final[0], "the state left behind by another split")


def test_a_reset_a_gain_between_batches_and_a_nan(lib):
    """a slot that is reset starts from zeros — block and history — and a0 = th = G as G stands THEN, while its neighbour goes on across a
    change of gain; a NaN among the samples reaches neither ps nor pt and comes out at its own position only, 64 + T / 2 later"""
    channels, table = 2, table_of((4, 24))
    c, late = ceiling_of(table), kit.delay(table_of((4, 24)))
    S = Slots(2, channels, table)
    x = [kit.bursts(n, channels, F, seed, burst=1.4) for n, seed in ((2048, 1), (1024, 2), (1024, 3), (1024, 4))]
    launch(lib, S, [x[0], x[1]], [0, 1], c)
    S.reset(0)
    S.gain[0], S.gain[1] = F(0.125), F(0.25)
    outs = launch(lib, S, [x[2], x[3]], [0, 1], c)
    same_bits(outs[0], kit.whole(x[2], 0.125, c, RELEASE, table)[0], "the reset slot against a new stream at the new gain")
    assert (outs[0][:late] == 0).all()
    whole = kit.whole(np.concatenate([x[1], x[3]]), np.repeat(np.array([1.0, 0.25], F), 16), c, RELEASE, table)[0]
    same_bits(outs[1], whole[1024:], "the neighbour across the change of gain")
    under, at = S.engaged()
    assert under > 0 and at > 0
    # the NaN
    y = kit.bursts(2048, 3, F, 9, burst=1.4)
    clean = y.copy()
    y[700, 1] = np.nan
    clean[700, 1] = 0.0
    A, Z = Slots(1, 3, table), Slots(1, 3, table)
    A.gain[0] = Z.gain[0] = F(2.0)
    got, ref = launch(lib, A, [y], [0], c)[0], launch(lib, Z, [clean], [0], c)[0]
    assert np.argwhere(np.isnan(got)).tolist() == [[700 + late, 1]]
    # (the NaN's T products are ignored where the clean input has h x 0 among finite terms: the detector may read lower around it, never a NaN)
    assert not np.isnan([t[2] for t in A.ref[0].targets]).any()
    within_the_bound([ref], c)


def test_the_true_peak_ceiling_on_the_quarter_rate_sine():
    """the kit alone: the fs / 4 sine at 45 degrees, samples 0.7071, true peak 1.  c = 10^(-1/20), G = 1: the plain limiter never engages
    and delivers >= 1.09 c; this one delivers <= c (1 + 2^-20), read with the same 4 x 24 table over the samples from 2048 on"""
    table = truepeak_kit.design(4, 24)
    c = F(10.0 ** (-1.0 / 20.0))
    x = kit.sine_quarter(8192)
    plain = limiter_kit.whole(x, 1.0, c, RELEASE)[0]
    got = kit.whole(x, 1.0, c, RELEASE, table)[0]
    tp_plain, tp = kit.true_peak(plain, table, 2048), kit.true_peak(got, table, 2048)
    print("quarter-rate sine: plain %.6f c, with the detector %.8f c" % (tp_plain / float(c), tp / float(c)))
    assert tp_plain >= 1.09 * float(c)
    assert tp <= float(c) * (1.0 + 2.0 ** -20)


def test_the_bound_under_a_moving_gain_is_measured_not_gated():
    """the kit alone: while the gain moves inside the filter's window the true-peak bound is not exact.  The figures are printed for
    DESIGN.md (section 7a has them as measured: bursts 1.0017 c, sweep 1.00003 c with the 4 x 24 table; 1.061 c and 1.040 c re-read with
    8 x 48) and only their direction is asserted: the detector never delivers more than the plain limiter"""
    t4, t8 = truepeak_kit.design(4, 24), truepeak_kit.design(8, 48)
    c = F(10.0 ** (-1.0 / 20.0))
    inputs = [("bursts seed %d" % seed, kit.bursts(16384, 2, F, seed, burst=1.4)) for seed in range(6)] + [("stepped sweep", kit.stepped_sweep(16384))]
    for name, x in inputs:
        plain, got = limiter_kit.whole(x, 1.0, c, RELEASE)[0], kit.whole(x, 1.0, c, RELEASE, t4)[0]
        fig = [kit.true_peak(y, t, 2048) / float(c) for y in (got, plain) for t in (t4, t8)]
        print("%s: %.6f c (4 x 24), %.6f c (8 x 48); plain %.4f c, %.4f c" % ((name,) + tuple(fig)))
        assert fig[0] <= fig[2] and fig[1] <= fig[3]


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """the emulator driver as a stand-alone program over exactly sized heap blocks, built with -fsanitize=address,undefined (CPU only)"""
    exe = str(tmp_path / "limiter_tp_emu_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DAACG_EMU_BUILD",
                    "-DLIMITER_TP_EMU_MAIN", "-I", os.path.join(ROOT, "tests", "emu"), "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                    "-o", exe, os.path.join(ROOT, "tests", "emu", "limiter_tp_emu.cpp")], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0 and "limiter_tp_emu: ok" in done.stdout, done.stdout + done.stderr
