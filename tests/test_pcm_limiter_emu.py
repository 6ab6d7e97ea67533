"""The gain and look-ahead limiter on a resident batch's PCM (aacg_pcm_limit, aac.js_amd/csrc/aacg_pcm_limit.h: limit_body) against the rule
of include/aacgpu.h in numpy float32 (limiter_kit), bit for bit — what leaves AND the state left behind — with poisoned guards around
the destination and the state block: the kernel's source run lane by lane on CPU threads (tests/emu/limiter_emu.cpp with
tests/emu/devport_emu.h and tests/emu/devport_limit_emu.h).

The rule, per block xk of 64 x C samples of a slot: p = max |xk|; tk = (G p > c) ? c / p : G; u = a0 + (r (G - a0)); a1 = min(min(th, tk),
u); d = a1 - a0; out[i] = (a0 + (d (i / 64))) xh[i]; xh = xk; a0 = a1; th = tk — every operation rounded to float32 on its own.  Inputs
are noise with bursts; every case asserts ON THE KIT'S RESULT that some block had tk < G and some tk = G, and, where the input is finite,
that |out| <= c (1 + 2^-21)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import limiter_kit as kit

F = np.float32
GUARD = 1024            # poisoned floats on either side of the destination and of the state
REC = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("slot", "<u4"), ("parity", "<u4"), ("fresh", "<u4"), ("gain", "<f4"), ("unused", "<u4", (2,))])
POISON = F(-77.25)
HEAD = 4
CEILING, RELEASE = F(0.3), F(0.0625)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("limiter_emu", ["tests/emu/limiter_emu.cpp"], tmp_path_factory.mktemp("limiter_emu"))
    L.emu_limit.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_float, C.c_float] + [C.c_uint32] * 3 + [C.c_int]
    L.emu_limit.restype = C.c_int
    sizes = (C.c_uint32 * 5)()
    L.emu_limit_sizes(sizes)
    assert list(sizes) == [256, 4, REC.itemsize, HEAD, kit.B] and REC.itemsize == 32
    return L


def guarded(n_floats):
    """n_floats at a 16-byte aligned address inside a block with GUARD poisoned floats on either side: (block, view)"""
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
    """what the host keeps for `n` slots — gains, parities, fresh flags —, the state block the device keeps, and the rule's own state"""

    def __init__(self, n, channels):
        self.C, self.n, self.SF = channels, n, HEAD + kit.B * channels
        self.block, raw = guarded(n * 2 * self.SF)
        self.state = raw.reshape(n, 2, self.SF)
        self.gain, self.parity, self.fresh = [F(1.0)] * n, [0] * n, [1] * n
        self.ref = [kit.State(channels) for _ in range(n)]

    def reset(self, slot):
        """aacg_pipeline_reset_stream: the held block and the nodes go, the gain stays"""
        self.fresh[slot], self.ref[slot] = 1, kit.State(self.C)

    def engaged(self):
        under, at = zip(*[r.engaged() for r in self.ref])
        return sum(under), sum(at)


def launch(lib, S, xs, slots, c=CEILING, r=RELEASE, blocks=None, reverse=0, check=True):
    """one emulated launch: stream s brings xs[s] (frames * 1024, C) for slot slots[s].  Returns what leaves per stream, compares it and
    the state left behind with the rule's, bit for bit, and advances S."""
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
    before = S.state.copy()
    groups = -(-len(xs) // 4)
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0
    assert lib.emu_limit(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), S.state.ctypes.data, c, r,
                         channels, dtype.itemsize, groups + 1 if blocks is None else blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst), "an element outside the destination was written"
    assert guards_intact(S.block, S.state.size), "a float outside the state was written"
    assert (src.view(dtype) == packed.reshape(-1)).all() or dtype == F            # (a NaN in the source compares unequal to itself)
    flat = dst.view(dtype).reshape(len(packed), channels)
    outs = [flat[1024 * q["frame_first"]:1024 * (q["frame_first"] + q["frames"])].copy() for q in rec]
    untouched = np.ones(S.state.shape, bool)
    untouched[:, :, 2:HEAD] = False                                               # (the two unused floats are nobody's)
    for s, (x, slot) in enumerate(zip(xs, slots)):
        new = S.parity[slot] ^ 1
        want = kit.rule(x, S.gain[slot], c, r, S.ref[slot])
        if check:
            same_bits(outs[s], want, "stream %d, what leaves" % s)
            left, ref = S.state[slot, new], S.ref[slot].floats()
            same_bits(left[:2], ref[:2], "stream %d, a0 and th left behind" % s)
            same_bits(left[HEAD:], ref[HEAD:], "stream %d, the block left behind" % s)
        untouched[slot, new] = False
        S.parity[slot], S.fresh[slot] = new, 0
    assert (S.state.view(np.uint32)[untouched] == before.view(np.uint32)[untouched]).all(), "the other parity's state or another slot's was written"
    return outs


def within_the_bound(outs, c):
    lim = float(c) * (1.0 + 2.0 ** -21)
    for o in outs:
        v = o.astype(np.float64) / (32768.0 if o.dtype == np.int16 else 1.0)
        assert np.abs(v).max() <= lim, (np.abs(v).max(), lim)


def test_the_kit_agrees_with_itself():
    """the rule over a whole history at once and block after block from a carried state, any split, a gain per batch: the same bits"""
    for dtype, channels in ((F, 2), (np.int16, 3), (F, 1)):
        x = kit.bursts(6 * 1024, channels, dtype, 5 + channels)
        gains = [F(1.0), F(3.5), F(0.25), F(0.0), F(2.0), F(2.0)]                 # per frame
        want, t, G = kit.whole(x, np.repeat(np.array(gains, F), 16), CEILING, RELEASE)
        assert (t < G).any() and (t == G).any()
        st = kit.State(channels)                                                  # (a call has one gain: a frame per call where it changes)
        got = [kit.rule(x[f * 1024:(f + 1) * 1024], gains[f], CEILING, RELEASE, st) for f in range(6)]
        same_bits(np.concatenate(got), want, "a gain per frame")
        assert st.engaged() == (int((t < G).sum()), int((t == G).sum()))
        want = kit.whole(x, 2.0, CEILING, RELEASE)[0]
        for split in ([6], [1, 2, 3], [4, 2]):
            st, got, at = kit.State(channels), [], 0
            for frames in split:
                got.append(kit.rule(x[at * 1024:(at + frames) * 1024], 2.0, CEILING, RELEASE, st))
                at += frames
            same_bits(np.concatenate(got), want, "split %s" % split)


@pytest.mark.parametrize("dtype", [F, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
def test_limiter_is_the_rule(lib, channels, dtype):
    """a ragged batch of five streams of 1..3 frames on fresh slots (two workgroups of four waves, and one more that finds nothing), then
    a second one of another shape on the other parity with gains changed up, down and to 0, by one workgroup that takes both groups"""
    dtype = np.dtype(dtype)
    S = Slots(7, channels)
    slots = [6, 4, 5, 1, 2]                                                       # not in order, not from 0
    for slot, g in zip(slots, (1.0, 4.0, 0.5, 1.0, 2.5)):
        S.gain[slot] = F(g)
    outs = []
    for b, frames_of in enumerate(([1, 3, 2, 1, 2], [2, 1, 3, 2, 1])):
        xs = [kit.bursts(f * 1024, channels, dtype, 100 * b + 10 * s + channels) for s, f in enumerate(frames_of)]
        outs += launch(lib, S, xs, slots, blocks=None if b == 0 else 1, reverse=b)
        S.gain[6], S.gain[4], S.gain[5] = F(3.0), F(0.75), F(0.0)                 # up, down, to nothing
    under, at = S.engaged()
    assert under > 0 and at > 0, "the kit never limited, or always: the case does not test what it is for"
    within_the_bound(outs, CEILING)
    assert all(p == 0 for p in S.parity[:1] + S.parity[3:4]) and all(S.parity[slot] == 0 and not S.fresh[slot] for slot in slots)


@pytest.mark.parametrize("dtype", [F, np.int16], ids=["f32", "i16"])
def test_any_split_into_batches_gives_the_same_bits(lib, dtype):
    """the same two streams in two splits, beside a third that is there in some batches only: what leaves, concatenated, is the rule's
    over the whole history, and the state left behind is the same"""
    dtype, channels = np.dtype(dtype), 2
    xa, xb, other = kit.bursts(5 * 1024, channels, dtype, 42), kit.bursts(5 * 1024, channels, dtype, 43), kit.bursts(1024, channels, dtype, 44)
    want = [kit.whole(x, g, CEILING, RELEASE) for x, g in ((xa, 1.0), (xb, 4.0))]
    for w, t, G in want:
        assert (t < G).any() and (t == G).any()
    final = []
    for split in ([5], [2, 3], [1, 1, 2, 1]):
        S, got, at = Slots(4, channels), ([], []), 0
        S.gain[1], S.gain[3] = F(1.0), F(4.0)
        for b, frames in enumerate(split):
            xs, slots = [xa[at * 1024:(at + frames) * 1024], xb[at * 1024:(at + frames) * 1024]], [1, 3]
            if b % 2 == 0:
                xs, slots = [xs[0], other, xs[1]], [1, 0, 3]
            outs = launch(lib, S, xs, slots, reverse=b % 2, check=False)
            got[0].append(outs[0])
            got[1].append(outs[-1])
            at += frames
        for k in (0, 1):
            same_bits(np.concatenate(got[k]), want[k][0], "split %s, stream %d" % (split, k))
        final.append(np.concatenate([S.state[slot, S.parity[slot]][[0, 1] + list(range(HEAD, S.SF))] for slot in (1, 3)]))
        within_the_bound(got[0] + got[1], CEILING)
    for f in final[1:]:
        same_bits(f, final[0], "the state left behind by another split")


def test_a_reset_and_gains_between_batches(lib):
    """a slot that is reset starts from a block of zeros and a0 = th = G as G stands THEN, while its neighbour goes on; a gain that falls
    reaches the output within one block as a ramp, a gain that rises approaches at the rate r"""
    channels = 2
    S = Slots(2, channels)
    x = [kit.bursts(2048, channels, F, 1), kit.bursts(1024, channels, F, 2), kit.bursts(1024, channels, F, 3), kit.bursts(1024, channels, F, 4)]
    launch(lib, S, [x[0], x[1]], [0, 1])
    S.reset(0)
    S.gain[0], S.gain[1] = F(0.125), F(0.25)
    outs = launch(lib, S, [x[2], x[3]], [0, 1])
    same_bits(outs[0], kit.whole(x[2], 0.125, CEILING, RELEASE)[0], "the reset slot against a new stream at the new gain")
    assert (outs[0][:64] == 0).all() and S.gain[0] == F(0.125)
    # the neighbour's fall from 1 to 0.25: its first block leaves at gains that ramp from the old node down to at most 0.25
    whole, t, G = kit.whole(np.concatenate([x[1], x[3]]), np.repeat(np.array([1.0, 0.25], F), 16), CEILING, RELEASE)
    same_bits(outs[1], whole[1024:], "the neighbour across the change of gain")
    held = x[1][-64:]
    k = np.abs(outs[1][:64, 0].astype(np.float64) / np.where(held[:, 0] == 0, 1, held[:, 0]).astype(np.float64))
    node = abs(float(outs[1][64, 0]) / float(x[3][0, 0]))                              # the gain at the next block's start
    assert node <= 0.25 * (1 + 2.0 ** -20) and k[0] > node and (np.diff(k) <= 1e-6).all()
    under, at = S.engaged()
    assert under > 0 and at > 0
    # ... and a rise from 0.25 to 4 on quiet input: the node gains approach 4 at r per block, never above it
    S.gain[1] = F(4.0)
    quiet = np.full((2048, channels), F(0.001))
    outs = launch(lib, S, [quiet], [1])
    g = outs[0][64::64, 0].astype(np.float64) / 0.001                                 # the node gains at blocks' starts
    assert (np.diff(g) > 0).all() and g[-1] < 4.0 and abs((4.0 - g[11]) / (4.0 - g[10]) - (1 - float(RELEASE))) < 1e-3


def test_zero_blocks_and_a_product_that_rounds_to_the_ceiling(lib):
    """a block of zeros (p = 0: no division); G = 0; and a block whose G p is not c exactly (f32: it lies above) but ROUNDS to c: not above it, so tk = G"""
    for dtype in (F, np.int16):
        dtype, channels = np.dtype(dtype), 2
        G = F(1.0 + 2.0 ** -23)
        p = F(1.0 + 2.0 ** -23) if dtype == F else F(32767.0 / 32768.0)
        c = G * p
        assert type(c) is F and float(G) * float(p) != float(c), "the product is not exact: it ROUNDS to c"
        assert dtype != F or float(G) * float(p) > float(c), "f32: the exact product lies above c, the rounded one does not"
        x = kit.bursts(3 * 1024, channels, dtype, 77, level=0.2, burst=0.7)
        x[128:256] = 0                                                                 # two blocks of zeros
        x[320, 1] = p if dtype == F else 32767                                         # block 5: its peak is p
        x[3 * 1024 - 64:] = 0
        S = Slots(3, channels)
        S.gain[0], S.gain[1], S.gain[2] = G, F(0.0), F(8.0)
        loud = kit.bursts(1024, channels, dtype, 78, level=0.01, burst=0.9)
        outs = launch(lib, S, [x, x, loud], [0, 1, 2], c=c)
        t = [tk for tk, _ in S.ref[0].targets]
        assert t[2] == t[3] == float(G) and t[5] == float(G), "zeros and the rounded product leave the target at G"
        assert all(tk == 0.0 for tk, _ in S.ref[1].targets) and not outs[1].astype(np.float64).any()
        under, at = S.engaged()
        assert under > 0 and at > 0
        within_the_bound(outs, c)


def test_a_nan_sample_is_ignored_by_the_peak(lib):
    """f32: a NaN among the samples does not reach the block's peak — the gains are those of the same input with a zero in its place —
    and comes out as a NaN at its own position only, one block later"""
    channels = 3
    x = kit.bursts(2048, channels, F, 9)
    clean = x.copy()
    x[700, 1] = np.nan
    clean[700, 1] = 0.0
    S, T = Slots(1, channels), Slots(1, channels)
    S.gain[0] = T.gain[0] = F(2.0)
    got, ref = launch(lib, S, [x], [0])[0], launch(lib, T, [clean], [0])[0]
    where = np.argwhere(np.isnan(got))
    assert where.tolist() == [[764, 1]]
    got[764, 1] = ref[764, 1]
    same_bits(got, ref, "everything but the NaN")
    assert [tk for tk, _ in S.ref[0].targets] == [tk for tk, _ in T.ref[0].targets]
    under, at = S.engaged()
    assert under > 0 and at > 0
    within_the_bound([ref], CEILING)
