"""The true-peak stage on a resident batch's transform PCM (aacg_pcm_truepeak, aac.js_amd/csrc/aacg_pcm_truepeak.h: truepeak_body) against
the rule of include/aacgpu.h in numpy float32 (truepeak_kit), bit for bit — the records AND the state left behind — with poisoned guards
around the record buffer and the state block: the kernel's source run lane by lane on CPU threads (tests/emu/truepeak_emu.cpp with
tests/emu/devport_emu.h).

The rule: acc = h[p][0] x[i], then acc = acc + (h[p][t] x[i - t]) for t = 1 .. T-1, every product and every sum rounded to float32 on its
own; a hop's record is the largest |acc| over its samples and all phases, a NaN if any acc is one.  Then what the number means: sines
whose samples miss their crests read -6.02 dBTP within EBU Tech 3341's tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aacgpu
import emu_lib
import loudness_kit
import truepeak_kit as kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 1024            # poisoned floats on either side of the records and of the state
REC = np.dtype([(n, np.uint32) for n in ("frame_first", "frames", "out_first", "n_out", "n0", "slot", "parity", "fresh")])
POISON = np.float32(-77.25)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("truepeak_emu", ["tests/emu/truepeak_emu.cpp"], tmp_path_factory.mktemp("truepeak_emu"))
    L.emu_truepeak.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_int]
    L.emu_truepeak.restype = C.c_int
    sizes = (C.c_uint32 * 11)()
    L.emu_truepeak_sizes(sizes)
    assert sizes[0] == 256 and sizes[1] == REC.itemsize == 32
    assert [sizes[2 + c] for c in range(9)] == [8448 * c + 2048 for c in range(9)]
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
    """what the host keeps for `n` slots — the meter's clocks, parities, fresh flags —, the state block the device keeps (zeros when the
    stage is set), and the rule's own state"""

    def __init__(self, n, channels, taps):
        self.C, self.T, self.n = channels, taps, n
        self.block, raw = guarded(n * 2 * taps * channels)
        raw[:] = 0.0
        self.state = raw.reshape(n, 2, taps * channels)
        self.N, self.parity, self.fresh = [0] * n, [0] * n, [1] * n
        self.ref = [kit.State(channels, taps) for _ in range(n)]
        # what the kit's own results showed on the way: a hop that held a frame's edge, one that held a batch's, a stream that emitted nothing
        self.straddled_frame = self.straddled_batch = self.emitted_nothing = False

    def reset(self, slot):
        self.N[slot], self.fresh[slot], self.ref[slot] = 0, 1, kit.State(self.C, self.T)


def aligned_table(table):
    t = np.ascontiguousarray(table, np.float32)
    raw = np.zeros(t.size + 4, np.float32)
    v = raw[((-raw.ctypes.data) % 16) // 4:][:t.size]
    v[:] = t.reshape(-1)
    return v


def launch(lib, S, xs, slots, hop, table, blocks=None, reverse=0, check=True):
    """one emulated launch: stream s brings xs[s] (frames * 1024, C) for slot slots[s].  Returns each stream's records (n_out, C),
    compares them and the state left behind with the rule's, bit for bit, and advances S."""
    dtype, channels = xs[0].dtype, xs[0].shape[1]
    Lp, T = np.asarray(table).shape
    H = (T - 1) * channels
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
    n_dst = out_first * channels
    dst_block, dst = guarded(n_dst)
    dst[:] = 0.0                                                          # the host clears a batch's records in front of the launch
    before = S.state.copy()
    tab = aligned_table(table)
    assert src.ctypes.data % 16 == 0 and tab.ctypes.data % 16 == 0
    assert lib.emu_truepeak(src.ctypes.data, dst.ctypes.data, rec.ctypes.data, len(xs), tab.ctypes.data, S.state.ctypes.data, hop, Lp, T,
                            channels, dtype.itemsize, first + 1 if blocks is None else blocks, reverse) == 1
    assert guards_intact(dst_block, n_dst), "a float outside the records was written"
    assert guards_intact(S.block, S.state.size), "a float outside the state was written"
    assert (src == np.ascontiguousarray(packed).reshape(-1).view(np.uint8)).all()
    flat = dst.reshape(out_first, channels)
    outs = [flat[r["out_first"]:r["out_first"] + r["n_out"]].copy() for r in rec]
    expect = before.copy()
    for s, (x, slot) in enumerate(zip(xs, slots)):
        old, new = S.parity[slot], S.parity[slot] ^ 1
        n_before = S.ref[slot].n
        want = kit.rule(x, hop, table, S.ref[slot])
        S.straddled_batch |= n_before % hop != 0
        S.straddled_frame |= any((n_before + 1024 * k) % hop != 0 for k in range(1, len(x) // 1024))
        S.emitted_nothing |= len(want) == 0
        assert len(want) == rec[s]["n_out"]
        if check:
            kit.same_records(outs[s], want, "stream %d, records" % s)
            kit.same_records(S.state[slot, new], S.ref[slot].words(), "stream %d, the state left behind" % s)
        expect[slot, new] = S.state[slot, new]
        expect[slot, old, H:] = 0.0                                       # the partial that was read is left empty for the batch after this
        S.N[slot], S.parity[slot], S.fresh[slot] = S.N[slot] + len(x), new, 0
    assert (S.state.view(np.uint32) == expect.view(np.uint32)).all(), "the other parity's history or another slot's state was written"
    return outs


def tables(Lp, T, kind):
    return kit.mixed_table(Lp, T) if kind == "mixed" else aacgpu.true_peak_design(Lp, T)["table"]


# the same five slots' frames, cut into batches in two ways: ragged batches of up to five streams of one to three frames
SPLIT_A = [[1, 3, 2, 1, 2], [3, 1, 1, 2, 0], [2, 2, 3, 1, 1]]
SPLIT_B = [[3, 1, 2, 2, 1], [1, 3, 1, 1, 1], [2, 2, 3, 1, 1]]
TOTALS = [6, 6, 6, 4, 3]
assert [sum(b[s] for b in SPLIT_A) for s in range(5)] == TOTALS == [sum(b[s] for b in SPLIT_B) for s in range(5)]

# (element, channels, hop, (phases, taps), table): every element type at 1, 2, 3, 6 and 8 channels, every hop, every table shape in both
# kinds — the smallest set that has each of them, not their product
CASES = [(np.float32, 1, 7, (1, 4), "mixed"), (np.int16, 2, 1000, (4, 12), "designed"), (np.float32, 3, 4800, (4, 24), "designed"),
         (np.int16, 6, 1024, (4, 24), "mixed"), (np.float32, 8, 4800, (8, 64), "mixed"), (np.int16, 8, 1000, (8, 64), "designed"),
         (np.float32, 2, 4800, (4, 12), "mixed"), (np.int16, 1, 4800, (1, 4), "designed"), (np.float32, 6, 1000, (4, 12), "designed"),
         (np.int16, 3, 7, (4, 24), "mixed"), (np.float32, 2, 1024, (8, 64), "designed")]


@pytest.mark.parametrize("case", CASES, ids=["%s-c%d-hop%d-L%dT%d-%s" % ("f32" if c[0] == np.float32 else "i16", c[1], c[2], c[3][0], c[3][1], c[4]) for c in CASES])
def test_truepeak_is_the_rule(lib, case, engine_lib):
    """Fresh slots, then both parities batch after batch, in two different splits of the same five streams; one workgroup more than
    there are frames, then two workgroups that walk the frames in reverse.  The third slot's second frame is a block of zeros.  On the
    kit's own results: some hop held a frame's edge and some hop a batch's wherever 1024 is no multiple of the hop (where it is, no hop
    can), and some batch emitted nothing for a stream wherever a hop is longer than a frame (where it is not, every frame emits)."""
    dtype, channels, hop, (Lp, T), kind = case
    table = tables(Lp, T, kind)
    assert table.shape == (Lp, T) and np.isfinite(table).all()
    if kind == "mixed":
        assert (table < 0).any() and (table > 0).any()
    whole = [source(f * 1024, channels, dtype, 100 * s + channels) for s, f in enumerate(TOTALS)]
    whole[2][1024:2048] = 0
    per_split = []
    for split in (SPLIT_A, SPLIT_B):
        S = Slots(7, channels, T)
        slots = [6 - s for s in range(5)]                                 # not in order, not from 0
        at, got, parities = [0] * 5, [[] for _ in range(5)], set()
        for b, frames_of in enumerate(split):
            here = [s for s in range(5) if frames_of[s]]
            xs = [whole[s][at[s] * 1024:(at[s] + frames_of[s]) * 1024] for s in here]
            parities |= {S.parity[slots[s]] for s in here}
            outs = launch(lib, S, xs, [slots[s] for s in here], hop, table, None if b % 2 == 0 else 2, b % 2)
            for s, o in zip(here, outs):
                got[s].append(o)
                at[s] += frames_of[s]
        assert at == TOTALS and parities == {0, 1}
        assert S.straddled_frame == S.straddled_batch == (1024 % hop != 0)
        assert S.emitted_nothing == (hop > 1024)
        per_split.append((got, S))
    for s in range(5):
        want, partial = kit.rule_whole(whole[s], hop, table)
        for got, S in per_split:
            kit.same_records(np.concatenate(got[s]), want, "stream %d, every batch's records against the rule over the whole stream" % s)
            slot = 6 - s
            kit.same_records(S.state[slot, S.parity[slot], (T - 1) * channels:], partial, "stream %d, the partial maximum at the end" % s)
    # the block of zeros: a hop that lies inside it, behind the reach of the samples in front of it, reads +0
    silent = [h for h in range(6 * 1024 // hop) if h * hop >= 1024 + T - 1 and (h + 1) * hop <= 2048]
    assert bool(silent) == (hop == 7)
    for got, S in per_split:
        assert (np.concatenate(got[2])[silent].view(np.uint32) == 0).all()


def test_the_kit_agrees_with_itself():
    """the rule twice in numpy: over a whole history, and hop by hop from a carried state cut at frames and off frames"""
    for dtype, channels, hop, (Lp, T) in ((np.float32, 2, 1000, (4, 12)), (np.int16, 3, 4800, (8, 64)), (np.float32, 1, 7, (1, 4))):
        x = source(7 * 1024, channels, dtype, hop)
        want = kit.self_check(x, hop, kit.mixed_table(Lp, T), [1024, 3072, 3073, 5000])
        assert len(want) == 7 * 1024 // hop


def test_a_reset_between_batches(lib, engine_lib):
    """a slot that is reset starts from nothing — clock, history, partial maximum — while its neighbour goes on; the partial it had
    carried (a hop of 4800 was under way) does not reach the new stream's first record"""
    hop, channels, table = 4800, 2, kit.mixed_table(4, 12)
    S = Slots(2, channels, 12)
    loud = source(2048, channels, np.float32, 1) * np.float32(64.0)
    launch(lib, S, [loud, source(1024, channels, np.float32, 2)], [0, 1], hop, table)
    assert (S.state[0, S.parity[0], 11 * channels:] > 0).all(), "slot 0 carries a partial maximum"
    S.reset(0)
    x = source(5 * 1024, channels, np.float32, 3)
    outs = launch(lib, S, [x[:3072], source(1024, channels, np.float32, 4)], [0, 1], hop, table, 2, 1)
    outs2 = launch(lib, S, [x[3072:], source(1024, channels, np.float32, 5)], [0, 1], hop, table)
    want, _ = kit.rule_whole(x, hop, table)
    kit.same_records(np.concatenate([outs[0], outs2[0]]), want, "the reset slot against a new stream")
    assert len(outs[0]) == 0 and len(outs2[0]) == 1 and S.N == [5120, 3072]
    assert float(want.max()) < 64.0 < float(np.abs(loud).max())


def test_a_nan_sample_makes_its_hops_nan(lib):
    """a NaN sample reaches the T - 1 samples behind it and no others: the records of the hops they lie in are NaNs, whether the hop
    lies inside a frame, holds a frame's edge (the atomic's path) or is carried into the next batch; every other record is a number"""
    hop, channels, (Lp, T) = 1000, 2, (4, 12)
    table = kit.mixed_table(Lp, T)
    x = source(4 * 1024, channels, np.float32, 11)
    x[300, 0] = np.nan               # inside hop 0 of frame 0
    x[1020, 1] = np.nan              # hop 1, and its reach crosses into frame 1
    x[2990, 0] = np.nan              # hop 2, which batch 1 carries into batch 2; its reach crosses into hop 3
    want, _ = kit.rule_whole(x, hop, table)
    assert np.isnan(want[:, 0]).tolist() == [True, False, True, True] and np.isnan(want[:, 1]).tolist() == [False, True, False, False]
    S = Slots(1, channels, T)
    got = launch(lib, S, [x[:2048]], [0], hop, table) + launch(lib, S, [x[2048:]], [0], hop, table, 1, 0)
    kit.same_records(np.concatenate(got), want, "a NaN sample")


def test_truepeak_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: the ragged batch
    (1, 3 and 2 frames, one stream in mid-hop), 1, 2, 3 and 8 channels, both element sizes, over heap blocks of exactly the buffers'
    sizes.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "truepeak_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DTRUEPEAK_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "truepeak_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "truepeak_emu: ok" in r.stdout, r.stdout + r.stderr


# EBU Tech 3341's true-peak cases in kind: sines of amplitude 0.5 at 48 kHz whose samples miss their crests
SINES = [(5000.0, 0.0), (8000.0, 67.5), (12000.0, 45.0), (16000.0, 60.0), (20000.0, 10.0)]


@pytest.mark.parametrize("freq,phase", SINES, ids=["%dHz-%gdeg" % s for s in SINES])
def test_what_the_number_means(lib, engine_lib, freq, phase):
    """the default design (four phases of 24 taps): the largest record after the first reads -6.02 dBTP within +0.2 / -0.4 dB, EBU
    Tech 3341's tolerance (a float64 restatement of the design reads -6.03, -6.02, -6.19, -6.31 and -6.15 for the five); the 12 kHz
    sine at 45 degrees reads below -9 dBFS as the meter's sample peak — the two quantities differ"""
    d = aacgpu.true_peak_design()
    assert (d["phases"], d["taps"]) == (4, 24)
    hop, n = 4800, 10 * 1024
    t = np.arange(n, dtype=np.float64)
    x = (0.5 * np.sin(2 * np.pi * freq * t / 48000.0 + np.deg2rad(phase))).astype(np.float32)[:, None]
    S = Slots(1, 1, 24)
    rec = np.concatenate(launch(lib, S, [x[:5 * 1024]], [0], hop, d["table"], 2, 0) + launch(lib, S, [x[5 * 1024:]], [0], hop, d["table"]))
    assert rec.shape == (2, 1)
    db = 20.0 * np.log10(float(rec[1:].max()))
    print("%g Hz at %g degrees: %.3f dBTP" % (freq, phase, db))
    assert -6.02 - 0.4 <= db <= -6.02 + 0.2
    if freq == 12000.0:
        meter = loudness_kit.rule(x, hop, np.array([[1, 0, 0, 0, 0], [1, 0, 0, 0, 0]], np.float32), loudness_kit.State(1))
        peak_db = 20.0 * np.log10(float(meter[:, 0, 1].max()))
        print("the meter's sample peak: %.3f dBFS" % peak_db)
        assert peak_db < -9.0
