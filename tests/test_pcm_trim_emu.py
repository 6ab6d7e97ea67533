"""A resident batch's packed PCM cut to each stream's window (aacg_pcm_trim, aac.js_amd/csrc/aacg_pcm_trim.h: trim_body) against a numpy
slice, BIT FOR BIT and byte for byte over the whole destination block: the kernel's source run lane by lane on CPU threads
(tests/emu/trim_emu.cpp with tests/emu/devport_emu.h), forward and with the workgroups in reverse.  The source holds random BITS (NaNs
of every kind for f32), the destination is poisoned and larger than needed, and what is expected is built from the poison: a byte
written outside a stream's own elements — in front of the block, between two streams, behind it — shows, as does one not written.

Beside it the feature stage's case that no caller could reach before the trim (aacg_pcm_features.h: features_body with n_in == 0),
through tests/emu/features_emu.cpp's existing interface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import features_kit
import test_pcm_features_emu as features_emu
import trim_kit as kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096            # poisoned bytes on either side of the destination
POISON = 0xC3
REC = np.dtype([(n, np.uint32) for n in ("src_first", "n_keep", "out_first", "item_first")])
T = kit.TILE
KEEPS = [0, 1, 3, 7, 8, 9, T - 1, T, T + 1, 2 * T + 5]
DTYPES = [np.float32, np.int16]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("trim_emu", ["tests/emu/trim_emu.cpp"], tmp_path_factory.mktemp("trim_emu"))
    L.emu_trim.argtypes = [C.c_void_p] * 3 + [C.c_uint64] + [C.c_uint32] * 6 + [C.c_int]
    L.emu_trim.restype = C.c_int
    L.emu_trim_span.argtypes = [C.c_uint64] * 3 + [C.c_uint32, C.c_void_p]
    L.emu_trim_items.argtypes, L.emu_trim_items.restype = [C.c_uint32, C.c_int], C.c_uint32
    sizes = (C.c_uint32 * 3)()
    L.emu_trim_sizes(sizes)
    assert sizes[1] == REC.itemsize == 16 and sizes[2] == T
    L.threads = int(sizes[0])
    return L


def aligned(n_bytes, fill):
    """a block of GUARD + n_bytes + GUARD bytes, all `fill`, whose middle part begins 16-byte aligned: (block, middle)"""
    raw = np.full(GUARD + n_bytes + GUARD + 16, fill, np.uint8)
    off = (-(raw.ctypes.data + GUARD)) % 16
    block = raw[off:off + GUARD + n_bytes + GUARD]
    return block, block[GUARD:GUARD + n_bytes]


def random_bits(n, channels, dtype, seed):
    """(n, channels) elements of random bits: every pattern, NaNs and infinities included, so only a copy of the bits passes"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), (n, channels), dtype=np.uint64).astype(np.uint32 if dtype == np.float32 else np.uint16)


def launch(lib, src, streams, row=None, blocks=None, reverse=0, gaps=None, slack=64):
    """one emulated launch over the source `src` (samples, channels) of bit patterns: stream s keeps streams[s] = (first sample in the
    source, n_keep).  Packed: tight, or with gaps[s] untouched samples in front of stream s.  row: planar rows of that many elements.
    The whole destination block — guards, gaps and `slack` samples behind the output — is compared with what the rule writes and nothing
    else.  Returns the items the launch had."""
    channels, bits = src.shape[1], src.dtype
    E = bits.itemsize
    rec = np.zeros(len(streams), REC)
    out_first = items = 0
    for s, (first, n_keep) in enumerate(streams):
        out_first += (gaps or [0] * len(streams))[s]
        rec[s] = (first, n_keep, out_first, items)
        out_first += n_keep
        items += lib.emu_trim_items(n_keep, 1 if row else 0)
        assert first + n_keep <= len(src)
    n_dst = (len(streams) * channels * row if row else (out_first + slack) * channels) * E
    dst_block, dst = aligned(n_dst, POISON)
    want_block = dst_block.copy()
    want = want_block[GUARD:GUARD + n_dst].view(bits)
    for s, (first, n_keep) in enumerate(streams):
        if row:
            rows = want[:len(streams) * channels * row].reshape(len(streams), channels, row)
            rows[s, :, :n_keep] = src[first:first + n_keep].T
            rows[s, :, n_keep:] = 0
        else:
            at = int(rec[s]["out_first"]) * channels
            want[at:at + n_keep * channels] = src[first:first + n_keep].reshape(-1)
    src_block, src_mem = aligned(src.nbytes, 0x3C)            # the extent ends where the source ends: what lies behind it is not the batch's
    src_mem.view(bits)[:] = src.reshape(-1)
    assert src_mem.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0
    blocks = items + 2 if blocks is None else blocks
    ran = lib.emu_trim(src_mem.ctypes.data, dst.ctypes.data, rec.ctypes.data, src.size, len(streams), items, row or 0, channels, E, max(blocks, 1), reverse)
    assert ran == (1 if items else 0), "a launch without items is none"
    wrong = np.flatnonzero(dst_block != want_block)
    assert wrong.size == 0, "%d bytes of the destination block differ from the rule's, the first at byte %d of the destination (%d bytes)" % (
        wrong.size, int(wrong[0]) - GUARD, n_dst)
    assert (src_mem.view(bits) == src.reshape(-1)).all() and (src_block[:GUARD] == 0x3C).all() and (src_block[GUARD + src.nbytes:] == 0x3C).all()
    return items


def three_ways(n_items):
    """one workgroup (it walks every item), four in reverse, and two more than there are items"""
    return [(1, 0), (4, 1), (None, 0)]


@pytest.mark.parametrize("layout", ["packed", "planar"])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "i16"])
def test_trim_is_the_slice(lib, dtype, channels, layout):
    """ten streams, one of every n_keep, each at an odd place of the source (so that source and destination residues differ from
    stream to stream), tight"""
    src = random_bits(sum(KEEPS) + 40 * len(KEEPS) + 17, channels, dtype, 7 * channels)
    streams, at = [], 0
    for k, n_keep in enumerate(KEEPS):
        at += 2 * k + 1                                      # the skipped samples in front of the stream's kept range
        streams.append((at, n_keep))
        at += n_keep + 3                                     # ... and the cut-off ones behind it
    row = 2048 if layout == "planar" else None
    for blocks, reverse in three_ways(0):
        items = launch(lib, src, streams, row, blocks, reverse)
        assert items == sum(max(-(-n // T), 1 if row else 0) for n in KEEPS)
    if layout == "planar":                                   # ... and rows far longer than any stream: the zeros are shared out among the items
        launch(lib, src, streams[-3:] + streams[:2], 4096, 3, 1)


@pytest.mark.parametrize("dtype,channels", [(np.int16, 1), (np.float32, 1), (np.int16, 3), (np.float32, 3)], ids=["i16-mono", "f32-mono", "i16-c3", "f32-c3"])
def test_every_pair_of_residues(lib, dtype, channels):
    """every residue modulo 16 bytes of the source against every one of the packed destination (8 x 8 for int16 mono, 4 x 4 for f32
    mono): a first stream keeps `rd` samples, so that the second one's output begins at that residue, and its source begins at `rs`;
    behind it a third, so that both of its ends have a neighbour in their granule"""
    V = 16 // np.dtype(dtype).itemsize
    src = random_bits(4 * T + 64, channels, dtype, 99)
    for n_keep in (1, V - 1, V, 37, T + 9):
        for rs in range(V):
            for rd in range(V):
                streams = [(0, rd), (V + rs, n_keep), (V + rs + n_keep + 5, 2)]
                launch(lib, src, streams, None, 2, (rs + rd) & 1)
                launch(lib, src, streams, None, 3, 1, gaps=[0, 0, 1])      # ... and with an untouched sample behind it instead


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "i16"])
def test_neighbours_share_a_granule(lib, dtype):
    """three streams back to back whose boundaries fall inside ONE 16-byte granule, mono; written by other workgroups in either order,
    nothing of a neighbour may be touched — and the same with canaries between the streams in the place of the neighbours"""
    V = 16 // np.dtype(dtype).itemsize
    src = random_bits(3 * T + 200, 1, dtype, 5)
    for counts in ([1, 1, 1], [V - 2, 1, 1], [V + 1, 1, V - 3] if V > 4 else [V + 1, 1, 1], [T + 1, 2, T + 5], [2 * T + V - 1, 1, 9]):
        streams = [(3, counts[0]), (3 + counts[0] + 1, counts[1]), (3 + counts[0] + 1 + counts[1] + 2, counts[2])]
        for blocks, reverse in three_ways(0):
            launch(lib, src, streams, None, blocks, reverse)
            launch(lib, src, streams, None, blocks, reverse, gaps=[1, 1, 1])
            launch(lib, src, streams, None, blocks, reverse, gaps=[0, V, 1])


@pytest.mark.parametrize("layout", ["packed", "planar"])
@pytest.mark.parametrize("dtype,channels", [(np.float32, 2), (np.int16, 1), (np.int16, 6)], ids=["f32-c2", "i16-c1", "i16-c6"])
def test_streams_and_batches_that_keep_nothing(lib, dtype, channels, layout):
    row = 1024 if layout == "planar" else None
    src = random_bits(3000, channels, dtype, 21)
    for blocks, reverse in three_ways(0):
        # a stream that keeps nothing between two that keep, in front of them, behind them
        assert launch(lib, src, [(1, 700), (900, 0), (901, 9)], row, blocks, reverse) == (4 if row else 3)
        launch(lib, src, [(5, 0), (5, 0), (7, T), (2000, 0)], row, blocks, reverse)
        # a batch that keeps nothing: packed, no item and no launch, the destination untouched; planar, its rows are zeros
        assert launch(lib, src, [(0, 0), (1024, 0), (2048, 0)], row, blocks, reverse) == (3 if row else 0)


@pytest.mark.parametrize("dtype,channels", [(np.int16, 1), (np.int16, 3), (np.float32, 1), (np.float32, 5)], ids=["i16-c1", "i16-c3", "f32-c1", "f32-c5"])
def test_the_source_ends_inside_a_vector(lib, dtype, channels):
    """a stream keeps up to the source's very last element where the extent is no multiple of 16 bytes, and one begins at its first: the
    aligned vectors that hold those elements are not all the source's"""
    for n in (1301, 1302, 1303, 1307):
        src = random_bits(n, channels, dtype, n)
        for layout_row in (None, 1024):
            launch(lib, src, [(0, 5), (n - 700, 700)], layout_row, 2, 1)
            launch(lib, src, [(n - 1, 1)], layout_row, 1, 0)


def test_the_rule_s_arithmetic(lib):
    """aacg_trim_span, which the pipeline's host code and aacg_trim_counts share, against Python integers — positions beyond 2^32"""
    out = (C.c_uint32 * 2)()
    for Q in (0, 1, 1024, 2 ** 32 - 3, 2 ** 33 + 77, 2 ** 41):
        for skip, keep in ((0, None), (0, 0), (Q + 5, 10), (Q + 1024, 1), (Q + 1023, 1), (max(Q - 3, 0), 4), (max(Q - 3, 0), 3), (Q, 1024), (Q + 1, None), (2 ** 40 - 1, 2 ** 40 - 1)):
            for n_in in (0, 1, 1024, 4096):
                lib.emu_trim_span(Q, skip, 2 ** 64 - 1 if keep is None else keep, n_in, out)
                assert (out[0], out[1]) == kit.span(Q, skip, keep, n_in), (Q, skip, keep, n_in)


def test_trim_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: 1, 2, 3 and 8
    channels, both element sizes, both layouts, over heap blocks of exactly the buffers' sizes — a source that ends inside a vector and a
    ragged output included.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "trim_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DTRIM_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "trim_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "trim_emu: ok" in r.stdout, r.stdout + r.stderr


# ---- the feature stage behind a trim: a stream that brings no sample ----------------------------------------------------------------
@pytest.fixture(scope="module")
def features_lib(tmp_path_factory):
    return features_kit.driver(tmp_path_factory.mktemp("features_emu_trim"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "i16"])
@pytest.mark.parametrize("row_extra", [None, 2], ids=["packed", "planar"])
def test_features_with_no_sample(features_lib, dtype, row_extra):
    """n_in == 0, which a trim's window makes possible: the old history goes to the other parity unchanged (a fresh slot's: zeros), no
    frame is emitted, planar padding is written — features_emu's launch checks all three — and the stream goes on afterwards as if the
    empty batch had not been: its frames are the rule's over what it consumed"""
    shape = features_kit.SHAPES[0]
    K, H, P, B, NM = shape
    basis, fb = features_kit.hostile_tables(K, B, NM)
    empty = np.zeros(0, dtype)
    state = features_emu.Slots(4, K)
    pre = features_kit.as_float(features_kit.source(K + 2 * H + 3, dtype, 31))
    state.seed(2, pre, 1)
    xs = [features_kit.source(1024, dtype, 41), features_kit.source(2048, dtype, 42)]
    # an empty stream between two that bring samples; slot 2 has history, slot 3 is fresh
    outs = features_emu.launch(features_lib, state, [xs[0], empty, empty], [0, 2, 3], shape, basis, fb, False, row_extra, 2, 1)
    assert [len(o) for o in outs][1:] == [0, 0] and state.N[2] == len(pre) and state.N[3] == 0 and state.fresh[3] == 0
    # a launch of empty streams only
    outs = features_emu.launch(features_lib, state, [empty, empty], [2, 3], shape, basis, fb, False, row_extra, None, 0)
    assert [len(o) for o in outs] == [0, 0]
    # ... and then samples: the frames of slot 2 are the rule's over (pre, xs[1]) behind those pre completed, slot 3's over xs[0] alone
    outs = features_emu.launch(features_lib, state, [xs[1], xs[0]], [2, 3], shape, basis, fb, False, row_extra, 3, 0)
    whole = features_kit.rule(features_lib, np.concatenate([pre, features_kit.as_float(xs[1])]), K, H, P, basis, fb, features_emu.FLOOR)
    done = features_kit.count(len(pre), K, H, P)
    assert np.array_equal(outs[0].view(np.uint32), whole[done:].view(np.uint32))
    alone = features_kit.rule(features_lib, features_kit.as_float(xs[0]), K, H, P, basis, fb, features_emu.FLOOR)
    assert np.array_equal(outs[1].view(np.uint32), alone.view(np.uint32))
