"""A resident batch's packed PCM mixed to one or two channels (aacg_pcm_mix, aac.js_amd/csrc/aacg_pcm_mix.h: mix_body) against the rule of
include/aacgpu.h in numpy float32 (mix_kit.mix_rule), on integer views of the whole destination and a poisoned guard on both sides of
it: the kernel's source run lane by lane on CPU threads (tests/emu/mix_emu.cpp with tests/emu/devport_emu.h).

The rule: acc = M[o][0] * x[0], then acc = acc + M[o][c] * x[c] for c = 1 .. C-1, every product and every sum rounded to float32, never
fused; f32 out = acc; int16 in = the sample as float, out = acc rounded to nearest even and saturated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import mix_kit

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096            # poisoned bytes on either side of the destination


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("mix_emu", ["tests/emu/mix_emu.cpp"], tmp_path_factory.mktemp("mix_emu"))
    L.emu_mix.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p, C.c_uint32, C.c_int]
    L.emu_mix.restype = C.c_int
    L.emu_mix_items.argtypes = [C.c_uint32] * 2
    L.emu_mix_items.restype = C.c_uint32
    sizes = (C.c_uint32 * 2)()
    L.emu_mix_sizes(sizes)
    assert sizes[1] == 16, "the matrix travels as 16 floats"
    L.threads = int(sizes[0])
    return L


def aligned(n_bytes, fill):
    """n_bytes of uint8 at a 16-byte aligned address, filled"""
    raw = np.full(n_bytes + 16, fill, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n_bytes]


def f32_source(n, channels, seed):
    """mixed signs, magnitudes 2^-20 .. 2^3, both ends present"""
    rng = np.random.default_rng(seed)
    x = (rng.choice([-1.0, 1.0], (n, channels)) * np.exp2(rng.uniform(-20.0, 3.0, (n, channels)))).astype(np.float32)
    x[0, :] = np.float32(2.0 ** -20)
    x[1, :] = np.float32(-8.0)
    return x


def i16_source(n, channels, matrix, seed):
    """the whole int16 range at random, and made rows in front: every channel at 32767, at -32768, at -32767, and for each row of the
    matrix the channels at the ends of the range with the coefficients' signs and against them — the largest sums either way"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, channels)).astype(np.int16)
    x[0, :], x[1, :], x[2, :] = 32767, -32768, -32767
    at = 3
    for row in np.asarray(matrix):
        x[at, :] = np.where(row >= 0, 32767, -32768)
        x[at + 1, :] = np.where(row >= 0, -32768, 32767)
        at += 2
    return x


def run(lib, x, matrix, blocks, reverse):
    """one emulated launch over x (frames * 1024, C) -> the destination as (frames * 1024, O), the guards checked"""
    matrix = np.ascontiguousarray(matrix, np.float32)
    (n, channels), out_channels, item = x.shape, matrix.shape[0], x.dtype.itemsize
    assert n % 1024 == 0
    src = aligned(x.nbytes, 0)
    src.view(x.dtype)[:] = x.reshape(-1)
    n_dst = n * out_channels * item
    block = aligned(GUARD + n_dst + GUARD, 0xC3)
    dst = block[GUARD:GUARD + n_dst]
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0
    items = lib.emu_mix_items(n // 1024, item)
    assert items == n // (16 // item)
    full = (items + lib.threads - 1) // lib.threads
    blocks = full + 2 if blocks is None else blocks
    assert lib.emu_mix(src.ctypes.data, dst.ctypes.data, n // 1024, channels, out_channels, item, matrix.ctypes.data, blocks, reverse) == 1
    assert (block[:GUARD] == 0xC3).all() and (block[GUARD + n_dst:] == 0xC3).all(), "a byte outside the destination was written"
    return dst.view(x.dtype).reshape(n, out_channels).copy(), full


def check(lib, x, matrix, blocks, reverse):
    got, full = run(lib, x, matrix, blocks, reverse)
    want = mix_kit.mix_rule(x, matrix)
    view = np.uint32 if x.dtype == np.float32 else np.uint16
    wrong = np.argwhere(np.ascontiguousarray(got).view(view) != np.ascontiguousarray(want).view(view))
    assert wrong.size == 0, "the kernel's mix differs from the rule at %d of %d elements, first at (sample, channel) %s: %r against %r (%s, %d -> %d, %s of %d workgroups)" % (
        len(wrong), got.size, wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])], x.dtype, x.shape[1], matrix.shape[0], blocks, full)
    return full


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("out_channels", [1, 2])
@pytest.mark.parametrize("channels", range(1, 9))
def test_mix_is_the_rule(lib, channels, out_channels, dtype):
    """every C x O x element type with the hostile matrix: 1 and 3 frames, with one workgroup (every lane walks several items where there
    are more than 256), with three, forward and in reverse, and with two workgroups more than the items need"""
    m = mix_kit.hostile_matrix(out_channels, channels)
    assert len(set(np.abs(m).ravel().tolist())) == m.size and (m < 0).any() == (m.size > 1) and (np.abs(m) > 1).any()
    for frames in (1, 3):
        n = frames * 1024
        if dtype == np.float32:
            x = f32_source(n, channels, 100 * channels + frames)
            assert np.abs(x).min() == np.float32(2.0 ** -20) and np.abs(x).max() == 8 and (x < 0).any() and (x > 0).any()
        else:
            x = i16_source(n, channels, m, 100 * channels + frames)
            exact = (m.astype(np.float64)[None, :, :] * x.astype(np.float64)[:, None, :]).sum(axis=2)
            assert exact.max() > 32768 and exact.min() < -32769, "sums beyond the int16 range in both directions"
            assert (x == 32767).any() and (x == -32768).any() and (x == -32767).any()
        check(lib, x, m, 1, 0)
        full = check(lib, x, m, 3, 1)
        check(lib, x, m, None, 0)
        if dtype == np.float32:
            assert full == frames                      # one f32 frame is one workgroup's 256 items: three blocks of one frame walk nothing twice, one block of three does
    # (an int16 frame is 128 items: a launch of one frame with three workgroups has two that find nothing to do)


@pytest.mark.parametrize("out_channels", [1, 2])
@pytest.mark.parametrize("channels", range(1, 9))
def test_mix_rounds_int16_halves_to_even_and_saturates(lib, channels, out_channels):
    """coefficients of 0.5 over int16 columns: every sum is exact in float, an odd sum of samples is an exact half — 0.5, 1.5, -0.5,
    -2.5 and so on go to the even neighbour —, and the columns at the ends of the range saturate where C > 2.  M = [0.5, 0.5] over odd
    sums is the two-channel case."""
    m = np.full((out_channels, channels), 0.5, np.float32)
    rng = np.random.default_rng(7 + channels)
    x = rng.integers(-6, 7, (1024, channels)).astype(np.int16)
    x[:8, 0] = [1, 3, -1, -3, 5, -5, 7, -7]                # with zeros beside them: 0.5 -> 0, 1.5 -> 2, -0.5 -> -0, -1.5 -> -2, 2.5 -> 2, ...
    x[:8, 1:] = 0
    x[8, :], x[9, :] = 32767, -32768
    x[10, :] = 32767
    x[10, 0] = 32766                                       # (C = 2: 32766.5 -> 32766, the even one)
    odd = x.astype(np.int64).sum(axis=1) % 2 == 1
    assert odd.sum() > 100, "exact halves"
    want = mix_kit.mix_rule(x, m)
    assert want[0, 0] == 0 and want[1, 0] == 2 and want[2, 0] == 0 and want[3, 0] == -2 and want[4, 0] == 2 and want[5, 0] == -2 and want[6, 0] == 4
    if channels > 2:
        assert want[8, 0] == 32767 and want[9, 0] == -32768
    check(lib, x, m, 1, 0)
    check(lib, x, m, 3, 1)


def test_mix_item_count_is_bounded(lib):
    """the host's part refuses a launch whose items do not fit 31 bits (the kernel counts them in 32) instead of wrapping; a pipeline's
    largest batch, 2^22 frames, fits"""
    assert lib.emu_mix_items(1 << 22, 4) == (1 << 22) * 256 and lib.emu_mix_items(1 << 22, 2) == (1 << 22) * 128
    assert lib.emu_mix_items(1 << 23, 4) == 0 and lib.emu_mix_items(1 << 24, 2) == 0


def test_mix_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: 1, 3, 6 and 7 channels
    to 1 and 2, both element sizes — where a source item is a 16-, 48-, 96- or 112-byte multiple and a misaligned or overrunning vector
    access would be — over heap blocks of exactly the buffers' sizes.  The sanitizers' runtimes are linked into the program: nothing is
    preloaded."""
    exe = str(tmp_path / "mix_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DMIX_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "mix_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mix_emu: ok" in r.stdout, r.stdout + r.stderr
