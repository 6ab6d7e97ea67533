"""A resident batch's PCM from the lane's packed buffer into a caller's planar tensor (aacg_pcm_planar, aac.js_amd/csrc/aacg_pcm_planar.h:
planar_body) against a numpy transposition, byte for byte over the whole destination and a poisoned guard on both sides of it: the
kernel's source run lane by lane on CPU threads (tests/emu/planar_emu.cpp with tests/emu/devport_emu.h).

The rule: dst[(s * C + c) * T + t] = src[(frame_first[s] * 1024 + t) * C + c] for t < frames[s] * 1024 and 0 behind that, T =
stride_frames * 1024; every element of the n_streams x C x T block is written, nothing outside it.  The source's values are distinct
per element, so a swapped channel, sample or frame cannot cancel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aacgpu
import emu_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PIPE_STREAM_DTYPE = np.dtype([("frame_first", "<u4"), ("frames", "<u4"), ("unit_first", "<u4"), ("frame_units", "<u4")])      # aacg_pipe_stream
GUARD = 4096            # poisoned bytes on either side of the destination


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    L = emu_lib.build_driver("planar_emu", ["tests/emu/planar_emu.cpp"], tmp_path_factory.mktemp("planar_emu"))
    L.emu_planar.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_int]
    L.emu_planar.restype = None
    L.emu_planar_items.argtypes = [C.c_uint32] * 3
    L.emu_planar_items.restype = C.c_uint32
    sizes = (C.c_uint32 * 3)()
    L.emu_planar_sizes(sizes)
    assert sizes[1] == PIPE_STREAM_DTYPE.itemsize and sizes[2] == aacgpu.SHAPE_STREAM_DTYPE.itemsize
    L.threads = int(sizes[0])
    return L


def aligned(n_bytes, fill):
    """n_bytes of uint8 at a 16-byte aligned address, filled"""
    raw = np.full(n_bytes + 16, fill, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n_bytes]


def source(n, dtype):
    """n elements, each its own index: as float (exact below 2^24), or as int16 modulo 65536"""
    i = np.arange(n, dtype=np.int64)
    return i.astype(np.float32) if dtype == np.float32 else (i % 65536).astype(np.uint16).view(np.int16)


def transposed(src, counts, channels, stride):
    """the rule in numpy: [stream][channel][stride * 1024]"""
    out = np.zeros((len(counts), channels, stride * 1024), src.dtype)
    first = 0
    for s, n in enumerate(counts):
        out[s, :, :n * 1024] = src[first * 1024 * channels:(first + n) * 1024 * channels].reshape(n * 1024, channels).T
        first += n
    return out


def check(lib, channels, dtype, counts, stride, blocks=None, reverse=0, table=PIPE_STREAM_DTYPE):
    dtype = np.dtype(dtype)
    S, n = len(counts), int(np.sum(counts))
    assert n * 1024 * channels < (1 << 24), "float indices stay exact"
    tab = np.zeros(S, table)
    tab["frames"] = counts
    tab["frame_first"] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for name in tab.dtype.names[2:]:
        tab[name] = 0xA5A5A5A5                            # the kernel reads a record's first two words only
    src_bytes = aligned(n * 1024 * channels * dtype.itemsize, 0)
    src = src_bytes.view(dtype)
    src[:] = source(src.size, dtype)
    n_dst = S * channels * stride * 1024 * dtype.itemsize
    block = aligned(GUARD + n_dst + GUARD, 0xC3)
    dst = block[GUARD:GUARD + n_dst]
    assert src.ctypes.data % 16 == 0 and dst.ctypes.data % 16 == 0
    items = lib.emu_planar_items(S, stride, dtype.itemsize)
    assert items == S * stride * 1024 // (16 // dtype.itemsize)
    full = (items + lib.threads - 1) // lib.threads
    blocks = full if blocks is None else blocks
    lib.emu_planar(src.ctypes.data, dst.ctypes.data, tab.ctypes.data, tab.dtype.itemsize, S, stride, channels, dtype.itemsize, blocks, reverse)
    want = transposed(src, counts, channels, stride)
    assert dst.tobytes() == want.tobytes(), "the kernel's tensor differs from the transposition (%d channels, %s, counts %s, stride %d, %d of %d workgroups)" % (
        channels, dtype, list(counts), stride, blocks, full)
    assert (block[:GUARD] == 0xC3).all() and (block[GUARD + n_dst:] == 0xC3).all(), "a byte outside the destination was written"
    return full


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("channels", range(1, 9))
def test_planar_is_the_transposition(lib, channels, dtype):
    """every channel count x both element sizes: three ragged streams without padding on the longest (stride 3) and with padding on
    all (stride 4), one stream of one frame, and 17 one-frame streams — more rows than one workgroup's stride covers (a workgroup of
    256 lanes takes one f32 frame or two int16 frames a step) —, workgroups forward and in reverse, with every workgroup a launch of
    that size gets and with so few that each lane walks several items"""
    check(lib, channels, dtype, [3, 1, 2], 3, blocks=2)
    check(lib, channels, dtype, [3, 1, 2], 3, reverse=1)
    check(lib, channels, dtype, [3, 1, 2], 4, blocks=3, reverse=1)
    check(lib, channels, dtype, [3, 1, 2], 4, blocks=1)
    check(lib, channels, dtype, [1], 1)
    check(lib, channels, dtype, [1], 1, blocks=1, reverse=1)
    full = check(lib, channels, dtype, [1] * 17, 1, blocks=2)
    assert full > 2
    check(lib, channels, dtype, [1] * 17, 1, blocks=3, reverse=1)
    # ... and the 48-byte records of the device plans' table, read with their own stride
    check(lib, channels, dtype, [2, 1], 2, blocks=2, table=aacgpu.SHAPE_STREAM_DTYPE)


def test_planar_item_count_is_bounded(lib):
    """the host's part refuses a launch whose items do not fit 31 bits (the kernel counts them in 32) instead of wrapping"""
    assert lib.emu_planar_items(4096, 1024, 4) == 4096 * 1024 * 256
    assert lib.emu_planar_items(4096, 2048, 4) == 0 and lib.emu_planar_items(1 << 20, 1 << 20, 2) == 0
    assert lib.emu_planar_items(4096, 2048, 2) == 4096 * 2048 * 128


def test_planar_under_sanitizers(tmp_path):
    """the same driver as a program of its own, built with -fsanitize=address,undefined and run as a child process: the int16 cases of
    1, 3 and 7 channels — where a source group is a 2-, 6- or 14-byte multiple and a misaligned or overrunning vector access would be —
    over heap blocks of exactly the buffers' sizes.  The sanitizers' runtimes are linked into the program: nothing is preloaded."""
    exe = str(tmp_path / "planar_emu_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-strict-aliasing", "-DAACG_EMU_BUILD", "-DPLANAR_EMU_MAIN", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-I", os.path.join(HERE, "emu"), "-pthread", "-Wall", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "emu", "planar_emu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "planar_emu: ok" in r.stdout, r.stdout + r.stderr
