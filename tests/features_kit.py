"""What the feature stage's tests share (tests/test_pcm_features_*.py): the emulator driver with the rule of include/aacgpu.h as a straight C
loop (tests/emu/features_emu.cpp: emu_features_rule), the counts' formula restated, hostile tables, inputs that never repeat, and the ulp
distance the log output is held to."""
import ctypes as C

import numpy as np

import emu_lib

SHAPES = [(32, 7, 31, 3, 1), (400, 160, 200, 201, 80), (1024, 1024, 0, 16, 128), (64, 1, 0, 33, 5)]      # (K, H, P, B, n_mels)
REC = np.dtype([("in_first", "<u4"), ("n_in", "<u4"), ("out_first", "<u4"), ("n_out", "<u4"), ("item_first", "<u4"), ("off0", "<i4"), ("slot", "<u4"), ("flags", "<u4")])
TILE = 16
_lib = None


def driver(tmp_dir):
    """the emulator driver, built once per process"""
    global _lib
    if _lib is None:
        L = emu_lib.build_driver("features_emu", ["tests/emu/features_emu.cpp"], tmp_dir)
        L.emu_features.argtypes = [C.c_void_p] * 3 + [C.c_uint32] * 2 + [C.c_void_p] * 3 + [C.c_uint32] * 4 + [C.c_float] + [C.c_uint32] * 4 + [C.c_int]
        L.emu_features.restype = C.c_int
        L.emu_features_rule.argtypes = [C.c_void_p, C.c_uint64] + [C.c_uint32] * 5 + [C.c_void_p] * 2 + [C.c_float, C.c_uint32, C.c_void_p]
        L.emu_features_rule.restype = C.c_uint64
        L.emu_features_check.argtypes = [C.c_uint32] * 5
        sizes = (C.c_uint32 * 4)()
        L.emu_features_sizes(sizes)
        assert sizes[1] == REC.itemsize == 32 and sizes[2] == TILE
        L.threads, L.lds_bytes = int(sizes[0]), int(sizes[3])
        _lib = L
    return _lib


def count(N, K, H, P):
    """feature frames a slot has emitted after N consumed samples: max(0, floor((N + P - K) / H) + 1)"""
    return max(0, (N + P - K) // H + 1)


def hostile_tables(K, B, n_mels, seed=7):
    """(basis (2B, K), fb (n_mels, B)): seeded random entries with |v| in [0.5, 2) and mixed signs — not a transform: a mis-indexed sample,
    row or bin shows grossly"""
    rng = np.random.default_rng(seed + 100000 * K + 100 * B + n_mels)

    def table(shape):
        return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 2.0, shape)).astype(np.float32)

    basis, fb = table((2 * B, K)), table((n_mels, B))
    assert (np.abs(basis) >= 0.5).all() and (np.abs(basis) < 2).all() and (basis < 0).any() and (basis > 0).any()
    return basis, fb


def source(n, dtype, seed):
    """n samples of which no two are equal: a stretch of a permutation of the int16 range — as int16, or PCM-scaled and off the grid as float"""
    assert n <= 65536
    v = np.random.default_rng(seed).permutation(65536)[:n].astype(np.int64) - 32768
    if dtype == np.int16:
        return v.astype(np.int16)
    return ((v + 0.37) / 32768.0).astype(np.float32)


def as_float(x):
    """what the stage takes: int16 samples times 2^-15 (exact), floats as they are"""
    x = np.asarray(x)
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32)


def rule(lib, x, K, H, P, basis, fb, floor=1e-3, log=False):
    """THE RULE over a whole stream since its reset, x float32: (count(len(x)), n_mels) float32"""
    x = np.ascontiguousarray(x, np.float32)
    basis, fb = np.ascontiguousarray(basis, np.float32), np.ascontiguousarray(fb, np.float32)
    n = count(len(x), K, H, P)
    out = np.zeros((max(n, 1), fb.shape[0]), np.float32)
    got = lib.emu_features_rule(x.ctypes.data, len(x), K, H, P, basis.shape[0], fb.shape[0], basis.ctypes.data, fb.ctypes.data, floor, 1 if log else 0, out.ctypes.data)
    assert got == n
    return out[:n]


def log_reference(mel, floor):
    """float32(log10 in float64 of max(the rule's mel, floor))"""
    return np.log10(np.maximum(mel.astype(np.float64), float(np.float32(floor)))).astype(np.float32)


def ulps(a, b):
    """distance of float32 arrays on the ordered integer line"""
    ia, ib = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: differs from the rule at %d of %d elements, first at (frame, mel) %s: %r against %r" % (
        what, len(wrong), got.size, wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])])
