"""The resampler's C ABI without a GPU (aacg_pipeline_set_resample, aacg_pipeline_out_samples, aacg_resample_counts, aacg_resample_design:
include/aacgpu.h): the new symbols in the library and in the binding's list, the counts against their formula, and the default table
against a restatement in numpy float64 (resample_kit.design)."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import resample_kit as kit

INVALID_ARG = -1
RATES = {(1, 3): (48000, 16000), (160, 441): (44100, 16000), (160, 147): (44100, 48000), (441, 160): (16000, 44100), (2, 1): (24000, 48000)}


def test_library_exports_the_new_symbols(engine_lib):
    for name in ("aacg_pipeline_set_resample", "aacg_pipeline_out_samples", "aacg_resample_counts", "aacg_resample_design"):
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    lib = aacgpu.load_library()
    assert len(lib.aacg_pipeline_set_resample.argtypes) == 5 and len(lib.aacg_pipeline_out_samples.argtypes) == 5
    assert len(lib.aacg_resample_counts.argtypes) == 6 and len(lib.aacg_resample_design.argtypes) == 9
    # null handles: the calls answer without a device
    h = np.ones(4, np.float32)
    n = np.zeros(1, np.uint32)
    assert lib.aacg_pipeline_set_resample(None, 1, 3, 4, h.ctypes.data) == INVALID_ARG
    assert lib.aacg_pipeline_out_samples(None, n.ctypes.data, n.ctypes.data, 1, n.ctypes.data) == INVALID_ARG


@pytest.mark.parametrize("ratio", kit.RATIOS, ids=["%d/%d" % r for r in kit.RATIOS])
def test_counts_are_the_formula(ratio):
    """per_frame[f] = ceil((n0 + 1024 (f + 1)) L / M) - ceil((n0 + 1024 f) L / M) from every clock modulo M (and from clocks beyond M,
    of which only the remainder counts), n0_after the clock to go on with; the sum over many calls is ceil(total L / M)"""
    L, M = ratio
    for n0 in sorted(set(list(range(0, M, max(M // 7, 1))) + [M - 1, M + 5, 70001])):
        per, after = aacgpu.resample_counts(L, M, n0, 5)
        want = [kit.n_out(n0 + 1024 * f, n0 + 1024 * (f + 1), L, M) for f in range(5)]
        assert per.tolist() == want and after == (n0 + 5 * 1024) % M, (n0, per, want)
        assert set(per.tolist()) <= {1024 * L // M, 1024 * L // M + 1} or (1024 * L) % M == 0
    n0, total, frames = 0, 0, 0
    rng = np.random.default_rng(L + M)
    for _ in range(200):
        f = int(rng.integers(1, 5))
        per, n0 = aacgpu.resample_counts(L, M, n0, f)
        total, frames = total + int(per.sum()), frames + f
        assert total == kit.ceil_div(frames * 1024 * L, M) and n0 == (frames * 1024) % M
    # no frame: nothing is written, the clock is its remainder
    per, after = aacgpu.resample_counts(L, M, M + 1 if M > 1 else 0, 0)
    assert len(per) == 0 and after == (1 if M > 1 else 0)


def test_counts_refusals():
    lib = aacgpu.load_library()
    per, after = np.full(4, 7, np.uint32), C.c_uint32(9)
    for L, M in ((0, 3), (3, 0), (1025, 3), (3, 1025)):
        assert lib.aacg_resample_counts(L, M, 0, 4, per.ctypes.data, C.byref(after)) == INVALID_ARG
    assert (per == 7).all() and after.value == 9, "a refused call wrote its outputs"
    assert lib.aacg_resample_counts(1, 3, 0, 4, None, None) == 0


@pytest.mark.parametrize("taps", [4, 16, 32, 64])
@pytest.mark.parametrize("ratio", kit.RATIOS, ids=["%d/%d" % r for r in kit.RATIOS])
def test_design_is_its_restatement(ratio, taps):
    """each coefficient equal to numpy's or the adjacent float (libm and numpy differ in the last bits of a double, and one rounding to
    float moves that by at most one ulp); L / M reduced; every phase row, summed in double, is 1 within 2^-24 x sum |h[p][t]|, the bound
    of rounding each coefficient once"""
    L, M = ratio
    in_rate, out_rate = RATES[ratio]
    if L * taps > 16384:
        with pytest.raises(aacgpu.AacgError):
            aacgpu.resample_design(in_rate, out_rate, taps)
        return
    for args, named in (((), {}), ((0.9, 6.0), {"rolloff": 0.9, "beta": 6.0})):
        gl, gm, got = aacgpu.resample_design(in_rate, out_rate, taps, *args)
        wl, wm, want = kit.design(in_rate, out_rate, taps, **named)
        assert (gl, gm) == (wl, wm) == (L, M) and got.shape == want.shape == (L, taps)
        assert kit.adjacent_or_equal(got, want).all(), np.argwhere(~kit.adjacent_or_equal(got, want))[:4]
        for row in got.astype(np.float64):
            total = 0.0
            for g in row:
                total += g
            assert abs(total - 1.0) <= 2.0 ** -24 * np.abs(row).sum(), (row, total)
    # the same ratio from rates that are not reduced the same way; the ratio alone with no table
    assert aacgpu.resample_design(in_rate * 3, out_rate * 3, taps)[:2] == (L, M)
    lib, l, m = aacgpu.load_library(), C.c_uint32(), C.c_uint32()
    assert lib.aacg_resample_design(in_rate, out_rate, taps, 0.0, 0.0, C.byref(l), C.byref(m), None, 0) == 0 and (l.value, m.value) == (L, M)


def test_design_is_symmetric_and_centred():
    """the prototype is linear-phase: g[n] = g[L T - 1 - n], that is h[p][t] against h[L - 1 - p][T - 1 - t] up to each row's own sum"""
    L, M, h = aacgpu.resample_design(48000, 16000, 32)
    assert (L, M) == (1, 3) and h[0].tolist() == h[0][::-1].tolist() and h[0].argmax() in (15, 16)
    L, M, h = aacgpu.resample_design(44100, 16000, 32)
    assert np.allclose(h, h[::-1, ::-1], rtol=0, atol=1e-6)


def test_design_refusals():
    """every limit of aacg_pipeline_set_resample, and the design's own"""
    lib = aacgpu.load_library()
    l, m, table = C.c_uint32(77), C.c_uint32(77), np.full(16384, 7.0, np.float32)

    def call(in_rate, out_rate, taps, rolloff=0.0, beta=0.0, lp=C.byref(l), mp=C.byref(m), tp=table.ctypes.data, cap=table.size):
        return lib.aacg_resample_design(in_rate, out_rate, taps, rolloff, beta, lp, mp, tp, cap)

    assert call(48000, 16000, 32) == 0
    table[:] = 7.0
    for taps in (0, 2, 6, 30, 68, 128):
        assert call(48000, 16000, taps) == INVALID_ARG, taps                      # taps: a multiple of 4 in 4..64
    assert call(48000, 48001, 4) == INVALID_ARG and call(2048, 2047, 4) == INVALID_ARG          # L, M <= 1024
    assert call(16000, 44100, 64) == INVALID_ARG and call(256, 257, 64) == INVALID_ARG          # L x taps <= 16384
    assert call(48000, 5000, 4) == INVALID_ARG and call(5000, 48000, 4) == INVALID_ARG          # 1/8 <= L / M <= 8
    assert call(8000, 1000, 4) == 0 and call(1000, 8000, 4) == 0
    table[:] = 7.0
    assert call(0, 16000, 32) == INVALID_ARG and call(48000, 0, 32) == INVALID_ARG
    assert call(48000, 16000, 32, lp=None) == INVALID_ARG and call(48000, 16000, 32, mp=None) == INVALID_ARG
    assert call(48000, 16000, 32, rolloff=1.5) == INVALID_ARG and call(48000, 16000, 32, rolloff=-0.1) == INVALID_ARG
    assert call(48000, 16000, 32, beta=-1.0) == INVALID_ARG and call(48000, 16000, 32, rolloff=float("nan")) == INVALID_ARG
    assert call(48000, 16000, 32, cap=31) == INVALID_ARG and call(44100, 16000, 32, cap=160 * 32 - 1) == INVALID_ARG
    assert call(48000, 16000, 32, tp=None, cap=32) == INVALID_ARG
    assert (table == 7.0).all(), "a refused call wrote the table"
