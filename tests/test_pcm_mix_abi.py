"""The mix's C ABI without a GPU (aacg_pipeline_set_mix, aacg_pipeline_out_channels, aacg_mix_standard: include/aacgpu.h): the new symbols
in the library and in the binding's list, and the standard downmix against its table computed in numpy float64 (mix_kit.standard_table)
and rounded to float32 once."""
import ctypes

import numpy as np
import pytest

import aacgpu
import mix_kit

GAINS = [2.0 ** -0.5, 0.5]
INVALID_ARG = -1


def test_library_exports_the_new_symbols(engine_lib):
    for name in ("aacg_pipeline_set_mix", "aacg_pipeline_out_channels", "aacg_mix_standard"):
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    lib = aacgpu.load_library()
    assert len(lib.aacg_pipeline_set_mix.argtypes) == 3 and len(lib.aacg_mix_standard.argtypes) == 5
    # null handles: the calls answer without a device
    m = np.ones(2, np.float32)
    assert lib.aacg_pipeline_set_mix(None, 1, m.ctypes.data) == INVALID_ARG
    assert lib.aacg_pipeline_out_channels(None) == INVALID_ARG


@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("out_channels", [1, 2])
@pytest.mark.parametrize("channels", sorted(mix_kit.POSITIONS))
def test_mix_standard_is_the_table(channels, out_channels, normalise):
    lib = aacgpu.load_library()
    for gain in GAINS:
        got = np.full((out_channels, channels), np.nan, np.float32)
        assert lib.aacg_mix_standard(channels, out_channels, gain, normalise, got.ctypes.data) == 0
        want = mix_kit.standard_table(channels, out_channels, gain, normalise)
        assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (got, want)
        assert (got == aacgpu.mix_standard(channels, out_channels, gain, bool(normalise))).all()
        if normalise:
            # a normalised row sums to 1 within 1 ulp of float (2^-23), accumulated in double
            for row in got.astype(np.float64):
                total = 0.0
                for g in row:
                    total += g
                assert abs(total - 1.0) <= 2.0 ** -23, (row, total)


def test_mix_standard_knows_the_positions():
    """the table by hand for 5.1 and for 7.1: which position gets what"""
    a, h = float(np.float32(2.0 ** -0.5)), 2.0 ** -0.5
    m = aacgpu.mix_standard(6, 2, normalise=False)
    assert m.tolist() == np.array([[h, 1, 0, a, 0, 0], [h, 0, 1, 0, a, 0]], np.float64).astype(np.float32).tolist()
    m = aacgpu.mix_standard(8, 2, surround_gain=0.5, normalise=False)
    assert m.tolist() == np.array([[h, 1, 0, 1, 0, 0.5, 0, 0], [h, 0, 1, 0, 1, 0, 0.5, 0]], np.float64).astype(np.float32).tolist()
    m = aacgpu.mix_standard(6, 2)
    assert abs(float(m[0, 1]) - 1.0 / (1.0 + h + h)) < 1e-7 and m[0, 5] == 0 and m[1, 5] == 0      # the familiar 1 / (1 + 1/sqrt 2 + 1/sqrt 2); no LFE
    m = aacgpu.mix_standard(4, 1, normalise=False)
    assert m.tolist() == np.array([[h, 0.5, 0.5, a * h]], np.float64).astype(np.float32).tolist()
    assert aacgpu.mix_standard(2, 2).tolist() == [[1, 0], [0, 1]] and aacgpu.mix_standard(1, 2).tolist() == [[1], [1]]


def test_mix_standard_refusals():
    lib = aacgpu.load_library()
    m = np.full(32, 7.0, np.float32)
    for channels, out_channels in ((7, 2), (0, 2), (9, 1), (6, 3), (6, 0)):
        assert lib.aacg_mix_standard(channels, out_channels, 0.5, 1, m.ctypes.data) == INVALID_ARG, (channels, out_channels)
    assert lib.aacg_mix_standard(6, 2, 0.5, 1, None) == INVALID_ARG
    assert lib.aacg_mix_standard(6, 2, float("nan"), 1, m.ctypes.data) == INVALID_ARG
    assert (m == 7.0).all(), "a refused call wrote the matrix"
    with pytest.raises(aacgpu.AacgError):
        aacgpu.mix_standard(7, 2)
