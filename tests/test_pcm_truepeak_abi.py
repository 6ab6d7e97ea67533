"""The true-peak stage's host-only part (include/aacgpu.h: aacg_true_peak_design; aac.js_amd/csrc/aacg_truepeak.cpp) and the binding's
surface: the symbols, the refusals that need no device (a null handle; the design's), the design against aacg_resample_design float for
float and against a float64 restatement, and the kit against itself.  The refusals of a live pipeline (no meter, the limits, a table
that is not finite, a second call, a call after the first batch, the two arming refusals) need a device to make the pipeline:
tests/test_pcm_truepeak_gpu.py::test_refusals_leave_the_pipeline_as_it_was.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import resample_kit
import truepeak_kit as kit

INVALID_ARG = -1
SYMBOLS = ("aacg_pipeline_set_true_peak", "aacg_pipeline_true_peak_out", "aacg_true_peak_design")


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    T = aacgpu.TruePeakConfig
    assert [n for n, _ in T._fields_] == ["phases", "taps", "table"] and (C.sizeof(T), T.taps.offset, T.table.offset) == (16, 4, 8)
    assert engine_lib.aacg_abi_version() == 6                              # new symbols only: no struct changed


def test_null_handle_refusals(engine_lib):
    """every pipeline call answers a null handle without a device"""
    lib, buf, h = aacgpu.load_library(), np.zeros(16, np.float32), np.ones((4, 12), np.float32)
    assert lib.aacg_pipeline_set_true_peak(None, C.byref(aacgpu.TruePeakConfig(4, 12, h.ctypes.data))) == INVALID_ARG
    assert lib.aacg_pipeline_set_true_peak(None, None) == INVALID_ARG
    assert lib.aacg_pipeline_true_peak_out(None, buf.ctypes.data, buf.size) == INVALID_ARG


@pytest.mark.parametrize("phases,taps", [(4, 24), (4, 12), (1, 4), (8, 64), (2, 8), (3, 16)])
@pytest.mark.parametrize("rolloff,beta", [(0.95, 5.0), (0.0, 0.0), (0.8, 9.0)])
def test_design_is_the_resamplers(engine_lib, phases, taps, rolloff, beta):
    """float for float the table aacg_resample_design(1, phases, taps, rolloff, beta) writes, zero defaults included; every row sums to
    1; and within a float of the float64 restatement"""
    d = aacgpu.true_peak_design(phases, taps, rolloff, beta)
    assert (d["phases"], d["taps"]) == (phases, taps) and d["table"].shape == (phases, taps) and d["table"].dtype == np.float32
    L, M, want = aacgpu.resample_design(1, phases, taps, rolloff, beta)
    assert (L, M) == (phases, 1)
    assert (d["table"].view(np.uint32) == np.asarray(want, np.float32).reshape(phases, taps).view(np.uint32)).all()
    assert np.abs(d["table"].astype(np.float64).sum(axis=1) - 1.0).max() < 1e-6
    again = kit.design(phases, taps, rolloff or 0.95, beta or 9.0)
    assert resample_kit.adjacent_or_equal(d["table"], again).all()


def test_design_defaults(engine_lib):
    d = aacgpu.true_peak_design()
    assert (d["phases"], d["taps"]) == (4, 24)
    assert (d["table"].view(np.uint32) == aacgpu.true_peak_design(4, 24, 0.95, 5.0)["table"].view(np.uint32)).all()


def test_design_refusals(engine_lib):
    """the stage's limits on phases and taps, and aacg_resample_design's own: rolloff outside (0, 1], beta outside (0, 30], a capacity
    below phases x taps, a null table with a capacity"""
    lib, t = aacgpu.load_library(), np.zeros(8 * 64, np.float32)
    design = lambda Lp, T, r=0.95, b=5.0, table=t.ctypes.data, cap=t.size: lib.aacg_true_peak_design(Lp, T, r, b, table, cap)
    assert design(4, 24) == 0
    for Lp, T in ((0, 24), (9, 24), (4, 0), (4, 2), (4, 10), (4, 68)):
        assert design(Lp, T) == INVALID_ARG, (Lp, T)
    for r, b in ((-0.1, 5.0), (1.5, 5.0), (float("nan"), 5.0), (0.95, -1.0), (0.95, 31.0)):
        assert design(4, 24, r, b) == INVALID_ARG, (r, b)
        assert lib.aacg_resample_design(1, 4, 24, r, b, C.byref(C.c_uint32()), C.byref(C.c_uint32()), t.ctypes.data, t.size) == INVALID_ARG
    assert design(4, 24, cap=95) == INVALID_ARG
    with pytest.raises(aacgpu.AacgError):
        aacgpu.true_peak_design(9, 24)


def test_the_kit_computes_the_rule_twice():
    """truepeak_kit: the rule over a whole history and hop by hop from a carried state agree bit for bit, with a NaN among the samples"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((5000, 3)).astype(np.float32)
    x[1234, 1] = np.nan
    want = kit.self_check(x, 700, kit.mixed_table(4, 12), [1, 1024, 2047, 4100])
    assert want.shape == (7, 3) and np.isnan(want[:, 1]).sum() in (1, 2) and not np.isnan(want[:, [0, 2]]).any()
    i16 = rng.integers(-32768, 32768, (3000, 2)).astype(np.int16)
    kit.self_check(i16, 1024, aacgpu.true_peak_design(8, 64)["table"], [1024, 2048])
