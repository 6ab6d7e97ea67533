"""The host-only part of the limiter's true-peak detector (include/aacgpu.h: aacg_trim_design_delay; aac.js_amd/csrc/aacg_limiter.cpp) and
the binding's surface: the three symbols, the ABI version, the design against exact integer arithmetic in Python, its equality with
aacg_trim_design at the delays 64 and 0, its refusals, and the refusals of the pipeline calls that need no device.  No GPU."""
import ctypes as C
import itertools
import os
import re
from fractions import Fraction

import pytest

import aacgpu
import resample_kit

INVALID_ARG = -1
ALL = 2 ** 64 - 1
LIMIT = 2 ** 40
SYMBOLS = ("aacg_pipeline_set_limiter_true_peak", "aacg_pipeline_limiter_delay", "aacg_trim_design_delay")
RATES = [(48000, 16000), (44100, 16000), (44100, 48000), (16000, 44100), (24000, 48000)]
DELAYS = [0, 64, 66, 76, 96, 1, 2 ** 32 - 1]              # none, the plain limiter, the detector at 4, 24 and 64 taps, and any other


def want_design(skip_in, keep_in, delay, L, M, taps):
    """A(t) = 2 L t + 2 L delay + L taps - 1 (the filter term only with a resampler pass); skip = ceil(A(skip_in) / 2M), keep = ceil(A(skip_in +
    keep_in) / 2M) - skip, residual = skip - A(skip_in) / 2M: Python integers and Fractions"""
    A = lambda t: 2 * L * t + 2 * L * delay + (L * taps - 1 if taps else 0)
    skip = -((-A(skip_in)) // (2 * M))
    keep = None if keep_in is None else -((-A(skip_in + keep_in)) // (2 * M)) - skip
    return skip, keep, skip - Fraction(A(skip_in), 2 * M)


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    assert engine_lib.aacg_abi_version() == 6                              # new symbols only: no struct changed
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aacgpu.h")).read()
    assert re.search(r"#define AACG_ABI_VERSION\s+6\b", text)
    for name in SYMBOLS:
        assert re.search(r"^int\s+%s\(" % name, text, re.M), name
    assert "Not here: true-peak (oversampled) limiting" not in text


def test_design_is_exact_integer_arithmetic(engine_lib):
    for (rin, rout), taps, skip_in, delay in itertools.product(RATES, [4, 8, 32, 64], [0, 1024, 2112, 2113, 2 ** 32 + 17, 2 ** 39], DELAYS):
        L, M, _ = resample_kit.design(rin, rout, 4)
        if L * taps > 16384:
            continue
        for keep_in in (None, 0, 1, 1024, 44100 * 300, 2 ** 33 + 5):
            want = want_design(skip_in, keep_in, delay, L, M, taps)
            if want[0] >= LIMIT or (want[1] is not None and want[1] >= LIMIT):
                with pytest.raises(aacgpu.AacgError):
                    aacgpu.trim_design(skip_in, keep_in, resample=(L, M, taps), delay=delay)
                continue
            got = aacgpu.trim_design(skip_in, keep_in, resample=(L, M, taps), delay=delay)
            assert got == want and isinstance(got[2], Fraction) and 0 <= got[2] < 1, (rin, rout, taps, skip_in, keep_in, delay, got, want)
    # without a resampler pass the filter term is left out
    for skip_in, keep_in, delay in itertools.product([0, 2112, 2 ** 40 - 77], (None, 0, 5000), (0, 64, 76)):
        assert aacgpu.trim_design(skip_in, keep_in, delay=delay) == (skip_in + delay, keep_in, Fraction(0)), (skip_in, keep_in, delay)


def test_the_delays_64_and_0_are_trim_design(engine_lib):
    """delay = 64 gives exactly aacg_trim_design(..., 1, ...) and delay = 0 exactly (..., 0, ...): results and refusals"""
    lib = aacgpu.load_library()
    cases = [(s, k, L, M, t) for s, k in itertools.product([0, 1, 2112, 2 ** 32 + 17, 2 ** 39, 2 ** 40 - 1, 2 ** 40 - 65, 2 ** 40], [ALL, 0, 1, 6000, 2 ** 33 + 5, 2 ** 40])
             for L, M, t in ((1, 1, 0), (1, 3, 32), (160, 441, 16), (441, 160, 64), (8, 1, 4), (1024, 1024, 64), (0, 1, 0), (1, 1025, 0), (1, 1, 65))]
    refused = 0
    for (s, k, L, M, t), (limiter, delay) in itertools.product(cases, ((1, 64), (0, 0))):
        a, b = [C.c_uint64(7) for _ in range(4)], [C.c_uint64(7) for _ in range(4)]
        ra = lib.aacg_trim_design(s, k, limiter, L, M, t, *[C.byref(v) for v in a])
        rb = lib.aacg_trim_design_delay(s, k, delay, L, M, t, *[C.byref(v) for v in b])
        assert ra == rb and [v.value for v in a] == [v.value for v in b], (s, k, L, M, t, limiter)
        refused += ra != 0
    assert 0 < refused < 2 * len(cases)


def test_design_refusals(engine_lib):
    lib = aacgpu.load_library()
    out = [C.c_uint64(7) for _ in range(4)]
    refs = [C.byref(v) for v in out]
    assert lib.aacg_trim_design_delay(2112, ALL, 76, 1, 3, 32, *refs) == 0 and out[1].value == ALL and out[3].value == 6
    assert lib.aacg_trim_design_delay(2112, 5, 76, 1, 1, 0, refs[0], refs[1], None, None) == 0 and (out[0].value, out[1].value) == (2188, 5)      # the residual is optional
    for v in out:
        v.value = 7
    for bad in ((2 ** 40, ALL, 0, 1, 1, 0), (0, 2 ** 40, 0, 1, 1, 0), (0, ALL, 76, 0, 1, 0), (0, ALL, 76, 1, 0, 0), (0, ALL, 76, 1025, 1, 0), (0, ALL, 76, 1, 1025, 0), (0, ALL, 76, 1, 1, 65),
                (2 ** 40 - 1, ALL, 76, 1, 1, 0),             # the result would be 2^40 + 75
                (0, ALL, 2 ** 32 - 1, 1024, 1, 0)):          # ... and 2^42
        assert lib.aacg_trim_design_delay(*bad, *refs) == INVALID_ARG, bad
    assert lib.aacg_trim_design_delay(0, ALL, 76, 1, 1, 0, None, refs[1], refs[2], refs[3]) == INVALID_ARG
    assert lib.aacg_trim_design_delay(0, ALL, 76, 1, 1, 0, refs[0], None, refs[2], refs[3]) == INVALID_ARG
    assert [v.value for v in out] == [7] * 4, "a refusal writes nothing"
    with pytest.raises(aacgpu.AacgError):
        aacgpu.trim_design(2 ** 40, None, delay=76)


def test_null_handle_refusals(engine_lib):
    """both pipeline calls answer a null handle, and the delay query a null pointer, without a device"""
    lib, n = aacgpu.load_library(), C.c_uint32(3)
    table = (C.c_float * 4)(1, 0, 0, 0)
    cfg = aacgpu.TruePeakConfig(1, 4, C.cast(table, C.c_void_p).value)
    assert lib.aacg_pipeline_set_limiter_true_peak(None, C.byref(cfg)) == INVALID_ARG
    assert lib.aacg_pipeline_limiter_delay(None, C.byref(n)) == INVALID_ARG and n.value == 3
