"""The limiter's host-only part (include/aacgpu.h: aacg_limiter_design; aac.js_amd/csrc/aacg_limiter.cpp) and the binding's surface: the
symbols and the struct, the ABI version, the design against the formula in Python doubles rounded to float32 once, and the refusals that
need no device.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import aacgpu

INVALID_ARG = -1
SYMBOLS = ("aacg_pipeline_set_limiter", "aacg_pipeline_set_gain", "aacg_pipeline_gain", "aacg_limiter_design")


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    T = aacgpu.LimiterConfig
    assert [n for n, _ in T._fields_] == ["ceiling", "release"] and (C.sizeof(T), T.release.offset) == (8, 4)
    assert engine_lib.aacg_abi_version() == 6                              # new symbols only: no struct changed
    assert aacgpu.LIMIT_BLOCK == 64


def test_the_header_states_the_rule_and_drops_the_meter_s_not_here():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aacgpu.h")).read()
    assert "#define AACG_LIMIT_BLOCK 64" in text and "a gain or limiter that applies the result" not in text
    assert re.search(r"#define AACG_ABI_VERSION\s+6\b", text)


def test_null_handle_refusals(engine_lib):
    """every pipeline call answers a null handle without a device"""
    lib, g = aacgpu.load_library(), C.c_float(3.0)
    assert lib.aacg_pipeline_set_limiter(None, C.byref(aacgpu.LimiterConfig(0.5, 0.5))) == INVALID_ARG
    assert lib.aacg_pipeline_set_gain(None, 0, 1.0) == INVALID_ARG
    assert lib.aacg_pipeline_gain(None, 0, C.byref(g)) == INVALID_ARG and g.value == 3.0


@pytest.mark.parametrize("rate", [48000, 44100, 22050, 8000, 96000])
def test_design_is_the_formula(engine_lib, rate):
    for ceiling_db, release_ms in ((-1.0, 200.0), (0.0, 50.0), (-6.0, 1000.0), (-0.1, 5.0), (3.0, 0.01)):
        cfg = aacgpu.limiter_design(rate, ceiling_db, release_ms)
        want_c = np.float32(10.0 ** (ceiling_db / 20.0))
        want_r = np.float32(1.0 - math.exp(-64.0 / (rate * release_ms / 1000.0)))
        assert isinstance(cfg, aacgpu.LimiterConfig)
        for got, want in ((cfg.ceiling, want_c), (cfg.release, want_r)):
            assert np.float32(got) == want, (rate, ceiling_db, release_ms, got, want)
        assert 0.0 < cfg.release <= 1.0 and cfg.ceiling > 0.0
    d = aacgpu.limiter_design(rate)
    assert np.float32(d.ceiling) == np.float32(10.0 ** (-1.0 / 20.0)), "the defaults are -1 dB and 200 ms"
    assert abs(d.release - (1.0 - math.exp(-64.0 / (rate * 0.2)))) < 1e-7


def test_design_refusals(engine_lib):
    lib, cfg = aacgpu.load_library(), aacgpu.LimiterConfig(7.0, 7.0)
    assert lib.aacg_limiter_design(0, -1.0, 200.0, C.byref(cfg)) == INVALID_ARG
    assert lib.aacg_limiter_design(48000, -1.0, 200.0, None) == INVALID_ARG
    # results outside aacg_pipeline_set_limiter's limits: a ceiling that overflows or is not a number, a release of 0, negative or NaN
    for ceiling_db, release_ms in ((1e4, 200.0), (float("nan"), 200.0), (-1e4, 200.0), (-1.0, 1e30), (-1.0, -5.0), (-1.0, float("nan")), (-1.0, float("inf"))):
        assert lib.aacg_limiter_design(48000, ceiling_db, release_ms, C.byref(cfg)) == INVALID_ARG, (ceiling_db, release_ms)
        with pytest.raises(aacgpu.AacgError):
            aacgpu.limiter_design(48000, ceiling_db, release_ms)
    assert (cfg.ceiling, cfg.release) == (7.0, 7.0), "a refusal writes nothing"
    assert lib.aacg_limiter_design(48000, -1.0, 0.0, C.byref(cfg)) == 0 and cfg.release == 1.0      # no time constant: all the way back in one block
