"""The loudness meter's host-only part (include/aacgpu.h: aacg_loudness_counts, aacg_loudness_design, aacg_loudness_integrate;
aac.js_amd/csrc/aacg_loudness.cpp) and the binding's surface: the symbols, the null-handle refusals, the design against a float64
restatement rounded once (equal values; at 48 kHz the standard's published coefficients), the counts against N // hop, the integration
against a float64 numpy restatement to 1e-9 LU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import loudness_kit as kit

INVALID_ARG = -1
SYMBOLS = ("aacg_pipeline_set_loudness", "aacg_pipeline_loudness_out", "aacg_pipeline_loudness_counts", "aacg_loudness_counts", "aacg_loudness_design",
           "aacg_loudness_integrate")


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    T = aacgpu.LoudnessConfig
    assert [n for n, _ in T._fields_] == ["hop", "coeffs"] and (C.sizeof(T), T.coeffs.offset) == (44, 4)
    assert engine_lib.aacg_abi_version() == 6                              # new symbols only: no struct changed


def test_null_handle_refusals(engine_lib):
    """every pipeline call answers a null handle without a device"""
    lib, n, buf = aacgpu.load_library(), np.zeros(4, np.uint32), np.zeros(16, np.float32)
    assert lib.aacg_pipeline_set_loudness(None, C.byref(aacgpu.LoudnessConfig(4800))) == INVALID_ARG
    assert lib.aacg_pipeline_loudness_out(None, buf.ctypes.data, buf.size, n.ctypes.data) == INVALID_ARG
    assert lib.aacg_pipeline_loudness_counts(None, n.ctypes.data, n.ctypes.data, 1, n.ctypes.data) == INVALID_ARG


@pytest.mark.parametrize("rate", [48000, 44100, 16000])
def test_design_is_the_restatement(engine_lib, rate):
    d = aacgpu.loudness_design(rate)
    want = kit.design64(rate)
    assert d["hop"] == rate // 10 and d["coeffs"].shape == (2, 5) and d["coeffs"].dtype == np.float32
    assert (d["coeffs"].view(np.uint32) == want.view(np.uint32)).all(), (d["coeffs"], want)
    if rate == 48000:
        assert (d["coeffs"] == kit.BS1770_48K.astype(np.float32)).all(), "the standard's published 48 kHz coefficients"
        assert np.abs(kit.design64(48000).astype(np.float64) - kit.BS1770_48K).max() < 1e-7
    assert aacgpu.loudness_design(rate, hop=512)["hop"] == 512


def test_design_refusals(engine_lib):
    lib, k = aacgpu.load_library(), np.zeros((2, 5), np.float32)
    assert lib.aacg_loudness_design(0, k.ctypes.data) == INVALID_ARG and lib.aacg_loudness_design(48000, None) == INVALID_ARG
    with pytest.raises(aacgpu.AacgError):
        aacgpu.loudness_design(0)


@pytest.mark.parametrize("hop", [1, 7, 1000, 1024, 4800, 2 ** 20])
def test_counts_are_the_formula(engine_lib, hop):
    rng = np.random.default_rng(hop)
    clocks = [0, 1, hop - 1, hop, hop + 1, 2 ** 40 + 17] + [int(v) for v in rng.integers(0, 2 ** 45, 40)]
    for n0 in clocks:
        for samples in (0, 1, hop - 1, hop, 1024, 3072, 16384, int(rng.integers(0, 2 ** 22))):
            assert aacgpu.loudness_counts(hop, n0, samples) == (n0 + samples) // hop - n0 // hop, (n0, samples)
    at = total = 0
    for n in (1024, 3072, 1024, 2048, 16384):
        total += aacgpu.loudness_counts(hop, at, n)
        at += n
    assert total == at // hop


def test_counts_refusals(engine_lib):
    lib, n = aacgpu.load_library(), C.c_uint64()
    assert lib.aacg_loudness_counts(4800, 0, 1024, None) == INVALID_ARG
    for hop in (0, 2 ** 20 + 1):
        assert lib.aacg_loudness_counts(hop, 0, 1024, C.byref(n)) == INVALID_ARG
        with pytest.raises(aacgpu.AacgError):
            aacgpu.loudness_counts(hop, 0, 1024)


def records(energies):
    """(n_hops, C, 2) records with these energies and peaks nobody reads"""
    e = np.asarray(energies, np.float32)
    return np.stack([e, np.full_like(e, 0.5)], axis=2)


def close(got, want):
    return (np.isneginf(got) and np.isneginf(want)) or abs(got - want) <= 1e-9


def test_integrate_is_the_restatement(engine_lib):
    rng = np.random.default_rng(1)
    hop = 4800
    # loud programme with quiet stretches: the relative gate removes some blocks, the absolute gate the silent ones
    e = hop * 10.0 ** (rng.uniform(-3.0, -1.0, (40, 2)))
    e[10:18] *= 1e-3                                                      # 30 dB down: below the relative gate, above the absolute one
    e[25:31] = 1e-12                                                      # below -70 LUFS
    for weights in (None, [1.0, 1.41], [0.0, 1.0]):
        got, mom = aacgpu.loudness_integrate(records(e), hop, weights, momentary=True)
        want, want_mom = kit.integrate64(records(e), hop, weights)
        assert close(got, want), (weights, got, want)
        assert mom.shape == want_mom.shape == (37,) and np.abs(mom - want_mom).max() <= 1e-9
        assert aacgpu.loudness_integrate(records(e), hop, weights) == got
    _, l = kit.integrate64(records(e), hop)
    ungated = -0.691 + 10.0 * np.log10((10.0 ** ((l[l > -70.0] + 0.691) / 10.0)).mean())
    assert (l <= -70.0).any() and ((l > -70.0) & (l <= ungated - 10.0)).any(), "both gates remove blocks in this case"
    assert kit.integrate64(records(e), hop)[0] > ungated + 0.1, "the relative gate raises the figure"


def test_integrate_with_nothing_above_the_gates(engine_lib):
    hop = 1000
    quiet = records(np.full((12, 1), hop * 1e-9))                          # -90.7 LUFS: every block below the absolute gate
    assert np.isneginf(aacgpu.loudness_integrate(quiet, hop)) and np.isneginf(kit.integrate64(quiet, hop)[0])
    silent = records(np.zeros((8, 3)))
    got, mom = aacgpu.loudness_integrate(silent, hop, momentary=True)
    assert np.isneginf(got) and np.isneginf(mom).all() and len(mom) == 5
    for n in (0, 1, 3):                                                   # fewer than four hops: no block
        got, mom = aacgpu.loudness_integrate(records(np.ones((n, 2))), hop, momentary=True)
        assert np.isneginf(got) and len(mom) == 0
    assert close(aacgpu.loudness_integrate(records(np.ones((4, 2))), hop), kit.integrate64(records(np.ones((4, 2))), hop)[0])


def test_integrate_refusals(engine_lib):
    lib, out, r = aacgpu.load_library(), C.c_double(), records(np.ones((5, 2)))
    assert lib.aacg_loudness_integrate(r.ctypes.data, 5, 2, 4800, None, C.byref(out), None) == 0
    assert lib.aacg_loudness_integrate(None, 5, 2, 4800, None, C.byref(out), None) == INVALID_ARG
    assert lib.aacg_loudness_integrate(r.ctypes.data, 5, 2, 4800, None, None, None) == INVALID_ARG
    for ch, hop in ((0, 4800), (9, 4800), (2, 0), (2, 2 ** 20 + 1)):
        assert lib.aacg_loudness_integrate(r.ctypes.data, 5, ch, hop, None, C.byref(out), None) == INVALID_ARG
    with pytest.raises(ValueError):
        aacgpu.loudness_integrate(np.ones((5, 2)), 4800)
    with pytest.raises(ValueError):
        aacgpu.loudness_integrate(r, 4800, weights=[1.0])
