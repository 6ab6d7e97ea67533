"""The feature stage's host-only part (include/aacgpu.h: aacg_features_counts, aacg_features_design; aac.js_amd/csrc/aacg_features.cpp)
and the binding's surface: the counts against a numpy restatement of the formula, the designed tables equal or adjacent float32 to a
restatement in numpy float64 here, and every host-side refusal of the limits.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import aacgpu
import resample_kit

INVALID_ARG = -1


def test_library_exports_the_new_symbols(engine_lib):
    for name in ("aacg_pipeline_set_features", "aacg_features_counts", "aacg_features_design"):
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    lib = aacgpu.load_library()
    assert len(lib.aacg_pipeline_set_features.argtypes) == 2 and len(lib.aacg_features_counts.argtypes) == 6 and len(lib.aacg_features_design.argtypes) == 11
    T = aacgpu.FeaturesConfig
    assert [n for n, _ in T._fields_] == ["frame_length", "hop", "pad_left", "n_rows", "n_mels", "log", "floor", "basis", "fb"]
    assert (C.sizeof(T), T.floor.offset, T.basis.offset, T.fb.offset) == (48, 24, 32, 40)
    # a null handle: the call answers without a device
    assert lib.aacg_pipeline_set_features(None, C.byref(T())) == INVALID_ARG


def count(N, K, H, P):
    """max(0, floor((N + P - K) / H) + 1), in numpy's integers"""
    return np.maximum(0, (np.asarray(N, np.int64) + P - K) // H + 1)


@pytest.mark.parametrize("K,H,P", [(400, 160, 200), (400, 160, 0), (32, 1, 31), (1024, 1024, 0), (64, 64, 63), (400, 400, 399), (36, 7, 5)])
def test_counts_are_the_formula(engine_lib, K, H, P):
    """count(n0 + samples) - count(n0) from every kind of clock: nothing consumed, N < K - P (no frame complete yet), on and off a hop,
    H = K, far along; the per-batch counts of a split add up to the whole stream's"""
    rng = np.random.default_rng(K + H + P)
    clocks = [0, 1, K - P - 1, K - P, K - P + 1, H, K, K + H - 1, 5 * H + 3, 2 ** 40 + 17] + [int(v) for v in rng.integers(0, 10 * K, 12)]
    for n0 in clocks:
        for samples in (0, 1, H - 1, H, K - P - 1, K - P, 341, 342, 1024, 3072, 12288):
            if n0 < 0 or samples < 0:
                continue
            want = int(count(n0 + samples, K, H, P) - count(n0, K, H, P))
            assert aacgpu.features_counts(K, H, P, n0, samples) == want, (n0, samples)
    assert aacgpu.features_counts(K, H, P, 0, K - P - 1) == 0 and aacgpu.features_counts(K, H, P, 0, K - P) == 1       # N < K - P: nothing yet
    at, total = 0, 0
    for n in (341, 342, 341, 1024, 2048):
        total += aacgpu.features_counts(K, H, P, at, n)
        at += n
    assert total == int(count(at, K, H, P))


def test_counts_refusals(engine_lib):
    lib, n = aacgpu.load_library(), C.c_uint64()
    assert lib.aacg_features_counts(400, 160, 200, 0, 1024, None) == INVALID_ARG
    for K, H, P in ((28, 7, 0), (1028, 7, 0), (402, 160, 0), (400, 0, 0), (400, 401, 0), (400, 160, 400)):
        assert lib.aacg_features_counts(K, H, P, 0, 1024, C.byref(n)) == INVALID_ARG, (K, H, P)
        with pytest.raises(aacgpu.AacgError):
            aacgpu.features_counts(K, H, P, 0, 1024)
    assert lib.aacg_features_counts(400, 160, 200, 2 ** 64 - 1, 2, C.byref(n)) == INVALID_ARG                            # a clock that would wrap


def design(rate, K, n_bins, n_mels, f_min=0.0, f_max=None):
    """aacg_features_design restated in numpy float64: (basis (2 n_bins, K), fb (n_mels, n_bins)) float32"""
    f_max = rate / 2 if f_max is None else f_max
    k = np.arange(K, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / K)                                    # the periodic Hann window
    b = np.arange(n_bins, dtype=np.int64)[:, None]
    ang = 2 * np.pi * ((b * np.arange(K, dtype=np.int64)[None, :]) % K).astype(np.float64) / K
    basis = np.empty((2 * n_bins, K), np.float64)
    basis[0::2], basis[1::2] = w * np.cos(ang), -(w * np.sin(ang))
    # the Slaney scale: 200 / 3 Hz per mel below 1 kHz, steps of ln(6.4) / 27 above
    f_sp, logstep = 200.0 / 3.0, np.log(6.4) / 27.0

    def to_mel(f):
        return 15.0 + np.log(f / 1000.0) / logstep if f >= 1000.0 else f / f_sp

    def to_hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), f_sp * m)

    edge = to_hz(to_mel(f_min) + (to_mel(f_max) - to_mel(f_min)) * np.arange(n_mels + 2, dtype=np.float64) / (n_mels + 1))
    f = np.arange(n_bins, dtype=np.float64) * rate / K
    lower = (f[None, :] - edge[:-2, None]) / (edge[1:-1] - edge[:-2])[:, None]
    upper = (edge[2:, None] - f[None, :]) / (edge[2:] - edge[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edge[2:] - edge[:-2]))[:, None]
    return basis.astype(np.float32), fb.astype(np.float32)


@pytest.mark.parametrize("rate,K,H,n_bins,n_mels,f_min,f_max", [(16000, 400, 160, 201, 80, 0.0, 0.0), (16000, 400, 160, 201, 128, 0.0, 0.0),
                                                              (48000, 1024, 512, 513, 64, 20.0, 20000.0), (8000, 32, 8, 17, 5, 100.0, 3500.0), (22050, 64, 64, 20, 1, 0.0, 8000.0)])
def test_design_is_the_restatement(engine_lib, rate, K, H, n_bins, n_mels, f_min, f_max):
    d = aacgpu.features_design(rate, K, H, n_bins, n_mels, f_min, f_max)
    basis, fb = design(rate, K, n_bins, n_mels, f_min, f_max or None)
    assert d["frame_length"] == K and d["hop"] == H and d["basis"].shape == basis.shape and d["fb"].shape == fb.shape
    assert resample_kit.adjacent_or_equal(d["basis"], basis).all() and resample_kit.adjacent_or_equal(d["fb"], fb).all()
    assert np.isfinite(d["basis"]).all() and np.isfinite(d["fb"]).all()
    # what the tables are: row 0 is the window (bin 0's cosine), bin 0 has no sine, every band is a triangle with its peak inside [f_min, f_max]
    assert (d["basis"][1].view(np.uint32) << 1 == 0).all() and d["basis"][0].argmax() == K // 2
    if n_mels > 1 and n_bins > 4 * n_mels:
        peaks = d["fb"].argmax(axis=1)
        assert (np.diff(peaks) > 0).all() and (d["fb"] >= 0).all() and (d["fb"].sum(axis=1) > 0).all()


def test_whisper_defaults(engine_lib):
    d = aacgpu.features_design()
    assert d["basis"].shape == (402, 400) and d["fb"].shape == (80, 201) and d["hop"] == 160
    assert d["fb"][:, 0].max() == 0 and abs(float(d["fb"][0].max()) - 0.0248) < 1e-3      # Slaney-normalised: the first band peaks near 2 / (edge width)


def test_design_refusals(engine_lib):
    lib = aacgpu.load_library()
    basis, fb = np.zeros((402, 400), np.float32), np.zeros((80, 201), np.float32)

    def call(rate=16000, K=400, H=160, n_bins=201, n_mels=80, f_min=0.0, f_max=0.0, b=basis.ctypes.data, nb=basis.size, f=fb.ctypes.data, nf=fb.size):
        return lib.aacg_features_design(rate, K, H, n_bins, n_mels, f_min, f_max, b, nb, f, nf)

    assert call() == 0
    bad = [dict(rate=0), dict(b=None), dict(f=None), dict(K=402), dict(K=28), dict(K=1028), dict(H=0), dict(H=401), dict(n_bins=0), dict(n_bins=514), dict(n_mels=0),
           dict(n_mels=129), dict(f_min=-1.0), dict(f_min=4000.0, f_max=4000.0), dict(f_max=8000.5), dict(nb=basis.size - 1), dict(nf=fb.size - 1), dict(f_min=float("nan"))]
    for how in bad:
        assert call(**how) == INVALID_ARG, how
    with pytest.raises(aacgpu.AacgError):
        aacgpu.features_design(16000, 402, 160)
