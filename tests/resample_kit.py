"""What the PCM resampler's tests share (tests/test_pcm_resample_*.py): the rule of include/aacgpu.h (aacg_pipeline_set_resample) in numpy
float32, the counts' formula, a hostile table, and the design function restated in numpy float64."""
from math import gcd

import numpy as np

RATIOS = [(1, 3), (160, 441), (160, 147), (441, 160), (2, 1)]


def ceil_div(a, b):
    return -((-a) // b)


def n_out(N0, N1, L, M):
    """outputs m with N0 <= floor(m M / L) < N1"""
    return ceil_div(N1 * L, M) - ceil_div(N0 * L, M)


def resample_rule(x, L, M, table):
    """The rule over a whole stream since its reset: x (N, C) float32 or int16, table (L, T) float32 -> (ceil(N L / M), C) of x's dtype.
    acc = h[p][0] * x[i], then acc = acc + h[p][t] * x[i - t] for t = 1 .. T-1, with i = floor(m M / L), p = (m M) mod L and x[j] = 0
    for j < 0: every product and every sum a float32 operation of its own.  int16: the samples converted to float, the sum rounded to
    nearest even and saturated."""
    x = np.asarray(x)
    h = np.ascontiguousarray(table, np.float32)
    assert x.ndim == 2 and h.shape[0] == L and x.dtype in (np.float32, np.int16)
    T = h.shape[1]
    xf = np.concatenate([np.zeros((T - 1, x.shape[1]), np.float32), x.astype(np.float32)])
    m = np.arange(ceil_div(x.shape[0] * L, M), dtype=np.int64)
    i, p = (m * M) // L + (T - 1), (m * M) % L
    acc = h[p, 0][:, None] * xf[i]
    for t in range(1, T):
        acc = acc + h[p, t][:, None] * xf[i - t]
    assert acc.dtype == np.float32
    if x.dtype == np.int16:
        return np.clip(np.rint(acc), -32768, 32767).astype(np.int16)
    return acc


def hostile_table(L, T, seed=5):
    """random signs, magnitudes 2^-6 .. 2^2, none a dyadic fraction: not a filter, every rounding shows"""
    rng = np.random.default_rng(seed + 1000 * L + T)
    h = rng.choice([-1.0, 1.0], (L, T)) * np.exp2(rng.uniform(-6.0, 2.0, (L, T))) * 1.0001
    h[0, 0], h[-1, -1], h[0, 1] = 3.3, -2.7, -0.3        # (the smallest table too has both signs and a coefficient above 1)
    return h.astype(np.float32)


def design(in_rate, out_rate, taps, rolloff=0.95, beta=9.0):
    """aacg_resample_design restated in float64: (L, M, table float32 (L, taps))"""
    g = gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    n = L * taps
    k = np.arange(n, dtype=np.float64)
    centre = (n - 1) * 0.5
    fc = 0.5 * rolloff / max(L, M)
    proto = np.sinc(2.0 * fc * (k - centre)) * np.kaiser(n, beta)
    rows = proto.reshape(taps, L).T                      # h[p][t] = g[p + t L]
    sums = np.array([sum(float(v) for v in row) for row in rows])
    return L, M, (rows / sums[:, None]).astype(np.float32)


def adjacent_or_equal(a, b):
    """float32 arrays: every element equal or the neighbouring float"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    # (coefficients of either sign: compare on the ordered integer line)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib) <= 1
