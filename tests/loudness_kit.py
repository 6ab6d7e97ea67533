"""What the loudness tests share (tests/test_pcm_loudness_*.py): the meter's rule of include/aacgpu.h as a plain loop in numpy float32, the
K-weighting design and the gated integration restated in numpy float64, hostile coefficient sets.  Nothing here shares code with the
kernel (aac.js_amd/csrc/aacg_pcm_loudness.h) or with the library's host part (aac.js_amd/csrc/aacg_loudness.cpp)."""
import numpy as np

F = np.float32


class State:
    """a slot's meter between batches: the clock, z1 and z2 of both sections, the partial energy and peak, per channel"""

    def __init__(self, channels):
        self.n = 0
        self.z = np.zeros((4, channels), F)          # z1 of section 0, z2 of section 0, z1 of section 1, z2 of section 1
        self.e = np.zeros(channels, F)
        self.pk = np.zeros(channels, F)

    def floats(self):
        """as the device keeps it: (channels, 6)"""
        return np.stack([self.z[0], self.z[1], self.z[2], self.z[3], self.e, self.pk], axis=1)


def as_x(pcm):
    """the rule's input of a block of PCM (N, C): float32 as it is, int16 times 2^-15 (exact)"""
    pcm = np.asarray(pcm)
    return pcm.astype(F) * F(2.0 ** -15) if pcm.dtype == np.int16 else pcm.astype(F)


def rule(pcm, hop, coeffs, state):
    """The rule over the samples pcm (N, C) of one slot from `state` (advanced in place): the records (n, C, 2) float32 that leave.
    Every operation is a float32 operation of its own (numpy rounds each elementwise result; nothing is fused), sample after sample;
    the channels run side by side."""
    x = as_x(pcm)
    k = np.asarray(coeffs, F).reshape(2, 5)
    z, out = state.z, []
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for t in range(len(x)):
            v = x[t]
            for i in (0, 1):
                b0, b1, b2, a1, a2 = k[i]
                y = (b0 * v) + z[2 * i]
                z[2 * i] = ((b1 * v) - (a1 * y)) + z[2 * i + 1]
                z[2 * i + 1] = (b2 * v) - (a2 * y)
                v = y
            state.e = state.e + (v * v)
            state.pk = np.maximum(state.pk, np.abs(x[t]))
            state.n += 1
            if state.n % hop == 0:
                out.append(np.stack([state.e, state.pk], axis=1))
                state.e, state.pk = np.zeros_like(state.e), np.zeros_like(state.pk)
    assert z.dtype == F and state.e.dtype == F and state.pk.dtype == F
    return np.array(out, F).reshape(len(out), x.shape[1], 2)


def hostile_coeffs(seed):
    """two stable sections (poles of radius 0.5 .. 0.98, any angle) with numerators of mixed signs and magnitudes around 1"""
    rng = np.random.default_rng(seed)
    k = np.zeros((2, 5), np.float64)
    for i in range(2):
        r, th = rng.uniform(0.5, 0.98), rng.uniform(0.0, np.pi)
        k[i, :3] = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.2, 1.6, 3)
        k[i, 3], k[i, 4] = -2.0 * r * np.cos(th), r * r
    k[0, 1], k[1, 0] = -abs(k[0, 1]), abs(k[1, 0])
    assert (k < 0).any() and (k > 0).any()
    return k.astype(F)


def design64(rate):
    """BS.1770's K-weighting re-derived at `rate` in float64, each value rounded to float32 once: (2, 5)"""
    k = np.zeros((2, 5), np.float64)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    k[0] = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    k[1] = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return k.astype(F)


# the standard's published 48 kHz coefficients
BS1770_48K = np.array([[1.5351248595869702, -2.6916961894063807, 1.19839281085285, -1.6906592931824103, 0.7324807742158501],
                       [1.0, -2.0, 1.0, -1.9900474548339797, 0.9900722503662099]], np.float64)


def integrate64(records, hop, weights=None):
    """(integrated LUFS or -inf, momentary LUFS of every block) of records (n_hops, C, 2), in float64: blocks of four hops one hop apart,
    the absolute gate at -70, the relative gate 10 LU below the kept blocks' mean"""
    e = np.asarray(records, np.float64)[:, :, 0]
    w = np.ones(e.shape[1]) if weights is None else np.asarray(weights, np.float64)
    if len(e) < 4:
        return -np.inf, np.zeros(0)
    four = e[:-3] + e[1:-2] + e[2:-1] + e[3:]
    z = (four / (4.0 * hop) * w[None, :]).sum(axis=1)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return -np.inf, l
    gate = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    keep &= l > gate
    return (-0.691 + 10.0 * np.log10(z[keep].mean()) if keep.any() else -np.inf), l
