"""What the tests of the limiter's true-peak detector share (tests/test_pcm_limiter_tp_*.py): the rule of include/aacgpu.h
(aacg_pipeline_set_limiter_true_peak) in numpy float32, twice — `whole` over a stream's whole sample history at once (the detector from
truepeak_kit.magnitudes, the peaks, the targets and the output as array operations, only the node gains as a loop), and `rule`, block
after block from a State that is carried across calls, with the filter spelled out tap by tap.  The two share no line and must agree bit
for bit (tests/test_pcm_limiter_tp_emu.py).  Nothing here shares code with the kernel (aac.js_amd/csrc/aacg_pcm_limit_tp.h).

The rule, with the table h[L][T], D = T / 2, x the limiter's input since the slot's reset (zeros in front) and z[j] = x[j - D]; for block k
(j = 64 k .. 64 k + 63):
    ps = max |z[j][ch]|;  acc = h[ph][0] x[j], acc = acc + (h[ph][t] x[j - t]) for t = 1 .. T-1;  pt = max |acc_ph[j][ch]|;  p = fmax(ps, pt)
every maximum an fmax from +0 in which a NaN is ignored; then limiter_kit's rule with xk := block k of z and this p:
    tk = (G p > c) ? c / p : G;  u = a0 + (r (G - a0));  a1 = min(min(th, tk), u);  d = a1 - a0;  out[i] = (a0 + (d (i / 64))) xh[i];
    xh = xk;  a0 = a1;  th = tk
every operation a float32 operation of its own; a fresh slot holds zeros for xh and the T - 1 samples of history, with a0 = th = G."""
import numpy as np

import limiter_kit
import truepeak_kit

F = np.float32
B = limiter_kit.B
W = limiter_kit.W
as_x, as_pcm, bursts = limiter_kit.as_x, limiter_kit.as_pcm, limiter_kit.bursts


def delay(table):
    """the stage's delay in samples: 64 + T / 2"""
    return B + np.asarray(table).shape[1] // 2


def peaks_whole(x, table):
    """x (N, C) float32, N a multiple of 64 -> (the delayed path z (N, C), p per block (N / 64,) float32)"""
    h = np.ascontiguousarray(table, F)
    D, n = h.shape[1] // 2, len(x) // B
    z = np.concatenate([np.zeros((D, x.shape[1]), F), x[:len(x) - D]])
    ps = np.fmax.reduce(np.abs(z).reshape(n, -1), axis=1, initial=F(0.0))
    bits = truepeak_kit.magnitudes(x, h)                                # per sample and channel, the largest |acc| as bits, a NaN above every number
    bits = np.where(bits > truepeak_kit.NAN_ABOVE, np.uint32(0), bits)  # ... and ignored here
    pt = np.ascontiguousarray(bits).view(F).reshape(n, -1).max(axis=1)
    p = np.fmax(ps, pt)
    assert z.dtype == F and p.dtype == F and not np.isnan(p).any()
    return z, p


def whole(pcm, G, c, r, table):
    """The rule over a stream's WHOLE history pcm (N, C) from a fresh slot.  G: one gain, or one per block.  Returns (what leaves, (N, C)
    of pcm's dtype; the targets tk per block; the gains G per block; the detector's p per block)."""
    x = as_x(pcm)
    n = len(x) // B
    G = np.broadcast_to(np.asarray(G, F), (n,)).copy()
    c, r = F(c), F(r)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        z, p = peaks_whole(x, table)
        over = G * p > c
        t = np.where(over, c / np.where(over, p, F(1.0)), G).astype(F)
        a = np.zeros(n + 1, F)
        a[0] = G[0]
        th = G[0]
        for k in range(n):
            u = a[k] + (r * (G[k] - a[k]))
            a[k + 1] = min(min(th, t[k]), u)                            # (none of them is a NaN)
            th = t[k]
        held = np.concatenate([np.zeros((B, x.shape[1]), F), z[:len(z) - B]]).reshape(n, B, -1)
        d = a[1:] - a[:-1]
        gain = a[:-1, None] + (d[:, None] * W[None, :])
        out = (gain[:, :, None] * held).reshape(x.shape)
    assert t.dtype == F and gain.dtype == F and out.dtype == F
    return as_pcm(out, np.asarray(pcm).dtype), t, G, p


class State:
    """a slot between batches: the held block of z, the node gain at its start and its target (None: fresh, they take G), and the last
    T - 1 samples of x.  targets: (tk, G, p) of every block that has arrived"""

    def __init__(self, channels, taps):
        self.xh = np.zeros((B, channels), F)
        self.hist = np.zeros((taps - 1, channels), F)
        self.a0 = self.th = None
        self.targets = []

    def floats(self):
        """the plain limiter's state as the device keeps it: a0, th, two unused floats, then the held block"""
        return np.concatenate([np.array([self.a0, self.th, 0, 0], F), self.xh.reshape(-1)])

    def history(self):
        """the second buffer: (T - 1) x C floats, the oldest sample first"""
        return self.hist.reshape(-1).copy()

    def engaged(self):
        """(blocks with tk < G, blocks with tk == G)"""
        return sum(1 for tk, G, p in self.targets if tk < G), sum(1 for tk, G, p in self.targets if tk == G)


def rule(pcm, G, c, r, table, state):
    """The rule over the samples pcm (N, C) of one slot from `state` (advanced in place), with the gain G for all of them: what leaves,
    (N, C) of pcm's dtype.  Block after block; the filter tap after tap, every product and every sum a float32 operation of its own."""
    x = as_x(pcm)
    h = np.asarray(table, F)
    L, T = h.shape
    D = T // 2
    G, c, r = F(G), F(c), F(r)
    if state.a0 is None:
        state.a0 = state.th = G
    out = np.zeros_like(x)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        for k in range(len(x) // B):
            seen = np.concatenate([state.hist, x[k * B:(k + 1) * B]])   # x[64 k - (T - 1)] .. x[64 k + 63]
            zk = seen[T - 1 - D:T - 1 - D + B].copy()
            p = np.fmax.reduce(np.abs(zk).reshape(-1), initial=F(0.0))  # fmax: a NaN is ignored
            for ph in range(L):
                acc = h[ph, 0] * seen[T - 1:]
                for t in range(1, T):
                    acc = acc + (h[ph, t] * seen[T - 1 - t:T - 1 - t + B])
                assert acc.dtype == F and acc.shape == zk.shape
                p = np.fmax(p, np.fmax.reduce(np.abs(acc).reshape(-1), initial=F(0.0)))
            tk = c / p if G * p > c else G
            u = state.a0 + (r * (G - state.a0))
            a1 = np.fmin(np.fmin(state.th, tk), u)
            d = a1 - state.a0
            gain = state.a0 + (d * W)
            out[k * B:(k + 1) * B] = gain[:, None] * state.xh
            state.xh, state.a0, state.th, state.hist = zk, a1, tk, seen[B:].copy()
            state.targets.append((float(tk), float(G), float(p)))
            assert all(type(v) is F for v in (p, tk, u, a1, d)) and gain.dtype == F
    return as_pcm(out, np.asarray(pcm).dtype)


def true_peak(pcm, table, first=0):
    """the true peak of delivered PCM (N, C) read with `table`, over the samples from `first` on: the largest |acc| as a float64"""
    x = as_x(pcm)
    bits = truepeak_kit.magnitudes(x, np.ascontiguousarray(table, F))[first:]
    assert not (bits > truepeak_kit.NAN_ABOVE).any()
    return float(np.ascontiguousarray(bits).view(F).max())


def sine_quarter(n, channels=1, amplitude=1.0):
    """a sine at fs / 4 with 45 degrees of phase: the samples are +-amplitude / sqrt 2, the true peak is the amplitude"""
    v = amplitude * np.sin(2.0 * np.pi * 0.25 * np.arange(n) + np.pi / 4.0)
    return np.repeat(v[:, None], channels, axis=1).astype(F)


def stepped_sweep(n, lo=0.2, hi=0.45, quiet=0.3, loud=1.3, steps=16):
    """a sine whose frequency steps from lo to hi of the rate, alternately quiet and loud, phase-continuous, one channel"""
    per = n // steps
    f = np.repeat(np.linspace(lo, hi, steps), per)
    amp = np.repeat(np.where(np.arange(steps) % 2 == 0, quiet, loud), per)
    phase = 2.0 * np.pi * np.cumsum(f)
    v = np.zeros(n)
    v[:len(f)] = amp * np.sin(phase)
    return v[:, None].astype(F)
