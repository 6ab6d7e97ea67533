"""What the limiter tests share (tests/test_pcm_limiter_*.py): the rule of include/aacgpu.h (aacg_pipeline_set_limiter) in numpy float32,
twice — `whole` over a stream's whole sample history at once (the peaks, the targets and the output as array operations, only the node
gains as a loop), and `rule`, block after block from a State that is carried across calls.  The two share no line and must agree bit for
bit (tests/test_pcm_limiter_emu.py).  Nothing here shares code with the kernel (aac.js_amd/csrc/aacg_pcm_limit.h).

The rule, per block xk of 64 x C samples of a slot, with the held block xh, the node gain a0 and the target th:
    p = max |xk| (from +0, a NaN ignored);  tk = (G p > c) ? c / p : G;  u = a0 + (r (G - a0));  a1 = min(min(th, tk), u);  d = a1 - a0
    out[i] = (a0 + (d (i / 64))) xh[i];  xh = xk;  a0 = a1;  th = tk
every operation a float32 operation of its own; a fresh slot holds zeros with a0 = th = G."""
import numpy as np

F = np.float32
B = 64
W = (np.arange(B, dtype=np.float64) / B).astype(F)          # i / 64, exact


def as_x(pcm):
    """the rule's input of PCM (N, C): float32 as it is, int16 times 2^-15 (exact)"""
    pcm = np.asarray(pcm)
    assert pcm.dtype in (np.float32, np.int16) and pcm.ndim == 2 and len(pcm) % B == 0
    return pcm.astype(F) * F(2.0 ** -15) if pcm.dtype == np.int16 else pcm


def as_pcm(out, dtype):
    """the rule's output as the pipeline's elements: float32 as computed, int16 out x 2^15 rounded to nearest even and saturated"""
    if dtype == np.int16:
        with np.errstate(invalid="ignore"):
            return np.clip(np.rint(out * F(32768.0)), -32768, 32767).astype(np.int16)
    return out


class State:
    """a slot's limiter between batches: the held block, the node gain at its start and its target (None: fresh, they take G).
    targets: (tk, G) of every block that has arrived, for the tests that must know whether the limiter engaged"""

    def __init__(self, channels):
        self.xh = np.zeros((B, channels), F)
        self.a0 = self.th = None
        self.targets = []

    def floats(self):
        """as the device keeps it: a0, th, two unused floats, then the held block"""
        return np.concatenate([np.array([self.a0, self.th, 0, 0], F), self.xh.reshape(-1)])

    def engaged(self):
        """(blocks with tk < G, blocks with tk == G)"""
        return sum(1 for tk, G in self.targets if tk < G), sum(1 for tk, G in self.targets if tk == G)


def rule(pcm, G, c, r, state):
    """The rule over the samples pcm (N, C) of one slot from `state` (advanced in place), with the gain G for all of them: what leaves,
    (N, C) of pcm's dtype.  Block after block, every operation a float32 scalar or elementwise operation of its own."""
    x = as_x(pcm)
    G, c, r = F(G), F(c), F(r)
    if state.a0 is None:
        state.a0 = state.th = G
    out = np.zeros_like(x)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        for k in range(len(x) // B):
            xk = x[k * B:(k + 1) * B]
            p = F(0.0)
            for v in np.abs(xk).reshape(-1):
                p = np.fmax(p, v)                                   # fmaxf: a NaN is ignored
            tk = c / p if G * p > c else G
            u = state.a0 + (r * (G - state.a0))
            a1 = np.fmin(np.fmin(state.th, tk), u)
            d = a1 - state.a0
            gain = state.a0 + (d * W)
            out[k * B:(k + 1) * B] = gain[:, None] * state.xh
            state.xh, state.a0, state.th = xk.copy(), a1, tk
            state.targets.append((float(tk), float(G)))
            assert all(type(v) is F for v in (p, tk, u, a1, d)) and gain.dtype == F
    return as_pcm(out, np.asarray(pcm).dtype)


def whole(pcm, G, c, r):
    """The rule over a stream's WHOLE history pcm (N, C) from a fresh slot.  G: one gain, or one per block (a gain that was changed
    between batches).  Returns (what leaves, (N, C) of pcm's dtype; the targets tk per block; the gains G per block)."""
    x = as_x(pcm)
    n = len(x) // B
    G = np.broadcast_to(np.asarray(G, F), (n,)).copy()
    c, r = F(c), F(r)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        p = np.fmax.reduce(np.abs(x).reshape(n, -1), axis=1, initial=F(0.0))
        over = G * p > c
        t = np.where(over, c / np.where(over, p, F(1.0)), G).astype(F)
        a = np.zeros(n + 1, F)                                      # the node gains: a[k] at the start of the block that leaves as block k arrives
        a[0] = G[0]
        th = G[0]
        for k in range(n):
            u = a[k] + (r * (G[k] - a[k]))
            a[k + 1] = min(min(th, t[k]), u)                        # (none of them is a NaN)
            th = t[k]
        held = np.concatenate([np.zeros((B, x.shape[1]), F), x[:len(x) - B]]).reshape(n, B, -1)
        d = a[1:] - a[:-1]
        gain = a[:-1, None] + (d[:, None] * W[None, :])
        out = (gain[:, :, None] * held).reshape(x.shape)
    assert p.dtype == F and t.dtype == F and gain.dtype == F and out.dtype == F
    return as_pcm(out, np.asarray(pcm).dtype), t, G


def bursts(n, channels, dtype, seed, level=0.05, burst=0.9):
    """noise at `level` of full scale with a few bursts up to `burst`, (n, channels): with a ceiling between the two and G = 1 some
    blocks have tk < G and some tk = G"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-level, level, (n, channels))
    for at in rng.integers(0, max(1, n - 40), max(2, n // 700)):
        x[at:at + 40] = rng.uniform(-burst, burst, (min(40, n - at), channels))
    if dtype == np.int16:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    return x.astype(F)
