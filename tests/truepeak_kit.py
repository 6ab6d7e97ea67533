"""What the true-peak stage's tests share (tests/test_pcm_truepeak_*.py): the rule of include/aacgpu.h (aacg_pipeline_set_true_peak) in numpy
float32 — the accumulation is resample_kit's restatement of the resampler's rule with M = 1 — once over a whole history and once hop by
hop from a carried state, which must agree bit for bit (self_check).  No code is shared with the kernel."""
import numpy as np

import resample_kit

NAN_ABOVE = np.uint32(0x7f800000)


def to_float(x):
    """the meter's input: float32 as it is, int16 times 2^-15 (exact)"""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.int16)
    return x if x.dtype == np.float32 else x.astype(np.float32) * np.float32(2.0 ** -15)


def magnitudes(xf, table):
    """xf (N, C) float32 with x[j] = 0 for j < 0 -> (N, C) uint32: per input sample the bits of the largest |acc| over the L phases, any
    NaN above every number.  acc = h[p][0] x[i], then acc = acc + (h[p][t] x[i - t]), t = 1 .. T-1: resample_rule with M = 1 gives output
    m = i L + p."""
    h = np.ascontiguousarray(table, np.float32)
    L = h.shape[0]
    acc = resample_kit.resample_rule(np.ascontiguousarray(xf, np.float32), L, 1, h)
    assert acc.dtype == np.float32 and acc.shape == (len(xf) * L, xf.shape[1])
    bits = np.ascontiguousarray(acc).view(np.uint32) & np.uint32(0x7fffffff)
    return bits.reshape(len(xf), L, xf.shape[1]).max(axis=1) if len(xf) else np.zeros((0, xf.shape[1]), np.uint32)


def as_records(bits):
    """(n, C) uint32 -> float32 records, every NaN the one quiet NaN (the tests compare NaN-ness, not payloads)"""
    out = np.ascontiguousarray(bits, np.uint32).copy()
    out[out > NAN_ABOVE] = 0x7fc00000
    return out.view(np.float32)


def rule_whole(x, hop, table):
    """The rule over a whole stream since its reset: x (N, C) float32 or int16 -> (N // hop, C) float32 records, and the partial
    maximum of the samples behind the last whole hop as (C,) float32."""
    xf = to_float(x)
    m = magnitudes(xf, table)
    n = len(xf) // hop
    rec = m[:n * hop].reshape(n, hop, xf.shape[1]).max(axis=1) if n else np.zeros((0, xf.shape[1]), np.uint32)
    rest = m[n * hop:]
    return as_records(rec), as_records(rest.max(axis=0) if len(rest) else np.zeros(xf.shape[1], np.uint32))


class State:
    """what a slot carries: the clock, the last T - 1 input samples as floats, the partial maximum as bits"""

    def __init__(self, channels, taps):
        self.n = 0
        self.hist = np.zeros((taps - 1, channels), np.float32)
        self.partial = np.zeros(channels, np.uint32)

    def words(self):
        """the state as the device keeps it: (T - 1) x C floats of history, then C floats of partial maximum"""
        return np.concatenate([self.hist.reshape(-1), as_records(self.partial)])


def rule(x, hop, table, state):
    """The rule from a carried state, hop by hop: x (N, C) of the slot's next samples -> the records these samples complete,
    (count, C) float32; the state moves on."""
    xf = to_float(x)
    T = np.asarray(table).shape[1]
    assert state.hist.shape == (T - 1, xf.shape[1])
    both = np.concatenate([state.hist, xf])
    m = magnitudes(both, table)[T - 1:]                  # the samples of the history were measured when they arrived
    out, at = [], 0
    while at < len(xf):
        take = min(hop - state.n % hop, len(xf) - at)
        state.partial = np.maximum(state.partial, m[at:at + take].max(axis=0))
        state.n += take
        at += take
        if state.n % hop == 0:
            out.append(state.partial)
            state.partial = np.zeros(xf.shape[1], np.uint32)
    state.hist = both[len(both) - (T - 1):].copy()
    return as_records(np.array(out, np.uint32).reshape(len(out), xf.shape[1]))


def same_records(got, want, what):
    """bit for bit where the rule gives a number, a NaN where it gives a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    wrong = np.argwhere(np.where(np.isnan(want), ~np.isnan(got), g != w))
    assert wrong.size == 0, "%s: differs from the rule at %d of %d values, first at %s: %r against %r" % (
        what, len(wrong), got.size, wrong[0], got[tuple(wrong[0])], want[tuple(wrong[0])])


def mixed_table(L, T, seed=5):
    """a table of mixed signs and magnitudes, not a filter: every rounding shows (resample_kit.hostile_table)"""
    return resample_kit.hostile_table(L, T, seed)


def design(phases, taps, rolloff=0.95, beta=5.0):
    """aacg_true_peak_design restated in float64 through resample_kit.design: rates 1 -> phases"""
    L, M, table = resample_kit.design(1, phases, taps, rolloff, beta)
    assert (L, M) == (phases, 1)
    return table


def self_check(x, hop, table, cuts):
    """the rule twice: over the whole of x, and from a carried state over x cut at `cuts` — the same records and the same state"""
    want, partial = rule_whole(x, hop, table)
    S = State(x.shape[1], np.asarray(table).shape[1])
    got = [rule(part, hop, table, S) for part in np.split(x, cuts)]
    same_records(np.concatenate(got), want, "carried against whole")
    same_records(as_records(S.partial), partial, "carried against whole, the partial maximum")
    T = np.asarray(table).shape[1]
    tail = np.concatenate([np.zeros((T - 1, x.shape[1]), np.float32), to_float(x)])[len(x):]
    assert (S.hist.view(np.uint32) == tail.view(np.uint32)).all() and S.n == len(x)
    return want
