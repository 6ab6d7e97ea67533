"""What the trim's tests share (tests/test_pcm_trim_*.py, tests/test_pipe_exit_trim.py): the rule of include/aacgpu.h (aacg_pipeline_set_trim)
in Python integers, the design formula in fractions.Fraction, and the tile of the kernel's items.  A plain module like resample_kit.py."""
from fractions import Fraction

ALL = None                  # a window without an end (AACG_TRIM_ALL in the C ABI)
LIMIT = 1 << 40             # skip and a finite keep are below it
TILE = 512                  # AACG_TRIM_TILE: samples of an item


def span(Q, skip, keep, n_in):
    """of n_in samples at position Q the window keeps (first, n_keep): the samples with index in [Q, Q + n_in) n [skip, skip + keep)"""
    lo = max(Q, skip)
    hi = Q + n_in if keep is ALL else min(Q + n_in, skip + keep)
    return (lo - Q, hi - lo) if hi > lo else (0, 0)


def counts(position, skip, keep, n_in):
    """aacg_trim_counts: ([first_of], [kept_of]) of consecutive pieces"""
    first, kept = [], []
    for n in n_in:
        f, k = span(position, skip, keep, n)
        first.append(f)
        kept.append(k)
        position += n
    return first, kept


def ceil_frac(x):
    return -((-x.numerator) // x.denominator)


def place(t, limiter, L, M, taps):
    """where input sample t of a stream comes out, in output samples, as a Fraction: behind the limiter's 64 samples and a linear-phase
    table's (L taps - 1) / (2 L) input samples, at L / M times the rate"""
    delay = Fraction(64 if limiter else 0) + (Fraction(L * taps - 1, 2 * L) if taps else 0)
    return (Fraction(t) + delay) * L / M


def design(skip_in, keep_in, limiter, L, M, taps):
    """aacg_trim_design: (skip, keep, residual)"""
    at = place(skip_in, limiter, L, M, taps)
    skip = ceil_frac(at)
    keep = ALL if keep_in is ALL else ceil_frac(place(skip_in + keep_in, limiter, L, M, taps)) - skip
    return skip, keep, skip - at


def sliced(x, windows):
    """a slot's whole received stream x (samples, channels) under a list of (from sample, skip, keep): the position restarts at each
    `from` -> the kept samples, concatenated"""
    import numpy as np
    out = []
    for k, (start, skip, keep) in enumerate(windows):
        end = windows[k + 1][0] if k + 1 < len(windows) else len(x)
        first, n = span(0, skip, keep, end - start)
        out.append(x[start + first:start + first + n])
    return np.concatenate(out) if out else x[:0]
