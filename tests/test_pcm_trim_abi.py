"""The trim's host-only part (include/aacgpu.h: aacg_trim_counts, aacg_trim_design; aac.js_amd/csrc/aacg_trim.cpp) and the binding's
surface: the symbols and the struct, the counts against the rule in Python integers, the design against fractions.Fraction, the refusals
that need no device, and the ALIGNMENT the design promises — on the CPU, with resample_kit's tables and rule: an impulse at source sample
skip_in + k comes out with its largest magnitude at index skip + k L / M - residual of the trimmed stream, within half an output sample.
No GPU."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest

import aacgpu
import resample_kit
import trim_kit as kit

INVALID_ARG = -1
SYMBOLS = ("aacg_pipeline_set_trim", "aacg_pipeline_set_stream_trim", "aacg_pipeline_stream_trim", "aacg_trim_counts", "aacg_trim_design")
ALL = aacgpu.TRIM_ALL


def test_library_exports_the_new_symbols(engine_lib):
    for name in SYMBOLS:
        assert name in aacgpu.ABI_SYMBOLS and hasattr(engine_lib, name), name
    T = aacgpu.TrimConfig
    assert [n for n, _ in T._fields_] == ["skip", "keep"] and (C.sizeof(T), T.keep.offset) == (16, 8)
    assert engine_lib.aacg_abi_version() == 6                              # new symbols only: no struct changed
    assert ALL == 2 ** 64 - 1


def test_null_handle_refusals(engine_lib):
    """every pipeline call answers a null handle without a device"""
    lib, v = aacgpu.load_library(), C.c_uint64(7)
    assert lib.aacg_pipeline_set_trim(None, C.byref(aacgpu.TrimConfig(0, ALL))) == INVALID_ARG
    assert lib.aacg_pipeline_set_stream_trim(None, 0, 0, ALL) == INVALID_ARG
    assert lib.aacg_pipeline_stream_trim(None, 0, C.byref(v), C.byref(v), C.byref(v)) == INVALID_ARG and v.value == 7


# windows that begin and end inside, on and outside a piece; keep 0 and ALL; positions beyond 2^32
PIECES = [1024, 1024, 341, 342, 1, 0, 1024, 2048]
WINDOWS = [(0, None), (0, 0), (2112, None), (1, 5000), (1024, 1024), (1023, 2), (1024, 0), (2048, 341), (2389, 343), (100, 10), (5804, None), (5803, 1), (9999, 5),
           (0, 5804), (0, 5805), (2731, 1), (2732, 1), (2731, 0), (kit.LIMIT - 1, kit.LIMIT - 1)]


@pytest.mark.parametrize("position", [0, 1, 1024, 2112, 2 ** 32 - 1000, 2 ** 32 + 12345, 2 ** 40 + 3])
def test_counts_are_the_rule(engine_lib, position):
    total = sum(PIECES)
    for skip, keep in WINDOWS + [(position + a, b) for a, b in ((0, None), (5, 1030), (1024, 1), (2389, 0), (total - 1, None), (total, None))]:
        if skip >= kit.LIMIT:
            continue
        first, kept = aacgpu.trim_counts(position, skip, keep, PIECES)
        want_first, want_kept = kit.counts(position, skip, keep, PIECES)
        assert first.tolist() == want_first and kept.tolist() == want_kept, (position, skip, keep)
        # the kept ranges are one contiguous range of the stream: behind its first piece every piece that keeps begins at its start
        keeps = [i for i, k in enumerate(want_kept) if k]
        assert all(want_first[i] == 0 for i in keeps[1:]) and all(want_first[i] + want_kept[i] == PIECES[i] for i in keeps[:-1])
        whole = kit.span(position, skip, keep, total)
        assert sum(want_kept) == whole[1]
    assert aacgpu.trim_counts(position, 0, None, [])[0].size == 0


def test_counts_refusals(engine_lib):
    lib = aacgpu.load_library()
    n_in, first, kept = np.array([1024, 1024], np.uint32), np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    args = lambda **kw: [kw.get("position", 0), kw.get("skip", 0), kw.get("keep", ALL), kw.get("n_in", n_in.ctypes.data), 2, kw.get("first", first.ctypes.data), kw.get("kept", kept.ctypes.data)]
    assert lib.aacg_trim_counts(*args()) == 0 and kept.tolist() == [1024, 1024]
    first[:], kept[:] = 77, 77
    for bad in (dict(n_in=None), dict(first=None), dict(kept=None), dict(skip=2 ** 40), dict(keep=2 ** 40), dict(skip=2 ** 63), dict(keep=ALL - 1), dict(position=2 ** 64 - 5)):
        assert lib.aacg_trim_counts(*args(**bad)) == INVALID_ARG, bad
    assert first.tolist() == [77, 77] and kept.tolist() == [77, 77], "a refusal of the arguments writes nothing"
    assert lib.aacg_trim_counts(*args(skip=2 ** 40 - 1, keep=2 ** 40 - 1)) == 0
    with pytest.raises(aacgpu.AacgError):
        aacgpu.trim_counts(0, 2 ** 40, None, [1024])


RATES = [(48000, 16000), (44100, 16000), (44100, 48000), (16000, 44100), (24000, 48000)]
TAPS = [8, 16, 32]
SKIPS = [0, 1024, 2112, 2113, 3000]


def test_design_is_the_formula(engine_lib):
    for (rin, rout), taps, skip_in, limiter in itertools.product(RATES, TAPS + [4, 64], SKIPS + [2 ** 32 + 17, 2 ** 39], (False, True)):
        L, M, _ = resample_kit.design(rin, rout, 4)
        if L * taps > 16384:
            continue
        for keep_in in (None, 0, 1, 1024, 44100 * 300, 2 ** 33 + 5):
            want = kit.design(skip_in, keep_in, limiter, L, M, taps)
            if want[0] >= kit.LIMIT or (want[1] is not None and want[1] >= kit.LIMIT):     # (2^39 samples at 441 / 160: a result at 2^40 or above is refused)
                with pytest.raises(aacgpu.AacgError):
                    aacgpu.trim_design(skip_in, keep_in, limiter, (L, M, taps))
                continue
            got = aacgpu.trim_design(skip_in, keep_in, limiter, (L, M, taps))
            assert got == want and isinstance(got[2], Fraction) and 0 <= got[2] < 1, (rin, rout, taps, skip_in, keep_in, limiter, got, want)
            # the issue's formula, spelled out: A(t) = 2 L t + 128 L limiter + L taps - 1
            A = lambda t: 2 * L * t + (128 * L if limiter else 0) + L * taps - 1
            assert got[0] == -((-A(skip_in)) // (2 * M)) and got[2] == got[0] - Fraction(A(skip_in), 2 * M)
            if keep_in is not None:
                assert got[1] == -((-A(skip_in + keep_in)) // (2 * M)) - got[0]
    # without a resampler pass the filter term is left out
    for skip_in, keep_in, limiter in itertools.product(SKIPS + [2 ** 40 - 65], (None, 0, 5000), (False, True)):
        assert aacgpu.trim_design(skip_in, keep_in, limiter) == (skip_in + (64 if limiter else 0), keep_in, Fraction(0)), (skip_in, keep_in, limiter)
    # a table given as such: its taps are its columns
    L, M, table = resample_kit.design(48000, 16000, 32)
    assert aacgpu.trim_design(2112, None, True, (L, M, table)) == aacgpu.trim_design(2112, None, True, (L, M, 32)) == kit.design(2112, None, True, 1, 3, 32)


def test_design_refusals(engine_lib):
    lib = aacgpu.load_library()
    out = [C.c_uint64(7) for _ in range(4)]
    refs = [C.byref(v) for v in out]
    assert lib.aacg_trim_design(2112, ALL, 1, 1, 3, 32, *refs) == 0 and out[1].value == ALL and out[3].value == 6
    assert lib.aacg_trim_design(2112, 5, 0, 1, 1, 0, refs[0], refs[1], None, None) == 0 and (out[0].value, out[1].value) == (2112, 5)      # the residual is optional
    for v in out:
        v.value = 7
    for bad in ((2 ** 40, ALL, 0, 1, 1, 0), (0, 2 ** 40, 0, 1, 1, 0), (0, ALL, 0, 0, 1, 0), (0, ALL, 0, 1, 0, 0), (0, ALL, 0, 1025, 1, 0), (0, ALL, 0, 1, 1025, 0), (0, ALL, 0, 1, 1, 65),
                (2 ** 40 - 1, ALL, 1, 1, 1, 0),              # the result would be 2^40 + 63
                (2 ** 39, ALL, 0, 8, 1, 4)):                 # ... and 2^42
        assert lib.aacg_trim_design(*bad, *refs) == INVALID_ARG, bad
    assert lib.aacg_trim_design(0, ALL, 0, 1, 1, 0, None, refs[1], refs[2], refs[3]) == INVALID_ARG
    assert lib.aacg_trim_design(0, ALL, 0, 1, 1, 0, refs[0], None, refs[2], refs[3]) == INVALID_ARG
    assert [v.value for v in out] == [7] * 4, "a refusal writes nothing"
    with pytest.raises(aacgpu.AacgError):
        aacgpu.trim_design(2 ** 40, None)


@pytest.mark.parametrize("rates", RATES, ids=["%d-%d" % r for r in RATES])
def test_an_impulse_lands_where_the_design_says(engine_lib, rates):
    """the alignment: through resample_kit.resample_rule with resample_kit.design's tables, the impulse at source sample skip_in + k —
    64 later where a limiter delays it — has its largest magnitude at skip + k L / M - residual of the received stream, within half an
    output sample.  The worst case is half a sample exactly: two equal neighbours, either of which may be the largest"""
    worst = Fraction(0)
    for taps in TAPS:
        L, M, table = resample_kit.design(rates[0], rates[1], taps)
        for skip_in, k, limiter in itertools.product(SKIPS, (0, 1, 37, 500), (False, True)):
            skip, keep, residual = aacgpu.trim_design(skip_in, None, limiter, (L, M, table))
            at = skip_in + k + (64 if limiter else 0)
            x = np.zeros((at + 2 * taps + 8, 1), np.float32)
            x[at] = 1.0
            y = np.abs(resample_kit.resample_rule(x, L, M, table)[:, 0])
            want = skip + Fraction(k * L, M) - residual
            peaks = np.flatnonzero(y == y.max())
            off = min(abs(Fraction(int(p)) - want) for p in peaks)
            print("%d -> %d, %d taps, skip_in %d, k %d, limiter %d: peak at %s, wanted %s (%.4f off)" % (rates + (taps, skip_in, k, limiter, peaks.tolist(), float(want), float(off))))
            assert float(off) <= 0.5 + 1e-9, (rates, taps, skip_in, k, limiter, peaks.tolist(), float(want))
            worst = max(worst, off)
            # ... which is index k L / M - residual of what the trim keeps
            assert 0 <= residual < 1 and keep is None
    assert worst <= Fraction(1, 2)
