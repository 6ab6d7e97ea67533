"""Per-block parity gates (test infrastructure): the engine's PCM against the oracle with correctly rounded FFT roots, one block
at a time.  A block is one (stream, frame, output channel): the 1024 samples of one channel of one frame, found from the unit
records (pcm_offset, n_out_ch).

Why per block: the batch-wide rms() of test_gpu_parity.py compares against the oracle as it follows the reference's float32
root recurrence (itself ~1.3e-6 from exact) at 5e-6 of the signal; one block wrong by 1e-4 in a batch of 8192 blocks, or a
systematic error of 3e-6 everywhere, passes it.  Against the exact-roots oracle the kernels sit far closer, and every block
is held to that.

Scale of a block: s = max(block RMS, 1e-2 x RMS of that stream's channel over the batch, 1e-9) for the RMS gate, and
s_peak = max(block peak, 1e-2 x that stream channel's peak, 1e-9) for the max gate; the second term keeps blocks where overlap
and head cancel (or a channel no unit covers, where the reference is exact zero) from a near-zero scale.

Thresholds, measured over every recipe of tests/test_route_matrix.py (two chained batches each; the int16 recipes through their
f32-output twins), worst block seen:
                                      lane emulator (CPU)          MI355X
  routes without optional stages:     RMS 2.22e-7  max 5.19e-7     RMS 2.09e-7  max 4.16e-7
  TNS / PNS / coupling elements:      RMS 5.40e-7  max 1.19e-6     RMS 5.46e-7  max 8.86e-7
  edges (tests/edge_cases.py, every band table; same gates):
    routes without optional stages:   RMS 3.78e-7  max 7.12e-7     RMS 3.78e-7  max 5.65e-7
    TNS / PNS / coupling elements:    RMS 1.04e-6  max 2.13e-6     RMS 1.04e-6  max 2.13e-6
The edge rows are higher because a block's scale is its own level while its first half is the previous frame's tail: after a
frame louder than itself (escape values, TNS gains) a block carries that frame's error.  The workload keeps single-band and
silent frames away from the seam where batch 1 follows batch 0 for that reason.
The excess of the second row is in the channels that carry TNS filters (their blocks twice the error of the others in the same
batch): the kernels run the all-pole filters through double-precision transition matrices, the oracle runs the reference's
float32 recursion, and the filter's gain amplifies the rounding.  Each gate is about three times the worst block seen.
"""
import numpy as np

TAU_RMS, TAU_MAX = 7e-7, 1.6e-6                 # routes without optional stages
TAU_RMS_STAGES, TAU_MAX_STAGES = 1.6e-6, 3.6e-6 # batches with TNS, PNS or coupling elements


def exact_reference(oracle, units, coeffs, meta, n_pcm, ov, **kw):
    """The oracle's PCM with correctly rounded FFT roots (orc_set_fft_roots; process-global inside the context), carrying ov."""
    with oracle.exact_fft_roots():
        return oracle.decode_batch(units, coeffs, meta, n_pcm, ov, **kw)


def block_index(units):
    """Sample indices of every block: int64 [n_blocks, 1024], and the (stream, output channel) of each block."""
    po, first = np.unique(np.asarray(units["pcm_offset"], np.int64), return_index=True)
    stream = np.asarray(units["stream"], np.int64)[first]
    n_out = np.asarray(units["n_out_ch"], np.int64)[first]
    idx, st, ch = [], [], []
    k = np.arange(1024, dtype=np.int64)
    for c in range(int(n_out.max())):
        sel = n_out > c
        idx.append(po[sel, None] + k[None, :] * n_out[sel, None] + c)
        st.append(stream[sel])
        ch.append(np.full(int(sel.sum()), c, np.int64))
    return np.concatenate(idx), np.concatenate(st), np.concatenate(ch)


def _scales(r, st, ch):
    """per block: (s, s_peak) from the reference's blocks r [n_blocks, 1024]"""
    blk_rms = np.sqrt(np.mean(r * r, axis=1))
    blk_peak = np.abs(r).max(axis=1)
    key = st * 64 + ch
    s_rms, s_peak = np.empty_like(blk_rms), np.empty_like(blk_peak)
    for k in np.unique(key):
        m = key == k
        s_rms[m] = np.sqrt(np.mean(r[m] * r[m]))
        s_peak[m] = np.abs(r[m]).max()
    return np.maximum.reduce([blk_rms, 1e-2 * s_rms, np.full_like(blk_rms, 1e-9)]), np.maximum.reduce([blk_peak, 1e-2 * s_peak, np.full_like(blk_peak, 1e-9)])


def block_errors(got, ref, units):
    """Per block: (RMS error / s, max |error| / s_peak), float64 [n_blocks] each.  Samples where both are NaN count as equal
    (the reference's out-of-range reads); NaN on one side only makes the block's errors infinite."""
    idx, st, ch = block_index(units)
    g = np.asarray(got, np.float64).ravel()[idx]
    r = np.asarray(ref, np.float64).ravel()[idx]
    both = np.isnan(g) & np.isnan(r)
    d = np.where(both, 0.0, g - r)
    d = np.where(np.isnan(d), np.inf, d)
    s, s_peak = _scales(np.where(np.isnan(r), 0.0, r), st, ch)
    return np.sqrt(np.mean(d * d, axis=1)) / s, np.abs(d).max(axis=1) / s_peak


def assert_blocks(got, ref, units, tau_rms=TAU_RMS, tau_max=TAU_MAX, what=""):
    """The per-block gate; returns the worst (RMS ratio, max ratio) for the record."""
    e_rms, e_max = block_errors(got, ref, units)
    worst = int(np.argmax(np.maximum(e_rms / tau_rms, e_max / tau_max)))
    assert np.all(e_rms <= tau_rms) and np.all(e_max <= tau_max), \
        "%s block %d of %d: RMS error %.3e x s (gate %.1e), max error %.3e x s_peak (gate %.1e)" % (
            what, worst, len(e_rms), e_rms[worst], tau_rms, e_max[worst], tau_max)
    return float(e_rms.max()), float(e_max.max())


def pcm16(x):
    """float PCM as the int16 seam stores it: round to nearest (even), saturate"""
    return np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def assert_blocks_int16(got, ref, units, tau_max=TAU_MAX, what=""):
    """int16 PCM against the exact-roots oracle: every sample of every block is the float reference rounded, or the neighbour
    where the reference lies within the float gate (tau_max x s_peak) of a rounding boundary — saturation included."""
    idx, st, ch = block_index(units)
    g = np.asarray(got).ravel()[idx].astype(np.float64)
    r = np.asarray(ref, np.float64).ravel()[idx]
    _, s_peak = _scales(r, st, ch)
    slack = tau_max * s_peak[:, None] * 32768.0
    lo = np.clip(np.rint(r * 32768.0 - slack), -32768, 32767)
    hi = np.clip(np.rint(r * 32768.0 + slack), -32768, 32767)
    bad = ~((g >= lo) & (g <= hi))
    assert not bad.any(), "%s %d samples in %d blocks off the rounded reference; first: block %d, got %d, reference x 32768 = %.4f" % (
        what, int(bad.sum()), int(bad.any(axis=1).sum()), int(np.nonzero(bad.any(axis=1))[0][0]),
        int(g[bad][0]), float((r * 32768.0)[bad][0]))
