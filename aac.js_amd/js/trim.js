/*
 * aac.js_amd/js/trim.js — the trim's rule of include/aacgpu.h (aacg_pipeline_set_trim) on the host, count for count what the device's
 * stage keeps: for decoders that do not take the resident route, so that both routes deliver the same chunks with the same lengths —
 * and the per-frame shares of a resident batch's kept range (counts: aacg_trim_counts' rule), which readChunk()'s arrays are sliced by.
 *
 * A stream has a window (skip S, keep K; K undefined or null: no end) and a position Q, in samples per channel of what the stage
 * receives.  A piece of n samples at Q keeps those with index in [Q, Q + n) n [S, S + K): one contiguous range, possibly none, and Q
 * advances by n.  A piece that keeps nothing delivers no chunk.  Numbers are exact below 2^53; S and a finite K are below 2^40.
 *
 * design: aacg_trim_design — the window at the stage's input for a window in samples of the stream's own rate and time, with the
 * limiter's 64 samples and a linear-phase table's (L taps - 1) / (2 L) input samples compensated: with A(t) = 2 L t + 128 L limiter +
 * L taps - 1, skip = ceil(A(skipIn) / 2M), keep = ceil(A(skipIn + keepIn) / 2M) - skip, residual = skip - A(skipIn) / 2M as the pair
 * (residualNum, residualDen).  Without a resampler pass L = M = 1 and taps = 0, and the filter term is left out.
 */
'use strict';

const LIMIT = 2 ** 40;

function checkWindow(skip, keep, who) {
    const finite = keep !== undefined && keep !== null;
    if (!Number.isInteger(skip) || skip < 0 || skip >= LIMIT || (finite && (!Number.isInteger(keep) || keep < 0 || keep >= LIMIT)))
        throw new RangeError(who + ': skip and a finite keep are integers in 0 .. 2^40 - 1');
    return finite ? keep : Infinity;
}

/* of n samples at position Q the window keeps { first, kept }: `kept` samples beginning at the piece's first-th */
function span(Q, skip, keep, n) {
    const end = (keep === undefined || keep === null) ? Infinity : skip + keep;
    const lo = Math.max(Q, skip), hi = Math.min(Q + n, end);
    return hi > lo ? { first: lo - Q, kept: hi - lo } : { first: 0, kept: 0 };
}

/* aacg_trim_counts: the share of the kept range that each of consecutive pieces of nIn[i] samples owns, the first at `position` */
function counts(position, skip, keep, nIn) {
    checkWindow(skip, keep, 'trim.counts');
    const firstOf = [], keptOf = [];
    for (let i = 0; i < nIn.length; i++) {
        const s = span(position, skip, keep, nIn[i]);
        firstOf.push(s.first); keptOf.push(s.kept);
        position += nIn[i];
    }
    return { firstOf, keptOf };
}

/* ceil(a / b) for integers 0 <= a < 2^53, b >= 1, without a rounded quotient */
function ceilDiv(a, b) { const r = a % b; return (a - r) / b + (r ? 1 : 0); }

/* aacg_trim_design; spec: { L, M, taps } of the resampler pass, or nothing */
function design(skipIn, keepIn, limiter, spec) {
    const keepFinite = checkWindow(skipIn, keepIn, 'trim.design');
    const L = spec ? spec.L | 0 : 1, M = spec ? spec.M | 0 : 1, taps = spec ? spec.taps | 0 : 0;
    if (L < 1 || M < 1 || L > 1024 || M > 1024 || taps < 0 || taps > 64) throw new RangeError('trim.design: L and M in 1..1024, taps in 0..64');
    const lat = (limiter ? 128 * L : 0) + (taps ? L * taps - 1 : 0), den = 2 * M;
    const a0 = 2 * L * skipIn + lat, skip = ceilDiv(a0, den);
    const keep = keepFinite === Infinity ? null : ceilDiv(2 * L * (skipIn + keepFinite) + lat, den) - skip;
    if (skip >= LIMIT || (keep !== null && keep >= LIMIT)) throw new RangeError('trim.design: the result is 2^40 or more');
    return { skip, keep, residualNum: skip * den - a0, residualDen: den };
}

/* One per stream on the parsing route: take(pcm) -> the kept part of the stream's next chunk (a view of pcm's type, n x channels
 * interleaved), or null where the chunk keeps nothing */
function Trimmer(channels, skip, keep) {
    this.C = channels | 0;
    if (this.C < 1) throw new RangeError('Trimmer: a channel count');
    this.set(skip || 0, keep);
}
Trimmer.prototype.set = function (skip, keep) { checkWindow(skip, keep, 'Trimmer'); this.skip = skip; this.keep = (keep === undefined) ? null : keep; this.position = 0; };
Trimmer.prototype.reset = function () { this.position = 0; };      // the window is the caller's setting and stays
Trimmer.prototype.take = function (pcm) {
    const n = pcm.length / this.C;
    const s = span(this.position, this.skip, this.keep, n);
    this.position += n;
    return s.kept ? pcm.subarray(s.first * this.C, (s.first + s.kept) * this.C) : null;
};

module.exports = { span, counts, design, Trimmer, LIMIT };
