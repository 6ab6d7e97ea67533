/*
 * aac.js_amd/js/resample.js — the resampling rule of include/aacgpu.h (aacg_pipeline_set_resample) on the host, bit for bit what the
 * device's aacg_pcm_resample_* kernels compute: for the decoders of a SharedEngine({ sampleRate }) that do not take the resident route,
 * so that every decoder of such an engine delivers the same rate whichever route it took — and the per-frame shares of a resident
 * batch's ragged output (counts), which the engine slices readChunk()'s arrays by.
 *
 * With the polyphase table h[L][T], output m = 0, 1, 2, ... of a channel since the stream began is, with i = floor(m M / L) and
 * p = (m M) mod L,
 *
 *   acc = fround(h[p][0] * x[i]);  acc = fround(acc + fround(h[p][t] * x[i - t]))  for t = 1 .. T-1, in that order;  x[j] = 0 for j < 0
 *
 * Math.fround after every product and every sum (mix.js says why that is the float operation's own rounding).  Every term is computed,
 * whatever its coefficient.  Float32Array: out = acc.  Int16Array: x is the sample as a number, out is acc rounded to nearest even and
 * saturated.  A frame of n input samples per channel at the clock N owns the outputs m with N <= i(m) < N + n: ceil((N + n) L / M) -
 * ceil(N L / M) of them; only N mod M counts, so the clock is kept modulo M.
 */
'use strict';

const toInt16 = require('./mix.js').toInt16;

function ceilDiv(a, b) { return Math.floor((a + b - 1) / b); }

/* the samples per channel that n input samples emit at the clock n0 (modulo M) */
function count(L, M, n0, n) { return ceilDiv((n0 + n) * L, M) - ceilDiv(n0 * L, M); }

/* spec: { L, M, taps, table: Float32Array(L * taps) }; one per stream: it carries the stream's clock and its last taps - 1 samples */
function Resampler(spec, channels) {
    const L = spec.L | 0, M = spec.M | 0, T = spec.taps | 0, C = channels | 0;
    if (L < 1 || M < 1 || T < 1 || C < 1 || !(spec.table instanceof Float32Array) || spec.table.length !== L * T) throw new RangeError('Resampler: { L, M, taps, table: Float32Array(L * taps) } and a channel count');
    this.L = L; this.M = M; this.T = T; this.C = C; this.table = spec.table;
    this.n0 = 0;
    this.hist = new Float64Array((T - 1) * C);             // the last T - 1 samples, oldest first (float values held in doubles)
}

Resampler.prototype.reset = function () { this.n0 = 0; this.hist.fill(0); };

/* how many samples per channel the next `n` input samples will emit */
Resampler.prototype.count = function (n) { return count(this.L, this.M, this.n0, n); };

/* pcm: Float32Array | Int16Array of n x channels interleaved samples, the stream's next -> a new array of pcm's type with the outputs
 * they own, count(n) x channels */
Resampler.prototype.push = function (pcm) {
    const L = this.L, M = this.M, T = this.T, C = this.C, h = this.table, fround = Math.fround;
    if (!(pcm instanceof Float32Array) && !(pcm instanceof Int16Array)) throw new TypeError('Resampler: pcm is a Float32Array or an Int16Array');
    if (pcm.length % C) throw new RangeError('Resampler: pcm holds n * channels samples');
    const n = pcm.length / C, i16 = pcm instanceof Int16Array, H = (T - 1) * C;
    const x = new Float64Array(H + pcm.length);
    x.set(this.hist, 0);
    x.set(pcm, H);
    const mLo = ceilDiv(this.n0 * L, M), nOut = ceilDiv((this.n0 + n) * L, M) - mLo;
    const out = i16 ? new Int16Array(nOut * C) : new Float32Array(nOut * C);
    for (let j = 0, to = 0; j < nOut; j++) {
        const u = (mLo + j) * M, i = Math.floor(u / L), p = u - i * L;
        const at = (i - this.n0 + T - 1) * C, row = p * T;     // x[i], channel 0, in the buffer: the history lies in front of the frame
        for (let c = 0; c < C; c++) {
            let acc = fround(h[row] * x[at + c]);
            for (let t = 1; t < T; t++) acc = fround(acc + fround(h[row + t] * x[at + c - t * C]));
            out[to++] = i16 ? toInt16(acc) : acc;
        }
    }
    if (H) this.hist.set(x.subarray(x.length - H));
    this.n0 = (this.n0 + n) % M;
    return out;
};

/* SharedEngine({ sampleRate }): the default table from the stream's rate to the engine's (addon.resampleDesign, aacg_resample_design);
 * null where the two are one */
function resolve(sampleRate, streamRate, addon, taps) {
    const out = sampleRate | 0;
    if (out < 1) throw new RangeError('SharedEngine: sampleRate is a rate in Hz');
    if (out === (streamRate | 0)) return null;
    return addon.resampleDesign(streamRate | 0, out, taps || 32);
}

module.exports = { Resampler: Resampler, count: count, resolve: resolve };
