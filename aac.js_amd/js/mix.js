/*
 * aac.js_amd/js/mix.js — the mix rule of include/aacgpu.h (aacg_pipeline_set_mix) on the host, bit for bit what the device's
 * aacg_pcm_mix_* kernels compute: for the decoders of a SharedEngine({ downmix }) that do not take the resident route, so that every
 * decoder of such an engine delivers the same O channels whichever route it took.
 *
 *   acc = fround(M[o][0] * x[0]);  acc = fround(acc + fround(M[o][c] * x[c]))  for c = 1 .. C-1, in that order
 *
 * Math.fround after every product and every sum: the product of two floats is exact in a double and the sum of two floats is rounded
 * there with 53 bits — more than twice 24 plus two, so rounding it again to float is the float operation's own rounding.  Every term
 * is computed, whatever its coefficient.  Float32Array: out = acc.  Int16Array: x is the sample as a number, out is acc rounded to
 * nearest even and saturated to [-32768, 32767].
 */
'use strict';

/* acc, a float held in a double, to the nearest integer, halves to the even one, saturated to int16 */
function toInt16(acc) {
    const f = Math.floor(acc), d = acc - f;               // exact: acc has 24 significant bits
    let r = d > 0.5 ? f + 1 : d < 0.5 ? f : (f % 2 === 0 ? f : f + 1);
    if (r > 32767) r = 32767;
    if (r < -32768) r = -32768;
    return r;
}

/* pcm: Float32Array | Int16Array of n x channels interleaved samples; matrix: Float32Array(outChannels * channels), row-major
 * -> a new array of pcm's type, n x outChannels */
function mix(pcm, channels, matrix, outChannels) {
    const C = channels | 0, O = outChannels | 0, fround = Math.fround;
    if (!(pcm instanceof Float32Array) && !(pcm instanceof Int16Array)) throw new TypeError('mix: pcm is a Float32Array or an Int16Array');
    if (C < 1 || O < 1 || !(matrix instanceof Float32Array) || matrix.length !== O * C || pcm.length % C) throw new RangeError('mix: matrix is a Float32Array(outChannels * channels), pcm n * channels samples');
    const n = pcm.length / C, i16 = pcm instanceof Int16Array, out = i16 ? new Int16Array(n * O) : new Float32Array(n * O);
    for (let t = 0, at = 0, to = 0; t < n; t++, at += C) {
        for (let o = 0, m = 0; o < O; o++, m += C) {
            let acc = fround(matrix[m] * pcm[at]);
            for (let c = 1; c < C; c++) acc = fround(acc + fround(matrix[m + c] * pcm[at + c]));
            out[to++] = i16 ? toInt16(acc) : acc;
        }
    }
    return out;
}

/* SharedEngine({ downmix }): 'stereo' | 'mono' (the standard matrix for `channels`: addon.mixStandard, aacg_mix_standard) or
 * { outChannels, matrix } -> { outChannels, matrix: Float32Array(outChannels * channels) } */
function resolve(downmix, channels, addon) {
    if (downmix === 'stereo' || downmix === 'mono') {
        const O = downmix === 'stereo' ? 2 : 1;
        return { outChannels: O, matrix: addon.mixStandard(channels, O, Math.SQRT1_2, true) };
    }
    if (!downmix || typeof downmix !== 'object') throw new TypeError('SharedEngine: downmix is \'stereo\', \'mono\' or { outChannels, matrix }');
    const O = downmix.outChannels | 0, matrix = downmix.matrix instanceof Float32Array ? downmix.matrix : new Float32Array(downmix.matrix || []);
    if ((O !== 1 && O !== 2) || matrix.length !== O * channels) throw new RangeError('SharedEngine: downmix.matrix has outChannels (1 or 2) x ' + channels + ' coefficients for a stream of ' + channels + ' channels');
    for (let i = 0; i < matrix.length; i++) if (!isFinite(matrix[i])) throw new RangeError('SharedEngine: downmix.matrix has a coefficient that is not finite');
    return { outChannels: O, matrix: matrix };
}

module.exports = { mix: mix, resolve: resolve, toInt16: toInt16 };
