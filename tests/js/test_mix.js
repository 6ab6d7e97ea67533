#!/usr/bin/env node
/*
 * tests/js/test_mix.js — the downmix under Node (tests/test_pcm_mix_js.py runs it).
 *   node tests/js/test_mix.js cpu       aac.js_amd/js/mix.js against the vectors the Python rule wrote (tests/golden/mix/vectors.json),
 *                                       bit for bit, Float32Array and Int16Array; what mix.resolve refuses
 *   node tests/js/test_mix.js standard  addon.mixStandard against the table in the same file (needs the addon and the library, no GPU)
 *   node tests/js/test_mix.js gpu       two 5.1 streams on SharedEngine({ resident: true, downmix: 'stereo' }): readChunk() equals, bit for
 *                                       bit, mix.js applied to the output of the same engine without downmix — on the resident route and
 *                                       for decoders forced onto the parsing route; and format.channelsPerFrame says 2
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const mixjs = require(path.join(root, 'aac.js_amd', 'js', 'mix.js'));
const vectors = JSON.parse(fs.readFileSync(path.join(root, 'tests', 'golden', 'mix', 'vectors.json')));
const mode = process.argv[2] || 'cpu';

function f32(bits) { return new Float32Array(Uint32Array.from(bits).buffer); }
function bitsOf(a) { return a instanceof Int16Array ? Array.from(a) : Array.from(new Uint32Array(a.buffer, a.byteOffset, a.length)); }

if (mode === 'cpu') {
    let n = 0;
    for (const c of vectors.cases) {
        const x = c.type === 'i16' ? Int16Array.from(c.x) : f32(c.x), want = c.want;
        const got = mixjs.mix(x, c.channels, f32(c.matrix), c.outChannels);
        assert.ok(c.type === 'i16' ? got instanceof Int16Array : got instanceof Float32Array);
        assert.deepStrictEqual(bitsOf(got), want, c.name + ': mix.js differs from the rule');
        n++;
    }
    assert.strictEqual(n, 48, 'every C x O: f32, int16 and the int16 halves');
    assert.deepStrictEqual([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 40000, -40000, 32767.5, -32768.5].map(mixjs.toInt16).map(function (v) { return v + 0; }), [0, 2, 2, 0, -2, -2, 32767, -32768, 32767, -32768]);
    const stub = { mixStandard: function (C, O) { return new Float32Array(C * O).fill(0.25); } };
    assert.strictEqual(mixjs.resolve('stereo', 6, stub).matrix.length, 12);
    assert.strictEqual(mixjs.resolve('mono', 6, stub).outChannels, 1);
    assert.strictEqual(mixjs.resolve({ outChannels: 2, matrix: new Float32Array(12) }, 6, stub).outChannels, 2);
    for (const bad of ['quad', 3, { outChannels: 3, matrix: new Float32Array(18) }, { outChannels: 2, matrix: new Float32Array(11) }, { outChannels: 1, matrix: Float32Array.from([1, NaN, 0, 0, 0, 0]) }])
        assert.throws(function () { mixjs.resolve(bad, 6, stub); }, /downmix/);
    assert.throws(function () { mixjs.mix(new Float64Array(6), 6, new Float32Array(6), 1); }, TypeError);
    console.log('mix cpu tests ok');
} else if (mode === 'standard') {
    const addon = host.loadAddon();
    for (const s of vectors.standard) {
        const got = addon.mixStandard(s.channels, s.outChannels, f32([s.gain])[0], !!s.normalise);
        assert.ok(got instanceof Float32Array);
        assert.deepStrictEqual(bitsOf(got), s.matrix, 'mixStandard(' + s.channels + ', ' + s.outChannels + ')');
    }
    assert.ok(vectors.standard.length >= 56);
    assert.deepStrictEqual(bitsOf(addon.mixStandard(6, 2)), bitsOf(addon.mixStandard(6, 2, Math.SQRT1_2, true)), 'the defaults');
    for (const bad of [[7, 2], [0, 2], [6, 3], [9, 1]]) assert.throws(function () { addon.mixStandard(bad[0], bad[1], 0.5, true); }, /aacg_mix_standard failed \(-1\)/);
    console.log('mix standard tests ok');
} else {
    const bytes = new Uint8Array(fs.readFileSync(path.join(root, 'tests', 'golden', 'streams', 'surround48.aac')));
    /* two decoders of the same 5.1 stream, the second one frame behind; parsing: forced onto the parsing route (a decoder that wants the
     * window shape carried on an engine made without it: SharedEngine.takesResident) */
    const run = function (downmix, parsing, outputKind) {
        const o = { resident: true, maxStreams: 4, maxChannels: 8, lookahead: 4, outputKind: outputKind | 0 };
        if (downmix) o.downmix = downmix;
        const shared = new host.SharedEngine(o), list = host.adts.frames(bytes);
        const decs = [0, 1].map(function (k) {
            const dec = new host.GpuAACDecoder({ frontend: new host.FrontEnd(), lookahead: 4, shared: shared, carryWindowShape: !!parsing });
            dec.init();
            const demux = new host.adts.AdtsDemuxer(function (event, payload) {
                if (event === 'format') Object.assign(dec.format, payload);
                else if (event === 'cookie') dec.setCookie(payload);
                else if (event === 'data') dec.feed(payload);
            });
            demux.push(bytes.subarray(list[k].offset));
            assert.strictEqual(!!dec.resident, !parsing, 'the route');
            return dec;
        });
        const out = decs.map(function (dec) {
            const frames = [];
            for (let f = dec.readChunk(); f; f = dec.readChunk()) frames.push(f.slice());
            return frames;
        });
        return { out: out, formats: decs.map(function (d) { return d.format.channelsPerFrame; }), launches: shared.launchCounts().launches };
    };
    const stereo = host.loadAddon().mixStandard(6, 2, Math.SQRT1_2, true);
    for (const leg of [{ parsing: false, kind: host.OUTPUT_F32 }, { parsing: false, kind: host.OUTPUT_I16 }, { parsing: true, kind: host.OUTPUT_F32 }]) {
        const plain = run(null, leg.parsing, leg.kind), mixed = run('stereo', leg.parsing, leg.kind);
        const custom = run({ outChannels: 1, matrix: Float32Array.from([1.3, -0.67, 1.04, -0.41, 1.78, -0.15]) }, leg.parsing, leg.kind);
        assert.deepStrictEqual(plain.formats, [6, 6]);
        assert.deepStrictEqual(mixed.formats, [2, 2]);
        assert.deepStrictEqual(custom.formats, [1, 1]);
        if (!leg.parsing) assert.ok(mixed.launches > 0 && mixed.launches === plain.launches, 'the resident route, launch for launch');
        for (let s = 0; s < 2; s++) {
            assert.ok(plain.out[s].length >= 4 - s && plain.out[s].length === mixed.out[s].length && plain.out[s].length === custom.out[s].length, 'frames');
            plain.out[s].forEach(function (frame, f) {
                assert.strictEqual(frame.length, 6 * 1024);
                assert.ok(leg.kind === host.OUTPUT_I16 && !leg.parsing ? frame instanceof Int16Array : frame instanceof Float32Array);
                assert.strictEqual(mixed.out[s][f].length, 2 * 1024);
                assert.deepStrictEqual(bitsOf(mixed.out[s][f]), bitsOf(mixjs.mix(frame, 6, stereo, 2)), 'stream ' + s + ' frame ' + f + ': downmix \'stereo\' is not mix.js over the unmixed output');
                assert.deepStrictEqual(bitsOf(custom.out[s][f]), bitsOf(mixjs.mix(frame, 6, Float32Array.from([1.3, -0.67, 1.04, -0.41, 1.78, -0.15]), 1)), 'stream ' + s + ' frame ' + f + ': a matrix of the caller\'s');
            });
            assert.ok(plain.out[s].some(function (frame) { return frame.some(function (v) { return v !== 0; }); }), 'the stream is music');
        }
        console.log('downmix ' + (leg.parsing ? 'parsing' : 'resident') + ' route, ' + (leg.kind === host.OUTPUT_I16 ? 'int16' : 'f32') + ': ' + plain.out[0].length + ' + ' + plain.out[1].length + ' frames equal mix.js over the unmixed engine\'s');
    }
    console.log('mix gpu tests ok');
}
