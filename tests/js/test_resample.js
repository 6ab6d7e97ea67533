#!/usr/bin/env node
/*
 * tests/js/test_resample.js — the resampler under Node (tests/test_pcm_resample_js.py runs it).
 *   node tests/js/test_resample.js cpu <vectors.json>   aac.js_amd/js/resample.js against vectors the Python rule wrote (made by the test
 *                                       into a temporary file): frame after frame through one Resampler, bit for bit, Float32Array and
 *                                       Int16Array, with the per-frame counts
 *   node tests/js/test_resample.js design               addon.resampleDesign: the ratio reduced, the table's size, what it refuses (needs
 *                                       the addon and the library, no GPU)
 *   node tests/js/test_resample.js gpu  two stereo streams on SharedEngine({ resident: true, sampleRate: 16000 }): readChunk() equals, bit
 *                                       for bit, resample.js applied frame by frame to the output of the same engine without sampleRate —
 *                                       on the resident route and for decoders forced onto the parsing route —, with each chunk's
 *                                       length the frame's share, and format.sampleRate says 16000
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const rs = require(path.join(root, 'aac.js_amd', 'js', 'resample.js'));
const mode = process.argv[2] || 'cpu';

function f32(bits) { return new Float32Array(Uint32Array.from(bits).buffer); }
function bitsOf(a) { return a instanceof Int16Array ? Array.from(a) : Array.from(new Uint32Array(a.buffer, a.byteOffset, a.length)); }

if (mode === 'cpu') {
    const vectors = JSON.parse(fs.readFileSync(process.argv[3]));
    let n = 0;
    for (const c of vectors.cases) {
        const x = c.type === 'i16' ? Int16Array.from(c.x) : f32(c.x);
        const r = new rs.Resampler({ L: c.L, M: c.M, taps: c.taps, table: f32(c.table) }, c.channels);
        const got = [], counts = [];
        for (let at = 0; at < x.length; at += c.frame * c.channels) {
            const want = r.count(c.frame), out = r.push(x.subarray(at, at + c.frame * c.channels));
            assert.ok(c.type === 'i16' ? out instanceof Int16Array : out instanceof Float32Array);
            assert.strictEqual(out.length, want * c.channels, c.name + ': count() against push()');
            counts.push(want);
            got.push.apply(got, bitsOf(out));
        }
        assert.deepStrictEqual(counts, c.counts, c.name + ': the frames\' shares');
        assert.deepStrictEqual(got, c.want, c.name + ': resample.js differs from the rule');
        r.reset();
        assert.deepStrictEqual(bitsOf(r.push(x.subarray(0, c.frame * c.channels))), c.want.slice(0, c.counts[0] * c.channels), c.name + ': after a reset');
        n++;
    }
    assert.strictEqual(n, vectors.expect, 'every case');
    assert.strictEqual(rs.count(1, 3, 0, 1024), 342); assert.strictEqual(rs.count(1, 3, 1, 1024), 341); assert.strictEqual(rs.count(160, 441, 440, 1024), 372);
    assert.throws(function () { new rs.Resampler({ L: 1, M: 3, taps: 4, table: new Float32Array(3) }, 2); }, RangeError);
    assert.throws(function () { new rs.Resampler({ L: 1, M: 3, taps: 4, table: new Float32Array(4) }, 2).push(new Float64Array(4)); }, TypeError);
    const stub = { resampleDesign: function (a, b, t) { return { L: 1, M: 3, taps: t, table: new Float32Array(t) }; } };
    assert.strictEqual(rs.resolve(48000, 48000, stub), null);
    assert.strictEqual(rs.resolve(16000, 48000, stub).taps, 32);
    assert.throws(function () { rs.resolve(0, 48000, stub); }, RangeError);
    console.log('resample cpu tests ok');
} else if (mode === 'design') {
    const host = require(path.join(root, 'aac.js_amd', 'js'));
    const addon = host.loadAddon();
    const d = addon.resampleDesign(44100, 16000, 32);
    assert.strictEqual(d.L, 160); assert.strictEqual(d.M, 441); assert.strictEqual(d.taps, 32);
    assert.ok(d.table instanceof Float32Array && d.table.length === 160 * 32);
    for (let p = 0; p < 160; p++) { let s = 0; for (let t = 0; t < 32; t++) s += d.table[p * 32 + t]; assert.ok(Math.abs(s - 1) < 1e-6, 'row ' + p + ' sums to 1'); }
    assert.deepStrictEqual(bitsOf(addon.resampleDesign(48000, 16000, 32).table), bitsOf(addon.resampleDesign(48000, 16000, 32, 0.95, 9).table), 'the defaults');
    for (const bad of [[48000, 16000, 30], [48000, 5000, 4], [16000, 44100, 64], [0, 16000, 32]]) assert.throws(function () { addon.resampleDesign(bad[0], bad[1], bad[2]); }, /aacg_resample_design failed \(-1\)/);
    console.log('resample design tests ok');
} else {
    const host = require(path.join(root, 'aac.js_amd', 'js'));
    const bytes = new Uint8Array(fs.readFileSync(path.join(root, 'tests', 'golden', 'streams', 'stereo48.aac')));
    /* two decoders of the same stereo stream, the second one frame behind; parsing: forced onto the parsing route (a decoder that wants the
     * window shape carried on an engine made without it: SharedEngine.takesResident) */
    const run = function (sampleRate, parsing, outputKind) {
        const o = { resident: true, maxStreams: 4, maxChannels: 2, lookahead: 4, outputKind: outputKind | 0 };
        if (sampleRate) o.sampleRate = sampleRate;
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
        return { out: out, rates: decs.map(function (d) { return d.format.sampleRate; }), launches: shared.launchCounts().launches };
    };
    const spec = host.loadAddon().resampleDesign(48000, 16000, 32);
    for (const leg of [{ parsing: false, kind: host.OUTPUT_F32 }, { parsing: false, kind: host.OUTPUT_I16 }, { parsing: true, kind: host.OUTPUT_F32 }]) {
        const plain = run(0, leg.parsing, leg.kind), down = run(16000, leg.parsing, leg.kind), same = run(48000, leg.parsing, leg.kind);
        assert.deepStrictEqual(plain.rates, [48000, 48000]);
        assert.deepStrictEqual(down.rates, [16000, 16000]);
        if (!leg.parsing) assert.ok(down.launches > 0 && down.launches === plain.launches, 'the resident route, launch for launch');
        for (let s = 0; s < 2; s++) {
            assert.ok(plain.out[s].length >= 16 && plain.out[s].length === down.out[s].length && plain.out[s].length === same.out[s].length, 'frames');
            const r = new rs.Resampler(spec, 2);
            let lengths = 0;
            plain.out[s].forEach(function (frame, f) {
                assert.strictEqual(frame.length, 2 * 1024);
                assert.ok(leg.kind === host.OUTPUT_I16 && !leg.parsing ? frame instanceof Int16Array : frame instanceof Float32Array);
                const want = r.push(frame);
                assert.ok(want.length === 2 * 341 || want.length === 2 * 342);
                assert.strictEqual(down.out[s][f].length, want.length, 'stream ' + s + ' frame ' + f + ': the chunk is the frame\'s share');
                assert.deepStrictEqual(bitsOf(down.out[s][f]), bitsOf(want), 'stream ' + s + ' frame ' + f + ': sampleRate 16000 is not resample.js over the plain output');
                assert.deepStrictEqual(bitsOf(same.out[s][f]), bitsOf(frame), 'the stream\'s own rate: nothing is resampled');
                lengths += want.length / 2;
            });
            assert.strictEqual(lengths, Math.ceil(plain.out[s].length * 1024 / 3));
            assert.ok(plain.out[s].some(function (frame) { return frame.some(function (v) { return v !== 0; }); }), 'the stream is music');
        }
        console.log('sampleRate ' + (leg.parsing ? 'parsing' : 'resident') + ' route, ' + (leg.kind === host.OUTPUT_I16 ? 'int16' : 'f32') + ': ' + plain.out[0].length + ' + ' + plain.out[1].length + ' frames equal resample.js over the plain engine\'s');
    }
    console.log('resample gpu tests ok');
}
