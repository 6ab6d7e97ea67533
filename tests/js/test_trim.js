/*
 * test_trim.js — aac.js_amd/js/trim.js against vectors the Python rule wrote (tests/test_pcm_trim_js.py: trim_kit in Python integers and
 * fractions): node tests/js/test_trim.js cpu <vectors.json> — no GPU, no addon; `design <vectors.json>`: the addon's trimDesign against the
 * same vectors (no GPU); `gpu`: SharedEngine({ resident: true, trim: true }) on a real MI355X — readChunk() against the same engine's
 * untrimmed output sliced by trim.js, chunk lengths included, resident and parsing route, f32 and int16, with and without sampleRate.
 */
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const trim = require(path.join(__dirname, '..', '..', 'aac.js_amd', 'js', 'trim.js'));

const window_ = (k) => (k === null ? undefined : k);
const mode = process.argv[2] || 'cpu';
if (mode === 'gpu') { gpu(); process.exit(0); }
if (mode === 'design') { design(); process.exit(0); }
if (mode !== 'cpu') { console.error('test_trim.js: mode cpu, design or gpu'); process.exit(2); }
const v = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));

let n = 0;
for (const c of v.counts) {
    const got = trim.counts(c.position, c.skip, window_(c.keep), c.n_in);
    assert.deepStrictEqual(got.firstOf, c.first_of, 'firstOf ' + JSON.stringify(c));
    assert.deepStrictEqual(got.keptOf, c.kept_of, 'keptOf ' + JSON.stringify(c));
    n++;
}
for (const c of v.design) {
    const got = trim.design(c.skip_in, window_(c.keep_in), c.limiter, c.taps || c.L !== 1 || c.M !== 1 ? { L: c.L, M: c.M, taps: c.taps } : undefined);
    assert.deepStrictEqual([got.skip, got.keep, got.residualNum * c.residual[1], got.residualDen % c.residual[1]], [c.skip, c.keep, c.residual[0] * got.residualDen, 0], 'design ' + JSON.stringify(c));
    n++;
}
/* a Trimmer over chunks of a stream, both element types: the chunks it delivers are the slices, with their lengths; none where nothing is kept */
for (const c of v.streams) {
    for (const T of [Float32Array, Int16Array]) {
        const t = new trim.Trimmer(c.channels, c.skip, window_(c.keep));
        let at = 0;
        const delivered = [];
        for (const len of c.chunks) {
            const pcm = new T(len * c.channels);
            for (let i = 0; i < pcm.length; i++) pcm[i] = ((at * c.channels + i) * 7 + 1) % 30000;
            const out = t.take(pcm);
            if (out) { assert.ok(out instanceof T); delivered.push([out.length / c.channels, out[0]]); }
            at += len;
        }
        assert.deepStrictEqual(delivered, c.delivered, 'stream ' + JSON.stringify(c));
        assert.strictEqual(t.position, at);
        t.reset();
        assert.deepStrictEqual([t.position, t.skip, t.keep], [0, c.skip, c.keep]);
        n++;
    }
}
for (const bad of [[2 ** 40, undefined], [0, 2 ** 40], [-1, undefined], [0.5, undefined], [0, -1]]) {
    assert.throws(() => trim.counts(0, bad[0], bad[1], [1024]), RangeError);
    assert.throws(() => trim.design(bad[0], bad[1], false), RangeError);
    assert.throws(() => new trim.Trimmer(2, bad[0], bad[1]), RangeError);
}
assert.throws(() => trim.design(0, undefined, false, { L: 1025, M: 1, taps: 4 }), RangeError);
assert.throws(() => trim.design(2 ** 40 - 1, undefined, true), RangeError);
console.log('trim cpu tests ok: ' + n + ' vectors');

function bitsOf(a) { return Array.from(a instanceof Float32Array ? new Uint32Array(a.buffer, a.byteOffset, a.length) : a); }

/* the addon's trimDesign (aacg_trim_design) against the Python vectors, and trim.js's design against it */
function design() {
    const host = require(path.join(__dirname, '..', '..', 'aac.js_amd', 'js'));
    const addon = host.loadAddon(), vec = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
    for (const c of vec.design) {
        const got = addon.trimDesign(c.skip_in, c.keep_in === null ? undefined : c.keep_in, c.limiter, c.L, c.M, c.taps);
        assert.deepStrictEqual([got.skip, got.keep], [c.skip, c.keep], 'trimDesign ' + JSON.stringify(c));
        assert.strictEqual(got.residualNum * c.residual[1], c.residual[0] * got.residualDen);
        assert.deepStrictEqual(got, trim.design(c.skip_in, window_(c.keep_in), c.limiter, { L: c.L, M: c.M, taps: c.taps }));
    }
    assert.throws(function () { addon.trimDesign(2 ** 40, undefined, false); }, /aacg_trim_design failed \(-1\)/);
    assert.throws(function () { addon.trimDesign(-1, undefined, false); }, TypeError);
    assert.throws(function () { addon.trimDesign(0.5, undefined, false); }, TypeError);
    console.log('trim design tests ok: ' + vec.design.length + ' vectors');
}

function gpu() {
    const host = require(path.join(__dirname, '..', '..', 'aac.js_amd', 'js'));
    const bytes = new Uint8Array(fs.readFileSync(path.join(__dirname, '..', 'golden', 'streams', 'stereo48.aac')));
    const list = host.adts.frames(bytes);
    /* two decoders of the same stereo stream, the second one frame behind; parsing: forced onto the parsing route (a decoder that wants
     * the window shape carried on an engine made without it: SharedEngine.takesResident); windows: per decoder [skip, length] or null */
    const run = function (o, parsing, windows) {
        const shared = new host.SharedEngine(Object.assign({ resident: true, maxStreams: 4, maxChannels: 2, lookahead: 4 }, o));
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
            assert.strictEqual(typeof dec.setTrim, o.trim ? 'function' : 'undefined', 'setTrim is there with { trim: true } only');
            if (windows && windows[k]) dec.setTrim(windows[k][0], windows[k][1]);
            return dec;
        });
        const out = decs.map(function (dec) {
            const chunks = [];
            for (let f = dec.readChunk(); f; f = dec.readChunk()) chunks.push(f.slice());
            return chunks;
        });
        return { out: out, decs: decs, launches: shared.launchCounts().launches };
    };
    const addon = host.loadAddon();
    let legs = 0;
    for (const leg of [{ parsing: false, kind: host.OUTPUT_F32 }, { parsing: false, kind: host.OUTPUT_I16 }, { parsing: true, kind: host.OUTPUT_F32 }]) {
        for (const sampleRate of [0, 16000]) {
            const o = { outputKind: leg.kind };
            if (sampleRate) o.sampleRate = sampleRate;
            const off = run(o, leg.parsing, null);                                                        // without the option
            const plain = run(Object.assign({ trim: true }, o), leg.parsing, null);                       // with it, every window at its default
            /* the first decoder: the priming alone; the second: a window that ends inside a frame, and begins so far in that whole flushes deliver nothing */
            const windows = [[2112, undefined], [9000, 5001]];
            const cut = run(Object.assign({ trim: true }, o), leg.parsing, windows);
            if (!leg.parsing) assert.ok(cut.launches > 0 && plain.launches === off.launches, 'the resident route, launch for launch');
            for (let s = 0; s < 2; s++) {
                assert.ok(off.out[s].length >= 16 && plain.out[s].length === off.out[s].length, 'default windows: the same chunks');
                off.out[s].forEach(function (frame, f) { assert.deepStrictEqual(bitsOf(plain.out[s][f]), bitsOf(frame), 'default windows change nothing'); });
                /* what the window is at the rate that leaves: the addon's design where the engine resamples */
                const spec = sampleRate ? addon.resampleDesign(48000, sampleRate, 32) : null;
                const w = spec ? addon.trimDesign(windows[s][0], windows[s][1], false, spec.L, spec.M, spec.taps) : { skip: windows[s][0], keep: windows[s][1] === undefined ? null : windows[s][1] };
                if (spec) assert.deepStrictEqual(cut.decs[s].trimResidual, { num: w.residualNum, den: w.residualDen });
                const t = new trim.Trimmer(2, w.skip, w.keep === null ? undefined : w.keep), want = [];
                let silent = 0;
                plain.out[s].forEach(function (frame) { const k = t.take(frame); if (k) want.push(k); else silent++; });
                assert.ok(silent >= 2 && want.length >= 1, 'frames inside the priming, and frames that deliver');
                assert.strictEqual(cut.out[s].length, want.length, 'stream ' + s + ': no chunk for a frame that owns no kept sample (' + cut.out[s].length + ' against ' + want.length + ')');
                let total = 0;
                want.forEach(function (chunk, f) {
                    assert.strictEqual(cut.out[s][f].length, chunk.length, 'stream ' + s + ' chunk ' + f + ': its length');
                    assert.ok(leg.kind === host.OUTPUT_I16 && !leg.parsing ? cut.out[s][f] instanceof Int16Array : cut.out[s][f] instanceof Float32Array);
                    assert.deepStrictEqual(bitsOf(cut.out[s][f]), bitsOf(chunk), 'stream ' + s + ' chunk ' + f + ': readChunk() is not the untrimmed output sliced by trim.js');
                    total += chunk.length / 2;
                });
                const received = plain.out[s].reduce(function (a, f) { return a + f.length / 2; }, 0);
                assert.strictEqual(total, w.keep === null ? received - w.skip : w.keep, 'the kept samples in all');
                assert.ok(want.some(function (c) { return c.some(function (v) { return v !== 0; }); }), 'the stream is music');
            }
            assert.ok(cut.out[1].length < cut.out[0].length);
            console.log('trim ' + (leg.parsing ? 'parsing' : 'resident') + ' route, ' + (leg.kind === host.OUTPUT_I16 ? 'int16' : 'f32') + ', ' + (sampleRate || 48000) + ' Hz: ' +
                        cut.out[0].length + ' + ' + cut.out[1].length + ' chunks equal trim.js over the untrimmed engine\'s');
            legs++;
        }
    }
    assert.strictEqual(legs, 6);
    assert.throws(function () { new host.SharedEngine({ resident: true }).setTrim({}, 0); }, /needs \{ trim: true \}/);
    console.log('trim gpu tests ok');
}
