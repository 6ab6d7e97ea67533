#!/usr/bin/env node
/*
 * tests/js/test_conceal.js — SharedEngine({ resident: true, ragged: true, devicePlans: true, conceal: true | { fadeSteps, holdFrames } }):
 * a frame the device refused and concealed is delivered, not thrown.
 *   node tests/js/test_conceal.js [cpu]              a stub addon (no GPU): the option reaches the pipeline's config, it throws at
 *                                                    construction without devicePlans, a result that carries the concealed flag
 *                                                    delivers its PCM and is counted, a refused frame without it still throws
 *   node tests/js/test_conceal.js gpu <dir> <out>    three stereo streams of tests/js/shape_cases.js (in <dir>) on a real GPU, one
 *                                                    frame cut to 9 bytes: readChunk() returns PCM for it, stats.concealedFrames is
 *                                                    1, and without the option the same feed throws the reference's message; the
 *                                                    feeds and the PCM go to <out> for tests/test_conceal_js.py to compare
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const streams = path.join(root, 'tests', 'golden', 'streams');

function open(shared, bytes, lookahead) {
    const dec = new host.GpuAACDecoder({ frontend: null, lookahead: lookahead, shared: shared });
    dec.init();
    const demux = new host.adts.AdtsDemuxer(function (event, payload) {
        if (event === 'format') Object.assign(dec.format, payload);
        else if (event === 'cookie') dec.setCookie(payload);
        else if (event === 'data') dec.feed(payload);
    });
    demux.push(bytes);
    return dec;
}

/* the stream with frame k cut to its first 9 bytes — the ADTS header and two bytes of the raw_data_block, the header's frame_length
 * rewritten to say so: a frame that ends inside its first element */
function cut(bytes, k) {
    const list = host.adts.frames(bytes), f = list[k];
    const out = new Uint8Array(bytes.length - f.length + 9);
    out.set(bytes.subarray(0, f.offset + 9), 0);
    out.set(bytes.subarray(f.offset + f.length), f.offset + 9);
    out[f.offset + 3] = (out[f.offset + 3] & 0xfc) | ((9 >> 11) & 3);
    out[f.offset + 4] = (9 >> 3) & 0xff;
    out[f.offset + 5] = (out[f.offset + 5] & 0x1f) | ((9 & 7) << 5);
    return out;
}

if ((process.argv[2] || 'cpu') === 'gpu') {
    const dir = process.argv[3], outDir = process.argv[4];
    const feeds = ['stereo48', 'split48', 'stereo48'].map(function (n) { return new Uint8Array(fs.readFileSync(path.join(dir, n + '.aac'))); });
    feeds[1] = cut(feeds[1], 5);
    feeds.forEach(function (b, i) { fs.writeFileSync(path.join(outDir, 'feed_' + i + '.aac'), b); });
    const sh = new host.SharedEngine({ resident: true, ragged: true, devicePlans: true, conceal: true, maxStreams: 4, lookahead: 4 });
    const decs = feeds.map(function (b) { return open(sh, b, 4); });
    const got = decs.map(function () { return []; });
    for (let f = 0; f < 12; f++)
        decs.forEach(function (d, i) {
            const x = d.readChunk();
            assert.ok(x instanceof Float32Array && x.length === 2048, 'stream ' + i + ' frame ' + f + ': PCM, concealed or not');
            got[i].push(new Float32Array(x));
        });
    decs.forEach(function (d, i) { assert.ok(!d.readChunk(), 'twelve frames a stream'); });
    assert.strictEqual(sh.stats.concealedFrames, 1);
    got.forEach(function (frames, i) {
        const all = new Float32Array(12 * 2048);
        frames.forEach(function (x, f) { all.set(x, f * 2048); });
        fs.writeFileSync(path.join(outDir, 'js_' + i + '.f32'), Buffer.from(all.buffer));
    });
    /* without the option the same feed throws the reference's message where the frame is reached, as ever */
    const plain = new host.SharedEngine({ resident: true, ragged: true, devicePlans: true, maxStreams: 4, lookahead: 4 });
    const pd = feeds.map(function (b) { return open(plain, b, 4); });
    let thrown = 0;
    for (let f = 0; f < 12; f++)
        pd.forEach(function (d, i) {
            if (i === 1 && f === 5) {
                assert.throws(function () { d.readChunk(); }, function (e) { return e instanceof Error && e.message === host.loadAddon().parseStatusString(1); });
                thrown++;
            } else assert.ok(d.readChunk() instanceof Float32Array, 'stream ' + i + ' frame ' + f);
        });
    assert.strictEqual(thrown, 1);
    assert.strictEqual(plain.stats.concealedFrames, 0);
    console.log('conceal gpu tests ok');
    process.exit(0);
}

/* an addon that decodes nothing, records what it is asked and answers with the results it is told to (tests/js/test_device_plans.js) */
function stubAddon(marks) {
    const a = { created: [], pending: [] };
    const run = function (pipeline, bytes, frames, slots, fps, results, C) {
        const counts = typeof fps === 'number' ? Array.from(slots, function () { return fps; }) : Array.from(fps);
        const N = counts.reduce(function (x, y) { return x + y; }, 0);
        let refused = 0;
        for (const m of marks) if (m.frame < N) { results[8 * m.frame] = m.status; results[8 * m.frame + 3] = m.flags; refused++; }
        const pcm = new Float32Array(N * 1024 * C);
        for (let i = 0; i < N; i++) pcm[i * 1024 * C] = i + 1;
        return { pcm: pcm, refused: refused };
    };
    a.pipelineCreate = function (o) { const p = { stub: true, opts: o }; a.created.push(p); return p; };
    a.pipelineDecode = run;
    a.pipelineSubmit = function () { a.pending.push(run.apply(null, arguments)); };
    a.pipelineCollect = function () { return a.pending.shift(); };
    a.pipelineResetStream = function () {};
    a.parseStatusString = function (s) { return 'status ' + s; };
    return a;
}
const stereo = new Uint8Array(fs.readFileSync(path.join(streams, 'stereo48.aac')));
/* the option needs the resident route and device plans */
for (const o of [{ resident: true, ragged: true }, { resident: true, devicePlans: false }, { devicePlans: true }])
    assert.throws(function () { return new host.SharedEngine(Object.assign({ conceal: true, addon: stubAddon([]) }, o)); }, /conceal needs/);
/* ... and reaches the pipeline's config: the defaults, or the caller's figures; off, no word of it */
for (const [opt, want] of [[true, { fadeSteps: 2, holdFrames: 6 }], [{ fadeSteps: 0, holdFrames: 3 }, { fadeSteps: 0, holdFrames: 3 }], [{ holdFrames: 9 }, { fadeSteps: 2, holdFrames: 9 }],
                           [undefined, undefined]]) {
    const addon = stubAddon([]);
    const shared = new host.SharedEngine({ resident: true, ragged: true, devicePlans: true, conceal: opt, addon: addon, maxStreams: 4, lookahead: 4, overlap: false });
    open(shared, stereo, 4).readChunk();
    assert.strictEqual(addon.created.length, 1);
    assert.deepStrictEqual(addon.created[0].opts.conceal, want);
    assert.strictEqual(addon.created[0].opts.planMode, 1);
    assert.strictEqual(shared.stats.concealedFrames, 0);
}
/* a refused frame whose result carries the flag is delivered and counted; one without it throws the status's message, as ever */
{
    const addon = stubAddon([{ frame: 1, status: 1, flags: 0x8 | 0x2 }, { frame: 2, status: 4, flags: 0x2 }]);
    const shared = new host.SharedEngine({ resident: true, ragged: true, devicePlans: true, conceal: true, addon: addon, maxStreams: 4, lookahead: 4, overlap: false });
    const dec = open(shared, stereo, 4);
    assert.strictEqual(dec.readChunk()[0], 1);
    const x = dec.readChunk();
    assert.ok(x instanceof Float32Array && x.length === 2048 && x[0] === 2, 'the concealed frame\'s own PCM');
    assert.throws(function () { dec.readChunk(); }, /^Error: status 4$/);
    assert.strictEqual(dec.readChunk()[0], 4);
    assert.strictEqual(shared.stats.concealedFrames, 1);
}
console.log('conceal cpu tests ok');
