#!/usr/bin/env node
/*
 * tests/js/test_resident_shape.js — SharedEngine({ resident: true, carryWindowShape: true }): decoders that carry each channel's
 * window shape take the resident route, their pipelines are created with bit 2 of the `stages` word.
 *   node tests/js/test_resident_shape.js [cpu]        a stub addon (no GPU): who takes which route, what the pipeline is asked for
 *   node tests/js/test_resident_shape.js gpu <dir>    the streams of tests/js/shape_cases.js (in <dir>) on a real GPU: readChunk()
 *                                                     returns the same samples, bit for bit, as the parsing route with
 *                                                     carryWindowShape — as ADTS streams and as 'mp4a' packets (residentPackets)
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const streams = path.join(root, 'tests', 'golden', 'streams');

function open(shared, file, modes, frontend) {
    const bytes = new Uint8Array(fs.readFileSync(file));
    const dec = new host.GpuAACDecoder(Object.assign({ frontend: frontend ? new host.FrontEnd() : null, lookahead: 4, shared: shared }, modes));
    dec.init();
    const demux = new host.adts.AdtsDemuxer(function (event, payload) {
        if (event === 'format') Object.assign(dec.format, payload);
        else if (event === 'cookie') dec.setCookie(payload);
        else if (event === 'data') dec.feed(payload);
    });
    demux.push(bytes);
    return dec;
}
function concat(parts) {
    const out = new Uint8Array(parts.reduce(function (a, b) { return a + b.length; }, 0));
    let at = 0;
    for (const p of parts) { out.set(p, at); at += p.length; }
    return out;
}
/* the same stream as MP4 samples: the ADTS headers cut off, the first block alone (a single-sample packet), then 3 blocks a packet */
function openPackets(shared, file, modes) {
    const bytes = new Uint8Array(fs.readFileSync(file)), list = host.adts.frames(bytes);
    const blocks = list.map(function (f) { return bytes.subarray(f.offset + f.header.headerBytes, f.offset + f.length); });
    const dec = new host.GpuAACDecoder(Object.assign({ frontend: new host.FrontEnd(), lookahead: 4, shared: shared, format: { formatID: 'mp4a' } }, modes));
    dec.init(); dec.setCookie(host.adts.cookie(list[0].header));
    dec.feedPacket(blocks[0], false);
    for (let i = 1; i < blocks.length; i += 3) dec.feedPacket(concat(blocks.slice(i, i + 3)), true);
    return dec;
}
function sameBits(x, y, what) {
    assert.ok(x && y && x.length === y.length, what);
    const u = new Uint32Array(x.buffer, x.byteOffset, x.length), v = new Uint32Array(y.buffer, y.byteOffset, y.length);
    for (let k = 0; k < u.length; k++) if (u[k] !== v[k]) assert.fail(what + ' sample ' + k + ': resident ' + x[k] + ', parsing route ' + y[k]);
}

if ((process.argv[2] || 'cpu') === 'gpu') {
    const dir = process.argv[3], manifest = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json')));
    const carry = { carryWindowShape: true };
    let frames = 0, differ = 0;
    for (const packets of [false, true]) {
        /* the eight streams, one decoder each: several pipelines (mono / stereo / 5.1 at 48 and 16 kHz) on one engine */
        const res = new host.SharedEngine({ resident: true, residentPackets: packets, carryWindowShape: true, maxStreams: 8, maxChannels: 8, lookahead: 4 });
        const par = new host.SharedEngine({ maxStreams: 8, maxChannels: 8 });
        const off = new host.SharedEngine({ resident: true, residentPackets: packets, maxStreams: 8, maxChannels: 8, lookahead: 4 });
        const a = [], b = [], z = [];
        for (const c of manifest) {
            const file = path.join(dir, c.name + '.aac');
            a.push(packets ? openPackets(res, file, carry) : open(res, file, carry, false));
            b.push(packets ? openPackets(par, file, carry) : open(par, file, carry, true));
            z.push(packets ? openPackets(off, file, {}) : open(off, file, {}, false));
        }
        assert.strictEqual(a.length, 8);
        for (const d of a) assert.strictEqual(d.resident, true, 'a decoder that carries its window shape takes the resident route of an engine that does');
        for (const d of b) assert.ok(!d.resident);
        for (const d of z) assert.strictEqual(d.resident, true);
        for (let f = 0; f < 12; f++)
            for (let i = 0; i < a.length; i++) {
                const x = a[i].readChunk(), y = b[i].readChunk(), w = z[i].readChunk();
                sameBits(x, y, (packets ? 'mp4a ' : 'adts ') + manifest[i].name + ' frame ' + f);
                /* ... and the carried shape is not a no-op: without it the resident route gives other samples somewhere */
                const u = new Uint32Array(x.buffer, x.byteOffset, x.length), v = new Uint32Array(w.buffer, w.byteOffset, w.length);
                let same = u.length === v.length;
                for (let k = 0; same && k < u.length; k++) same = u[k] === v[k];
                if (!same) differ++;
                frames++;
            }
        for (let i = 0; i < a.length; i++) assert.ok(!a[i].readChunk() && !b[i].readChunk(), 'twelve frames a stream');
        console.log((packets ? "'mp4a' packets: " : 'ADTS: ') + JSON.stringify(res.launchCounts()));
    }
    assert.ok(frames === 2 * 8 * 12 && differ >= 2 * 8, 'frames ' + frames + ', of them other samples than without the carried shape: ' + differ);
    console.log('resident shape gpu tests ok: ' + frames + ' frames bit for bit, ' + differ + ' of them not the samples of an engine without carryWindowShape');
    process.exit(0);
}

/* an addon that decodes nothing and records what it is asked (tests/js/test_resident_stages.js) */
function stubAddon() {
    const a = { created: [], pending: [] };
    const run = function (pipeline, bytes, frames, slots, fps, results, C) {
        const counts = typeof fps === 'number' ? Array.from(slots, function () { return fps; }) : Array.from(fps);
        return { pcm: new Float32Array(counts.reduce(function (x, y) { return x + y; }, 0) * 1024 * C), refused: 0 };
    };
    a.pipelineCreate = function (o) { const p = { stub: true, opts: o }; a.created.push(p); return p; };
    a.pipelineDecode = run;
    a.pipelineSubmit = function () { a.pending.push(run.apply(null, arguments)); };
    a.pipelineCollect = function () { return a.pending.shift(); };
    a.pipelineResetStream = function () {};
    a.parseStatusString = function (s) { return 'status ' + s; };
    return a;
}
const stereo = path.join(streams, 'stereo48.aac');
const engineStub = function () { return { decodeBatch: function () { throw new Error('not in this test'); }, resetStream: function () {}, close: function () {} }; };
for (const [tns, pns, stages] of [[0, 0, 4], [1, 1, 7], [1, 0, 5], [0, 1, 6]]) {
    const addon = stubAddon();
    const shared = new host.SharedEngine({ resident: true, addon: addon, engine: engineStub, maxStreams: 8, lookahead: 4, overlap: false, tnsMode: tns, pnsMode: pns,
                                           carryWindowShape: true });
    const dec = open(shared, stereo, { tnsMode: tns, pnsMode: pns, carryWindowShape: true }, false);
    assert.strictEqual(dec.resident, true, 'carryWindowShape on both sides: the resident route');
    assert.strictEqual(addon.created.length, 1);
    assert.strictEqual(addon.created[0].opts.stages | 0, stages, 'the pipeline\'s stages word');
    dec.readChunk();
    /* a mismatch goes to the parsing route: a decoder that does not carry on an engine that does */
    const other = open(shared, stereo, { tnsMode: tns, pnsMode: pns }, true);
    assert.ok(!other.resident, 'no carryWindowShape on the decoder: the parsing route');
    assert.strictEqual(addon.created.length, 1, 'no second pipeline');
}
/* ... and the other way round, as before: an engine without the option keeps such a decoder on the parsing route, stages word 0 */
{
    const addon = stubAddon();
    const shared = new host.SharedEngine({ resident: true, addon: addon, engine: engineStub, maxStreams: 8, lookahead: 4, overlap: false });
    assert.ok(!open(shared, stereo, { carryWindowShape: true }, true).resident);
    assert.strictEqual(addon.created.length, 0);
    assert.strictEqual(open(shared, stereo, {}, false).resident, true);
    assert.strictEqual(addon.created[0].opts.stages | 0, 0);
}
/* int16 PCM goes with the carried shape (the plain launch writes it), not with the spec stages */
{
    const addon = stubAddon();
    const shared = new host.SharedEngine({ resident: true, addon: addon, engine: engineStub, maxStreams: 8, lookahead: 4, overlap: false, carryWindowShape: true,
                                           outputKind: host.OUTPUT_I16 });
    assert.strictEqual(open(shared, stereo, { carryWindowShape: true }, false).resident, true);
    assert.strictEqual(addon.created[0].opts.stages | 0, 4);
    assert.strictEqual(addon.created[0].opts.outputKind | 0, host.OUTPUT_I16);
    const spec = new host.SharedEngine({ resident: true, addon: stubAddon(), engine: engineStub, maxStreams: 8, lookahead: 4, tnsMode: 1, carryWindowShape: true,
                                         outputKind: host.OUTPUT_I16 });
    assert.ok(!open(spec, stereo, { tnsMode: 1, carryWindowShape: true }, true).resident);
}
/* 'mp4a' packets follow: residentPackets decides, the carried shape must match as for ADTS */
{
    const mk = function (o) { return Object.assign({ config: { profile: 2, chanConfig: 2, sampleIndex: 3 }, format: { formatID: 'mp4a' } }, o || {}); };
    const on = new host.SharedEngine({ resident: true, residentPackets: true, carryWindowShape: true });
    assert.ok(on.takesResident(mk({ carryWindowShape: true })) && !on.takesResident(mk()));
    assert.ok(!new host.SharedEngine({ resident: true, carryWindowShape: true }).takesResident(mk({ carryWindowShape: true })));
}
console.log('resident shape cpu tests ok');
