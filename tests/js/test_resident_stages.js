#!/usr/bin/env node
/*
 * tests/js/test_resident_stages.js — SharedEngine({ resident: true, tnsMode, pnsMode }): decoders in the engine's spec modes take
 * the resident route, their pipelines are created with the matching `stages` word.
 *   node tests/js/test_resident_stages.js [cpu]        a stub addon (no GPU): who takes which route, what the pipeline is asked for
 *   node tests/js/test_resident_stages.js gpu <dir>    the streams of tests/js/stage_cases.js (in <dir>) on a real GPU: readChunk()
 *                                                      returns the same samples, bit for bit, as the parsing route on the same options
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

if ((process.argv[2] || 'cpu') === 'gpu') {
    const dir = process.argv[3], manifest = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json')));
    const modes = { tnsMode: host.TNS_SPEC, pnsMode: host.PNS_SPEC };
    let frames = 0, samples = 0;
    for (const devicePlans of [false, true]) {
        /* every stream twice on each engine: cross-stream batches of several pipelines (mono / stereo / 5.1 at 48 and 16 kHz) */
        const cases = manifest.filter(function (c) { return !c.oddFrame; });
        const res = new host.SharedEngine(Object.assign({ resident: true, devicePlans: devicePlans, maxStreams: 8, maxChannels: 8, lookahead: 4, applyPulses: true }, modes));
        const par = new host.SharedEngine(Object.assign({ maxStreams: 8, maxChannels: 8, applyPulses: true }, modes));
        const a = [], b = [];
        for (const c of cases) for (let k = 0; k < 2; k++) {
            a.push(open(res, path.join(dir, c.name + '.aac'), modes, false));
            b.push(open(par, path.join(dir, c.name + '.aac'), Object.assign({ applyPulses: true }, modes), true));
        }
        for (const d of a) assert.strictEqual(d.resident, true, 'a decoder in the engine\'s spec modes takes the resident route');
        for (const d of b) assert.ok(!d.resident);
        for (let f = 0; f < 12; f++)
            for (let i = 0; i < a.length; i++) {
                const x = a[i].readChunk(), y = b[i].readChunk();
                assert.ok(x && y && x.length === y.length, 'frame ' + f + ' of decoder ' + i);
                const u = new Uint32Array(x.buffer, x.byteOffset, x.length), v = new Uint32Array(y.buffer, y.byteOffset, y.length);
                for (let k = 0; k < u.length; k++) if (u[k] !== v[k]) assert.fail('decoder ' + i + ' frame ' + f + ' sample ' + k + ': resident ' + x[k] + ', parsing route ' + y[k]);
                frames++; samples += x.length;
            }
        const c = res.launchCounts();
        assert.ok(c.launches > 0 && (devicePlans ? c.shaped === c.launches : c.shaped === 0));
        console.log('devicePlans ' + devicePlans + ': ' + JSON.stringify(c));
    }
    assert.ok(frames === 2 * 16 * 12 && samples > 0);
    console.log('resident stages gpu tests ok: ' + frames + ' frames bit for bit');
    process.exit(0);
}

/* an addon that decodes nothing and records what it is asked (tests/js/test_device_plans.js) */
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
for (const [tns, pns, stages] of [[0, 0, 0], [1, 0, 1], [0, 1, 2], [1, 1, 3]]) {
    const addon = stubAddon();
    const shared = new host.SharedEngine({ resident: true, addon: addon, engine: engineStub, maxStreams: 8, lookahead: 4, overlap: false, tnsMode: tns, pnsMode: pns });
    const dec = open(shared, stereo, { tnsMode: tns, pnsMode: pns }, false);
    assert.strictEqual(dec.resident, true, 'modes equal to the engine\'s: the resident route');
    assert.strictEqual(addon.created.length, 1);
    assert.strictEqual(addon.created[0].opts.stages | 0, stages, 'the pipeline\'s stages word');
    dec.readChunk();
    /* modes that differ from the engine's are refused as on the parsing route; cceMode and carryWindowShape still exclude */
    if (tns || pns) assert.throws(function () { open(shared, stereo, {}, true); }, /differ from the shared engine/);
    else assert.throws(function () { open(shared, stereo, { tnsMode: 1 }, true); }, /differ from the shared engine/);
    const other = open(shared, stereo, { tnsMode: tns, pnsMode: pns, carryWindowShape: true }, true);
    assert.ok(!other.resident, 'carryWindowShape: the parsing route');
}
/* int16 PCM with stages: the resident route has no such launch — the parsing route */
{
    const addon = stubAddon();
    const shared = new host.SharedEngine({ resident: true, addon: addon, engine: engineStub, maxStreams: 8, lookahead: 4, tnsMode: 1, outputKind: host.OUTPUT_I16 });
    assert.ok(!open(shared, stereo, { tnsMode: 1 }, true).resident);
    assert.strictEqual(addon.created.length, 0);
}
console.log('resident stages cpu tests ok');
