#!/usr/bin/env node
/*
 * tests/js/test_device_plans.js — SharedEngine({ resident: true, ragged: true, devicePlans: true }) with a stub addon (no GPU): the
 * option reaches the pipeline's config as planMode 1, it is off by default, nothing else about a flush differs (the plan mode is
 * the pipeline's business), and the counters are summed over the pipelines.
 *   node tests/js/test_device_plans.js [cpu]   the stub addon
 *   node tests/js/test_device_plans.js gpu     jittered streams with and without device plans on a real GPU: the same checksums
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const streams = path.join(root, 'tests', 'golden', 'streams');

/* an addon that decodes nothing and records what it is asked (tests/js/test_ragged_shared.js) */
function stubAddon() {
    const a = { calls: [], pending: [], created: [] };
    const run = function (pipeline, bytes, frames, slots, fps, results, C) {
        const counts = typeof fps === 'number' ? Array.from(slots, function () { return fps; }) : Array.from(fps);
        const N = counts.reduce(function (x, y) { return x + y; }, 0);
        a.calls.push({ pipeline: pipeline, slots: slots.slice(), fps: typeof fps === 'number' ? fps : fps.slice(), frames: frames.slice() });
        pipeline.batches++;
        return { pcm: new Float32Array(N * 1024 * C), refused: 0 };
    };
    a.pipelineCreate = function (o) { const p = { stub: true, opts: o, batches: 0 }; a.created.push(p); return p; };
    a.pipelineDecode = run;
    a.pipelineSubmit = function () { a.pending.push(run.apply(null, arguments)); };
    a.pipelineCollect = function () { return a.pending.shift(); };
    a.pipelineResetStream = function () {};
    a.pipelinePlanBuilds = function (p) { return p.opts.planMode ? 0 : p.batches; };
    a.pipelineLaunchCounts = function (p) { return { shaped: p.opts.planMode ? p.batches : 0, chained: 0, launches: p.batches }; };
    a.parseStatusString = function (s) { return 'status ' + s; };
    return a;
}

function open(shared, name, k) {
    const bytes = new Uint8Array(fs.readFileSync(path.join(streams, name + '.aac'))), list = host.adts.frames(bytes);
    const dec = new host.GpuAACDecoder({ frontend: new host.FrontEnd(), lookahead: 16, shared: shared });
    dec.init();
    const demux = new host.adts.AdtsDemuxer(function (event, payload) {
        if (event === 'format') Object.assign(dec.format, payload);
        else if (event === 'cookie') dec.setCookie(payload);
        else if (event === 'data') dec.feed(payload);
    });
    demux.push(bytes.subarray(0, list[k - 1].offset + list[k - 1].length));
    return dec;
}

if ((process.argv[2] || 'cpu') === 'gpu') {
    /* 128 jittered streams of the committed files on a resident ragged SharedEngine with and without device plans: the same
     * checksums stream by stream, no plan built with device plans, every batch shaped on the device */
    const jitter = require(path.join(__dirname, 'jitter_feed.js'));
    const manifest = JSON.parse(fs.readFileSync(path.join(streams, 'manifest.json')));
    const sources = manifest.map(function (m) {
        const one = new Uint8Array(fs.readFileSync(path.join(streams, m.name + '.aac'))), b = new Uint8Array(one.length * 4);
        for (let i = 0; i < 4; i++) b.set(one, i * one.length);
        return { name: m.name, bytes: b, list: host.adts.frames(b) };
    });
    const got = {};
    for (const devicePlans of [false, true]) {
        const sh = new host.SharedEngine({ resident: true, ragged: true, devicePlans: devicePlans, maxStreams: 128, maxChannels: 8, lookahead: 16 });
        const r = jitter.run({ host: host, shared: sh, sources: sources, streams: 128, rounds: 24, seed: 11 });
        const c = sh.launchCounts();
        got[devicePlans] = { sums: r.sums, frames: r.frames, builds: sh.planBuilds(), counts: c };
        console.log('jitter devicePlans ' + devicePlans + ': ' + r.frames + ' frames in ' + sh.stats.batches + ' flushes, ' + sh.planBuilds() + ' plans built, ' + JSON.stringify(c));
        assert.ok(c.launches > 0 && c.launches <= sh.stats.batches);
        assert.strictEqual(c.shaped, devicePlans ? c.launches : 0);
    }
    assert.strictEqual(got[true].builds, 0, 'device plans: no plan is built');
    assert.ok(got[false].builds > 0);
    assert.strictEqual(got[true].frames, got[false].frames);
    assert.deepStrictEqual(got[true].sums, got[false].sums, 'the same PCM checksums, stream by stream');
    console.log('device plans gpu tests ok');
    process.exit(0);
}

const seen = {};
for (const devicePlans of [undefined, false, true]) {
    const addon = stubAddon();
    const o = { resident: true, ragged: true, addon: addon, maxStreams: 8, lookahead: 16, overlap: false };
    if (devicePlans !== undefined) o.devicePlans = devicePlans;
    const shared = new host.SharedEngine(o);
    assert.strictEqual(shared.devicePlans, !!devicePlans);
    const decs = [open(shared, 'stereo48', 3), open(shared, 'stereo48', 9), open(shared, 'mono22', 2)];      // two pipelines: stereo 48 kHz, mono 22 kHz
    decs[0].readChunk(); decs[2].readChunk();
    assert.strictEqual(addon.created.length, 2, 'one pipeline per sample rate and channel count');
    for (const p of addon.created) {
        assert.strictEqual(p.opts.planMode, devicePlans ? 1 : 0, 'planMode in the config of every pipeline');
        assert.strictEqual(p.opts.maxFrames, 16);
    }
    assert.deepStrictEqual(Array.from(addon.calls[0].fps), [3, 9]);
    assert.deepStrictEqual(Array.from(addon.calls[1].fps), [2]);
    assert.strictEqual(shared.planBuilds(), devicePlans ? 0 : 2);
    assert.deepStrictEqual(shared.launchCounts(), { shaped: devicePlans ? 2 : 0, chained: 0, launches: 2 });
    seen[String(devicePlans)] = addon.calls.map(function (c) { return { slots: Array.from(c.slots), fps: Array.from(c.fps), frames: Array.from(c.frames) }; });
}
assert.deepStrictEqual(seen['true'], seen['undefined'], 'a flush submits the same batches in either plan mode');
assert.deepStrictEqual(seen['false'], seen['undefined']);
/* an addon from before the counters: nothing to sum, no error */
{
    const addon = stubAddon();
    delete addon.pipelineLaunchCounts; delete addon.pipelinePlanBuilds;
    const shared = new host.SharedEngine({ resident: true, ragged: true, devicePlans: true, addon: addon, maxStreams: 8, lookahead: 16, overlap: false });
    open(shared, 'stereo48', 2).readChunk();
    assert.deepStrictEqual(shared.launchCounts(), { shaped: 0, chained: 0, launches: 0 });
    assert.strictEqual(shared.planBuilds(), 0);
}
console.log('device plans cpu tests ok');
