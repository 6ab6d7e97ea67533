#!/usr/bin/env node
/*
 * tests/js/test_ragged_shared.js — SharedEngine({ resident: true, ragged: true }): each stream's own frame count per flush.
 *   node tests/js/test_ragged_shared.js cpu   a stub addon (opts.addon) records what a flush submits: counts, packed frame tables,
 *                                             per-stream PCM views; without `ragged` the flush still cuts every stream to the fewest
 *   node tests/js/test_ragged_shared.js gpu   256 jittered streams on one resident ragged SharedEngine against decoders of their own
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const streams = path.join(root, 'tests', 'golden', 'streams');
const jitter = require(path.join(__dirname, 'jitter_feed.js'));
const mode = process.argv[2] || 'cpu';

/* an addon that decodes nothing: frame i of a batch's packed order comes back as 1024 x C samples of value 1000 x batch + i */
function stubAddon() {
    const a = { calls: [], pending: [] };
    const run = function (pipeline, bytes, frames, slots, fps, results, C, ring, ringElems) {
        const counts = typeof fps === 'number' ? Array.from(slots, function () { return fps; }) : Array.from(fps);
        const N = counts.reduce(function (x, y) { return x + y; }, 0);
        assert.strictEqual(frames.length, 2 * N, 'a frame table of two words per packed frame');
        assert.strictEqual(results.length, 8 * N, 'one 8-byte result per packed frame');
        const k = a.calls.length, pcm = new Float32Array(N * 1024 * C);
        for (let i = 0; i < N; i++) pcm.fill(1000 * k + i, i * 1024 * C, (i + 1) * 1024 * C);
        a.calls.push({ bytes: bytes.slice(), frames: frames.slice(), slots: slots.slice(), fps: typeof fps === 'number' ? fps : fps.slice(), C: C, ring: ring, ringElems: ringElems });
        return { pcm: pcm, refused: 0 };
    };
    a.pipelineCreate = function (o) { a.created = o; return { stub: true }; };
    a.pipelineDecode = run;
    a.pipelineSubmit = function () { a.pending.push(run.apply(null, arguments)); };
    a.pipelineCollect = function () { return a.pending.shift(); };
    a.pipelineResetStream = function () {};
    a.parseStatusString = function (s) { return 'status ' + s; };
    return a;
}

const bytes = new Uint8Array(fs.readFileSync(path.join(streams, 'stereo48.aac'))), list = host.adts.frames(bytes);
/* a decoder fed the stream's first k ADTS frames (bytes [0, end of frame k)) */
function open(shared, k) {
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
function frameBytes(i) { return bytes.subarray(list[i].offset, list[i].offset + list[i].length); }

if (mode === 'cpu') {
    const have = [1, 5, 16];
    for (const overlap of [false, true]) {
        for (const ring of [0, 3]) {
            /* ragged: counts [1, 5, 16], frames packed stream after stream, each stream's frames its own PCM */
            const addon = stubAddon();
            const shared = new host.SharedEngine({ resident: true, ragged: true, addon: addon, maxStreams: 8, lookahead: 16, overlap: overlap, pcmRing: ring });
            const decs = have.map(function (k) { return open(shared, k); });
            const first = decs[0].readChunk();
            assert.strictEqual(addon.created.maxFrames, 16);
            assert.strictEqual(addon.calls.length, 1, 'one flush, one batch');
            const c = addon.calls[0];
            assert.ok(c.fps instanceof Uint32Array, 'ragged: per-stream counts');
            assert.deepStrictEqual(Array.from(c.fps), have);
            assert.deepStrictEqual(Array.from(c.slots), [0, 1, 2]);
            assert.strictEqual(c.ring, ring);
            if (ring) assert.strictEqual(c.ringElems, 8 * 16 * 1024 * 2, 'a ring buffer holds maxStreams x lookahead frames');
            /* the frame table: stream s's frames at [first_s, first_s + counts[s]), pointing at its own bytes in order */
            let i = 0;
            for (let s = 0; s < have.length; s++)
                for (let f = 0; f < have[s]; f++, i++) {
                    const off = c.frames[2 * i], len = c.frames[2 * i + 1];
                    assert.ok(Buffer.from(c.bytes.subarray(off, off + len)).equals(Buffer.from(frameBytes(f))), 'stream ' + s + ' frame ' + f);
                }
            /* the PCM: stream s's frame f is packed frame first_s + f */
            const got = [[first]];
            for (let s = 0; s < decs.length; s++) {
                if (s) got.push([]);
                for (let x; (x = decs[s].queue.length ? decs[s].readChunk() : null);) got[s].push(x);
            }
            const firsts = [0, 1, 6];
            for (let s = 0; s < have.length; s++) {
                assert.strictEqual(got[s].length, have[s], 'stream ' + s + ': every buffered frame delivered');
                got[s].forEach(function (x, f) {
                    assert.strictEqual(x.length, 1024 * 2);
                    assert.ok(x.every(function (v) { return v === firsts[s] + f; }), 'stream ' + s + ' frame ' + f + ' is packed frame ' + (firsts[s] + f));
                });
            }
            assert.strictEqual(shared.stats.frames, 22);
            assert.strictEqual(decs[0].readChunk(), null, 'nothing left');
        }
        /* ragged unset: the flush cuts every stream to the fewest frames any of them has (F = 1) */
        const addon = stubAddon();
        const shared = new host.SharedEngine({ resident: true, addon: addon, maxStreams: 8, lookahead: 16, overlap: overlap });
        const decs = have.map(function (k) { return open(shared, k); });
        decs[0].readChunk();
        const c = addon.calls[0];
        assert.strictEqual(c.fps, 1, 'a number, as before');
        assert.strictEqual(c.frames.length, 2 * 3);
        for (let s = 0; s < 3; s++) assert.ok(decs[s].queue.length + (s ? 0 : 1) >= 1);
        assert.strictEqual(decs[1].readChunk()[0], 1);
        assert.strictEqual(decs[2].readChunk()[0], 2);
    }
    /* a paused reader (a full queue) sits a flush out; the others still bring what they have */
    {
        const addon = stubAddon();
        const shared = new host.SharedEngine({ resident: true, ragged: true, addon: addon, maxStreams: 8, lookahead: 4, overlap: false });
        const decs = [3, 2, 4].map(function (k) { return open(shared, k); });
        decs[0].readChunk();
        assert.deepStrictEqual(Array.from(addon.calls[0].fps), [3, 2, 4]);
        decs[1].readChunk(); decs[1].readChunk();
        [5, 6].forEach(function (k) { decs[1].feed(frameBytes(k)); });
        decs[1].readChunk();
        assert.deepStrictEqual(Array.from(addon.calls[1].slots), [1], 'the streams with full queues sit the flush out');
        assert.deepStrictEqual(Array.from(addon.calls[1].fps), [2]);
    }
    /* jittered arrival (tests/js/jitter_feed.js) with the stub: every fed frame is read, in both modes; ragged flushes are fewer */
    {
        const src = [{ bytes: bytes, list: list }], seen = {};
        for (const ragged of [false, true]) {
            const addon = stubAddon();
            const sh = new host.SharedEngine({ resident: true, ragged: ragged, addon: addon, maxStreams: 32, lookahead: 16 });
            const r = jitter.run({ host: host, shared: sh, sources: src, streams: 24, rounds: 12, seed: 3 });
            assert.strictEqual(r.frames, sh.stats.frames);
            seen[ragged] = { frames: r.frames, flushes: sh.stats.batches, instances: r.instances };
            if (ragged) addon.calls.forEach(function (c) { assert.ok(c.fps instanceof Uint32Array && c.fps.every(function (n) { return n >= 1 && n <= 16; })); });
        }
        assert.strictEqual(seen[true].frames, seen[false].frames, 'the same frames read with and without ragged');
        assert.strictEqual(seen[true].instances, seen[false].instances);
        assert.ok(seen[true].flushes < seen[false].flushes, JSON.stringify(seen));
    }
    console.log('ragged shared cpu tests ok');
    process.exit(0);
}

if (mode === 'gpu') {
    /* 256 streams of the committed files (each repeated four times) with jittered arrival on ONE resident ragged SharedEngine:
     * every frame every stream returns has the bits a decoder of its own (no shared engine) gives for the same frame of the same
     * bytes.  The streams of one source are the same bytes, so one independent decoder per source stands for all of them. */
    const manifest = JSON.parse(fs.readFileSync(path.join(streams, 'manifest.json')));
    const sources = manifest.map(function (m) {
        const one = new Uint8Array(fs.readFileSync(path.join(streams, m.name + '.aac'))), b = new Uint8Array(one.length * 4);
        for (let i = 0; i < 4; i++) b.set(one, i * one.length);
        return { name: m.name, bytes: b, list: host.adts.frames(b) };
    });
    const alone = sources.map(function (src) {
        const dec = new host.GpuAACDecoder({ frontend: new host.FrontEnd(), lookahead: 16 });
        dec.init(); dec.setCookie(host.adts.cookie(src.list[0].header)); dec.feed(src.bytes);
        const out = [];
        for (let x; (x = dec.readChunk());) out.push(Buffer.from(x.buffer, x.byteOffset, x.byteLength));
        assert.strictEqual(out.length, src.list.length, src.name + ': every frame alone');
        return out;
    });
    /* (with pcmRing a frame is valid until K more flushes of its pipeline, read or not: a reader paused for rounds while its
     * peers' reads flush falls behind that by design, so the ring variant runs without pauses) */
    const variants = [{ overlap: true, pcmRing: 0 }, { overlap: false, pcmRing: 0 }, { overlap: true, pcmRing: 8, pauses: false }];
    const sums = [];
    for (const v of variants) {
        const sh = new host.SharedEngine({ resident: true, ragged: true, maxStreams: 256, maxChannels: 8, lookahead: 16, overlap: v.overlap, pcmRing: v.pcmRing });
        let checked = 0;
        const r = jitter.run({ host: host, shared: sh, sources: sources, streams: 256, rounds: 24, seed: 11, pauses: v.pauses !== false, onFrame: function (i, src, f, pcm) {
            const got = Buffer.from(pcm.buffer, pcm.byteOffset, pcm.byteLength);
            if (!got.equals(alone[src][f])) throw new Error(JSON.stringify(v) + ': stream ' + i + ' (' + sources[src].name + ') frame ' + f + ' differs from its decoder alone');
            checked++;
        } });
        assert.strictEqual(checked, r.frames);
        /* (a batch is one group's: five sources, one pipeline per sample rate and channel count, about 51 streams each) */
        assert.ok(sh.stats.frames / sh.stats.batches > 16, 'frames per batch ' + sh.stats.frames / sh.stats.batches);
        sums.push(r.sums);
        console.log('jitter ' + JSON.stringify(v) + ': ' + r.frames + ' frames of ' + r.instances + ' decoders in ' + sh.stats.batches + ' flushes, ' + sh.planBuilds() + ' plans built');
    }
    assert.deepStrictEqual(sums[1], sums[0]); assert.deepStrictEqual(sums[2], sums[0]);
    console.log('ragged shared gpu tests ok');
    process.exit(0);
}

throw new Error('unknown mode ' + mode);
