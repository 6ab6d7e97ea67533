#!/usr/bin/env node
/*
 * tests/js/test_mp4a_resident.js — 'mp4a' decoders on the resident route (SharedEngine({ resident: true, residentPackets: true })).
 *   node tests/js/test_mp4a_resident.js cpu    routing only (no addon, no GPU)
 *   node tests/js/test_mp4a_resident.js gpu    the committed streams as MP4 chunks (the ADTS headers cut off, several blocks to a
 *                                               packet) through the real pipeline, next to ADTS streams on the same engine
 */
'use strict';
const fs = require('fs'), path = require('path'), assert = require('assert');
const root = path.join(__dirname, '..', '..');
const host = require(path.join(root, 'aac.js_amd', 'js'));
const streams = path.join(root, 'tests', 'golden', 'streams');
const mode = process.argv[2] || 'cpu';
const names = ['stereo48', 'surround48', 'mono22', 'extras8k', 'cce96', 'stereo48', 'surround48', 'stereo48'];

function load(name) {
    const bytes = new Uint8Array(fs.readFileSync(path.join(streams, name + '.aac'))), list = host.adts.frames(bytes);
    return { bytes: bytes, list: list, cookie: host.adts.cookie(list[0].header),
             blocks: list.map(function (f) { return bytes.subarray(f.offset + f.header.headerBytes, f.offset + f.length); }) };
}
function concat(parts) {
    const out = new Uint8Array(parts.reduce(function (a, b) { return a + b.length; }, 0));
    let at = 0;
    for (const p of parts) { out.set(p, at); at += p.length; }
    return out;
}
/* packets of `per` blocks each (multi), the stream's first block alone (a single-sample packet: it IS a frame) */
function packets(s, per) {
    const out = [{ bytes: s.blocks[0], multi: false }];
    for (let i = 1; i < s.blocks.length; i += per) out.push({ bytes: concat(s.blocks.slice(i, i + per)), multi: true });
    return out;
}
function mp4Decoder(s, shared, lookahead, frontend) {
    const dec = new host.GpuAACDecoder({ frontend: frontend || new host.FrontEnd(), lookahead: lookahead, shared: shared, format: { formatID: 'mp4a' } });
    dec.init(); dec.setCookie(s.cookie);
    return dec;
}
function adtsDecoder(s, shared, lookahead) {
    const dec = new host.GpuAACDecoder({ frontend: new host.FrontEnd(), lookahead: lookahead, shared: shared });
    dec.init();
    const demux = new host.adts.AdtsDemuxer(function (event, payload) {
        if (event === 'format') Object.assign(dec.format, payload);
        else if (event === 'cookie') dec.setCookie(payload);
        else if (event === 'data') dec.feed(payload);
    });
    demux.push(s.bytes);
    return dec;
}
/* every decoder read round robin until all are dry; a thrown error is an item of the output too (its message) */
function drain(decs) {
    const out = decs.map(function () { return []; });
    for (let live = decs.length; live;) {
        live = 0;
        decs.forEach(function (d, i) {
            let x;
            try { x = d.readChunk(); } catch (e) { out[i].push(e.message); live++; return; }
            if (x) { out[i].push(x.slice()); live++; }
        });
    }
    return out;
}
function same(a, b, what) {
    assert.strictEqual(a.length, b.length, what + ': frames ' + a.length + ' vs ' + b.length);
    a.forEach(function (x, t) {
        if (typeof x === 'string' || typeof b[t] === 'string') { assert.strictEqual(x, b[t], what + ' item ' + t); return; }
        assert.ok(Buffer.from(x.buffer, x.byteOffset, x.byteLength).equals(Buffer.from(b[t].buffer, b[t].byteOffset, b[t].byteLength)), what + ': frame ' + t + ' differs');
    });
}

if (mode === 'cpu') {
    /* routing: takesResident needs nothing but the decoder's cookie and format */
    const mk = function (formatID, o) { return Object.assign({ config: { profile: 2, chanConfig: 2, sampleIndex: 3 }, format: { formatID: formatID } }, o || {}); };
    const on = new host.SharedEngine({ resident: true, residentPackets: true }), off = new host.SharedEngine({ resident: true });
    assert.ok(on.takesResident(mk('mp4a')), "residentPackets: an 'mp4a' decoder takes the resident route");
    assert.ok(!off.takesResident(mk('mp4a')), "without residentPackets an 'mp4a' decoder takes the parsing route");
    assert.ok(on.takesResident(mk('aac ')) && off.takesResident(mk('aac ')) && off.takesResident(mk(undefined)), 'ADTS decoders are resident either way');
    assert.ok(!new host.SharedEngine({ residentPackets: true }).takesResident(mk('mp4a')), 'residentPackets alone does not make an engine resident');
    assert.ok(!on.takesResident(mk('mp4a', { tnsMode: 1 })) && !on.takesResident(mk('mp4a', { config: { profile: 1, chanConfig: 2 } })), 'spec modes and other profiles stay off');
    console.log('mp4a resident cpu tests ok');
    process.exit(0);
}

const S = names.map(load);
/* what the ADTS streams give on the resident route: the yardstick for the same blocks as MP4 samples */
function adtsResident() {
    const sh = new host.SharedEngine({ maxStreams: 16, maxChannels: 8, resident: true, lookahead: 4 });
    const decs = S.map(function (s) { return adtsDecoder(s, sh, 4); });
    assert.ok(decs.every(function (d) { return d.resident; }));
    return drain(decs);
}
const want = adtsResident();
want.forEach(function (w, i) { assert.strictEqual(w.length, S[i].list.length, names[i] + ': ADTS frames'); });

/* the streams as MP4 chunks, fed packet by packet between reads, with three ADTS streams on the same engine */
function mp4Run(opts, per, what, upFront) {
    const sh = new host.SharedEngine(Object.assign({ maxStreams: 16, maxChannels: 8, resident: true, residentPackets: true }, opts));
    const L = opts.lookahead;
    const mp4 = S.map(function (s) { return mp4Decoder(s, sh, L); });
    const adts = [0, 1, 2].map(function (i) { return adtsDecoder(S[i], sh, L); });
    assert.ok(mp4.concat(adts).every(function (d) { return d.resident; }), what + ': every decoder resident');
    const pk = S.map(function (s) { return packets(s, per); });
    const out = S.map(function () { return []; }), aout = adts.map(function () { return []; });
    /* upFront: every packet before the first read (with a PCM ring a queued frame is valid for K - 1 more flushes, and a reader fed
     * a packet at a time makes a flush whenever it runs dry — the ring's contract, not the route's) */
    if (upFront) { mp4.forEach(function (d, i) { for (const q of pk[i]) d.feedPacket(q.bytes, q.multi); }); pk.forEach(function (l) { l.length = 0; }); }
    for (let round = 0; ; round++) {
        let live = 0;
        mp4.forEach(function (d, i) {
            if (round < pk[i].length) { d.feedPacket(pk[i][round].bytes, pk[i][round].multi); live++; }
            const x = d.readChunk();
            if (x) { out[i].push(x.slice()); live++; }
        });
        adts.forEach(function (d, i) { const x = d.readChunk(); if (x) { aout[i].push(x.slice()); live++; } });
        if (!live) break;
    }
    out.forEach(function (o, i) { same(o, want[i], what + ' ' + names[i]); });
    aout.forEach(function (o, i) { same(o, want[i], what + ' ADTS ' + names[i]); });
}
mp4Run({ lookahead: 4 }, 3, 'lookahead 4, 3 blocks per packet');
mp4Run({ lookahead: 4, overlap: false }, 3, 'overlap off');
mp4Run({ lookahead: 4, pcmRing: 8 }, 5, 'pcmRing 8', true);
mp4Run({ lookahead: 16 }, 40, 'lookahead 16, 40 blocks per packet (walks resume)');

/* errors: a packet that ends inside a block and a packet with a corrupted block in the middle — frames and errors in the order
 * the parsing route gives (same engine kind, 'mp4a' without residentPackets) */
{
    const s = S[0], n = s.blocks.length;
    const bad = s.blocks[4].slice(); bad[0] = 0xA0; bad[1] = 0xFF;           // element type 5 (PCE): 'TODO: PCE_ELEMENT'
    const feed = [concat(s.blocks.slice(0, 3)), concat([s.blocks[3], bad, s.blocks[5]]), concat(s.blocks.slice(6, n - 1)),
                  s.blocks[n - 1].subarray(0, s.blocks[n - 1].length >> 1)];
    const run = function (residentPackets) {
        const sh = new host.SharedEngine({ maxStreams: 4, maxChannels: 8, resident: true, residentPackets: residentPackets, lookahead: 4 });
        const d = mp4Decoder(s, sh, 4);
        assert.strictEqual(!!d.resident, residentPackets);
        const out = [];
        for (const b of feed) d.feedPacket(b, true);
        for (let k = 0; k < 4 * n; k++) {
            let x;
            try { x = d.readChunk(); } catch (e) { out.push(e.message); continue; }
            if (!x) break;
            out.push(x.slice());
        }
        return out;
    };
    const got = run(true), ref = run(false);
    const msgs = function (o) { return o.map(function (x, t) { return typeof x === 'string' ? t + ':' + x : null; }).filter(Boolean); };
    assert.deepStrictEqual(msgs(got), msgs(ref), 'errors where the parsing route raises them');
    assert.ok(msgs(got).length === 2, 'two errors: ' + JSON.stringify(msgs(got)));
    const firstErr = got.findIndex(function (x) { return typeof x === 'string'; });
    same(got.slice(0, firstErr), ref.slice(0, firstErr), 'frames before the first error');
    same(got.slice(0, firstErr), want[0].slice(0, firstErr), 'frames before the first error against ADTS');
}
console.log('mp4a resident gpu tests ok');
