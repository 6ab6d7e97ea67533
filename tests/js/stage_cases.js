#!/usr/bin/env node
/*
 * tests/js/stage_cases.js — TEST KIT: ADTS streams for the spec-correct stages on the resident route
 * (tests/test_resident_stages_gpu.py): frames with TNS filters, noise bands and pulse data throughout.
 *
 *   node tests/js/stage_cases.js <outdir>
 *
 * Writes, with the synthetic writer (aac_writer.js) and the random-frame generator (stream_cases.js: randomFrame with
 * { tns, pns, pulse }), one stream of 12 ADTS frames per case — mono, stereo, stereo with split windows, 5.1, at two sample
 * indexes whose long and short TNS band limits differ (48 kHz: 40 / 14, 16 kHz: 42 / 14 of other band tables) — and a
 * manifest.  Pipelines that decode them take AACG_PARSE_APPLY_PULSES.
 * The seeds are fixed: chosen so that the JavaScript front end parses every frame (a random pulse may leave the spectrum), at
 * least a quarter of the channel-frames end with a filter to run and at least a tenth of the units carry noise bands; the test
 * asserts all three again from what the device returns.  AACG_STAGE_SEEDS="name=seed,..." overrides them (the search for them).
 */
'use strict';
const fs = require('fs'), path = require('path');
const root = path.join(__dirname, '..', '..');
const codebooks = require(path.join(root, 'aac.js_amd', 'js', 'codebooks.js'));
const { FrontEnd } = require(path.join(root, 'aac.js_amd', 'js', 'frontend.js'));
const { Writer, Rng } = require('./aac_writer.js');
const { randomFrame, layoutChannels, PATTERN } = require('./stream_cases.js');

const outdir = process.argv[2];
if (!outdir) { console.error('usage: stage_cases.js <outdir>'); process.exit(2); }
fs.mkdirSync(outdir, { recursive: true });
const cb = codebooks.standard();

const FRAMES = 12;
const STAGE_CASES = [
    { name: 'mono48', si: 3, layout: ['sce'], chanConfig: 1, seed: 203 },
    { name: 'stereo48', si: 3, layout: ['cpe'], chanConfig: 2, seed: 102 },
    { name: 'split48', si: 3, layout: ['cpe'], chanConfig: 2, noCommon: true, seed: 403 },
    { name: 'five1_48', si: 3, layout: ['sce', 'cpe', 'cpe', 'lfe'], chanConfig: 6, seed: 104 },
    { name: 'mono16', si: 8, layout: ['sce'], chanConfig: 1, seed: 105 },
    { name: 'stereo16', si: 8, layout: ['cpe'], chanConfig: 2, seed: 106 },
    { name: 'split16', si: 8, layout: ['cpe'], chanConfig: 2, noCommon: true, seed: 306 },
    { name: 'five1_16', si: 8, layout: ['sce', 'cpe', 'cpe', 'lfe'], chanConfig: 6, seed: 108 },
];
for (const kv of (process.env.AACG_STAGE_SEEDS || '').split(',')) {
    const m = /^(\w+)=(\d+)$/.exec(kv);
    if (m) for (const c of STAGE_CASES) if (c.name === m[1]) c.seed = parseInt(m[2], 10);
}

const manifest = [];
for (const c of STAGE_CASES) {
    const wr = new Writer(cb, c.si), rng = new Rng(c.seed >>> 0), chunks = [];
    const fe = new FrontEnd({ codebooks: cb, referenceQuirks: true });
    let parsed = 0, units = 0, pnsUnits = 0, tnsChannels = 0, channels = 0;
    for (let t = 0; t < FRAMES; t++) {
        const elements = randomFrame(wr, rng, c.layout, function (ei) { return PATTERN[(t + ei) % PATTERN.length]; },
                                     { tns: true, pns: true, pulse: true, noCommon: !!c.noCommon });
        const bytes = wr.adtsFrame(elements, c.chanConfig);
        chunks.push(Buffer.from(bytes));
        fe.pushPacket(bytes);
        try {
            const frame = fe.parseFrame({ config: { sampleIndex: c.si } });
            parsed++;
            for (const e of frame.elements) { units++; if (e.hasPns) pnsUnits++; for (const ch of e.ch) { channels++; if (ch.tns) tnsChannels++; } }
        } catch (err) { /* counted as not parsed: the manifest says so */ }
    }
    fs.writeFileSync(path.join(outdir, c.name + '.aac'), Buffer.concat(chunks));
    manifest.push({ name: c.name, sampleIndex: c.si, channels: layoutChannels(c.layout), elements: c.layout.length, frames: FRAMES, seed: c.seed,
                    parsed: parsed, units: units, pnsUnits: pnsUnits, channelFrames: channels, tnsChannels: tnsChannels });
}
/* one more, for the refusal that stays: a mono stream of plain long frames whose frame 5 carries a TNS filter of order 13 — inside
 * the syntax (tns.js:84 accepts up to 20), beyond AACG_TNS_MAX_ORDER: refused where TNS records are made, decoded elsewhere */
{
    const wr = new Writer(cb, 3), rng = new Rng(1313), chunks = [], odd = 5;
    for (let t = 0; t < FRAMES; t++) {
        const ch = wr.randomChannel(rng, { seq: 0 });
        if (t === odd) {
            const field = [];
            for (let i = 0; i < 13; i++) field.push(rng.below(16));
            ch.tns = { res: [1], filt: [[{ length: 12, order: 13, direction: false, compress: 0, field: field }]] };
        }
        chunks.push(Buffer.from(wr.adtsFrame([{ type: 'sce', id: 0, ch: [ch] }], 1)));
    }
    fs.writeFileSync(path.join(outdir, 'order13.aac'), Buffer.concat(chunks));
    manifest.push({ name: 'order13', sampleIndex: 3, channels: 1, elements: 1, frames: FRAMES, parsed: FRAMES, oddFrame: odd });
}
fs.writeFileSync(path.join(outdir, 'manifest.json'), JSON.stringify(manifest));
console.log('stage cases written: ' + manifest.length);
