#!/usr/bin/env node
/*
 * tests/js/shape_cases.js — TEST KIT: plain ADTS streams for the carried window shape on the resident route
 * (tests/test_resident_shape_gpu.py): no TNS filter, no noise band, no pulse data — what differs between a decoder that windows a
 * frame's first half with the previous frame's shape and one that always takes sine is then the window alone.
 *
 *   node tests/js/shape_cases.js <outdir>
 *
 * The eight cases of tests/js/stage_cases.js with its seeds (203, 102, 403, 104, 105, 106, 306, 108), five1_48 apart: with its seed
 * there, 104, the second channel goes from sine to KBD in frame 3 and never back; 304 here.  Generated with { tns: false, pns: false, pulse: false }: one stream of 12 ADTS
 * frames per case — mono, stereo, stereo with split windows, 5.1, at sample indexes 3 and 8 — and a manifest.  With these seeds the
 * JavaScript front end parses every frame, no unit has noise bands, every channel changes its shape both ways, and frame 3 or
 * frame 7 is KBD in some channel (at 4 frames a batch KBD is carried across a batch boundary); the manifest says so per stream
 * (kbdAtBoundary, bothWays) and the test asserts all of it again from the device parser's records.
 */
'use strict';
const fs = require('fs'), path = require('path');
const root = path.join(__dirname, '..', '..');
const codebooks = require(path.join(root, 'aac.js_amd', 'js', 'codebooks.js'));
const { FrontEnd } = require(path.join(root, 'aac.js_amd', 'js', 'frontend.js'));
const { Writer, Rng } = require('./aac_writer.js');
const { randomFrame, layoutChannels, PATTERN } = require('./stream_cases.js');

const outdir = process.argv[2];
if (!outdir) { console.error('usage: shape_cases.js <outdir>'); process.exit(2); }
fs.mkdirSync(outdir, { recursive: true });
const cb = codebooks.standard();

const FRAMES = 12;
const SHAPE_CASES = [
    { name: 'mono48', si: 3, layout: ['sce'], chanConfig: 1, seed: 203 },
    { name: 'stereo48', si: 3, layout: ['cpe'], chanConfig: 2, seed: 102 },
    { name: 'split48', si: 3, layout: ['cpe'], chanConfig: 2, noCommon: true, seed: 403 },
    { name: 'five1_48', si: 3, layout: ['sce', 'cpe', 'cpe', 'lfe'], chanConfig: 6, seed: 304 },
    { name: 'mono16', si: 8, layout: ['sce'], chanConfig: 1, seed: 105 },
    { name: 'stereo16', si: 8, layout: ['cpe'], chanConfig: 2, seed: 106 },
    { name: 'split16', si: 8, layout: ['cpe'], chanConfig: 2, noCommon: true, seed: 306 },
    { name: 'five1_16', si: 8, layout: ['sce', 'cpe', 'cpe', 'lfe'], chanConfig: 6, seed: 108 },
];

const manifest = [];
for (const c of SHAPE_CASES) {
    const wr = new Writer(cb, c.si), rng = new Rng(c.seed >>> 0), chunks = [];
    const fe = new FrontEnd({ codebooks: cb, referenceQuirks: true });
    let parsed = 0, pnsUnits = 0;
    const shapes = [];                                     // [frame][channel]
    for (let t = 0; t < FRAMES; t++) {
        const elements = randomFrame(wr, rng, c.layout, function (ei) { return PATTERN[(t + ei) % PATTERN.length]; },
                                     { tns: false, pns: false, pulse: false, noCommon: !!c.noCommon });
        const bytes = wr.adtsFrame(elements, c.chanConfig);
        chunks.push(Buffer.from(bytes));
        fe.pushPacket(bytes);
        try {
            const frame = fe.parseFrame({ config: { sampleIndex: c.si } });
            parsed++;
            const row = [];
            for (const e of frame.elements) { if (e.hasPns) pnsUnits++; for (const ch of e.ch) row.push(ch.windowShape | 0); }
            shapes.push(row);
        } catch (err) { shapes.push([]); }
    }
    const C = layoutChannels(c.layout);
    let bothWays = parsed === FRAMES;
    for (let ch = 0; ch < C && bothWays; ch++) {
        let up = false, down = false;
        for (let t = 1; t < FRAMES; t++) { up = up || (shapes[t - 1][ch] === 0 && shapes[t][ch] === 1); down = down || (shapes[t - 1][ch] === 1 && shapes[t][ch] === 0); }
        bothWays = up && down;
    }
    const kbdAtBoundary = parsed === FRAMES && (shapes[3].indexOf(1) >= 0 || shapes[7].indexOf(1) >= 0);
    fs.writeFileSync(path.join(outdir, c.name + '.aac'), Buffer.concat(chunks));
    manifest.push({ name: c.name, sampleIndex: c.si, channels: C, elements: c.layout.length, frames: FRAMES, seed: c.seed,
                    parsed: parsed, pnsUnits: pnsUnits, bothWays: bothWays, kbdAtBoundary: kbdAtBoundary });
}
fs.writeFileSync(path.join(outdir, 'manifest.json'), JSON.stringify(manifest));
console.log('shape cases written: ' + manifest.length);
