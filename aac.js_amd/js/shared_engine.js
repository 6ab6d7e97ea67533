/*
 * aac.js_amd/js/shared_engine.js — one engine for many decoders: cross-stream batching behind the plugin surface.
 *
 * The reference is one AACDecoder per stream (src/decoder.js:125-216): N concurrent Aurora players are N decoders, and a
 * GpuAACDecoder on its own hands the GPU its OWN stream's look-ahead (16 frames = one workgroup of a 256-CU chip).  Decoders
 * created with { shared: sharedEngine } instead take a stream slot each of an engine they share — one engine per sample rate,
 * which fixes the scalefactor-band tables — and whenever one of them runs out of decoded frames, readChunk() has EVERY
 * registered decoder parse ahead what it has buffered and submits all of it as ONE batch:
 *
 *   const shared = new SharedEngine({ maxStreams: 256, maxChannels: 8 });
 *   const dec = new GpuAACDecoder({ shared, frontend, lookahead: 16 });  ...  dec.readChunk()
 *
 * The surface stays the reference's (init / setCookie / readChunk, synchronous); a stream's frames still come back in order,
 * a malformed frame's error is still thrown by the readChunk call that reaches it, and a stream's PCM does not depend on
 * which other streams shared its batches (streams only meet in the launch: no arithmetic crosses them).  An engine error
 * raised BEFORE anything was launched (a refused unit, a capacity or layout error) is retried decoder by decoder, so that it
 * only costs the stream that caused it; a device error goes to every stream of the batch (their state may have moved).
 *
 * { resident: true } — the front end on the device as well: the decoders do not parse at all.  Each keeps the bytes its
 * demuxer fed it; a flush finds the next frames' boundaries (the 13-bit ADTS frame_length: six byte reads per frame), hands the
 * bytes of ALL streams to ONE native call (aacg_pipeline_decode: bit streams up, parse kernel, kept plan refreshed on the device,
 * transform kernel, PCM down) and slices what comes back.  JavaScript touches no coefficient and no unit record; what
 * readChunk() returns are views of the batch's PCM array.  For ADTS byte streams of any channel configuration 1..8 (one
 * pipeline per sample rate and channel count; a stream's element layout — SCE + CPE + CPE + LFE, say — is learnt on the device
 * from its first frame, coupling elements are parsed and dropped), as the reference executes them (TNS identity, no PNS) or, on a
 * SharedEngine made with { tnsMode, pnsMode }, with the spec-correct TNS filters and noise bands (aacg_pipeline_config.stages: the
 * TNS records are made on the device; float32 PCM).  MP4 samples ('mp4a': packets without ADTS headers, several to a buffer, whose
 * boundaries only a parse finds) and decoders with cceMode take the parsing route above on the same SharedEngine, and so does a
 * decoder whose carryWindowShape is not the SharedEngine's ({ resident: true, carryWindowShape: true }: each channel's window shape is
 * carried from frame to frame on the device, aacg_pipeline_config.stages bit 2; with int16 PCM too) — unless
 * { residentPackets: true }: then an 'mp4a' decoder takes the resident route too.  A single-sample packet is a frame; the blocks
 * of a multi-sample packet are found on the device (aacg_pipeline_walk_submit: one GPU lane walks one packet), a flush ahead of
 * the flush that decodes them, and then travel like ADTS frames.
 * { resident: true, ragged: true } — a flush takes from each stream what it has buffered, up to lookahead frames, instead of
 * cutting every stream to the count of the one with the fewest (aacg_pipeline_submit_ragged: per-stream frame counts, frames and
 * PCM packed stream after stream); one stream with a single frame buffered no longer makes the whole flush a one-frame batch.
 * { resident: true, ragged: true, devicePlans: true } — ragged flushes seldom repeat a batch shape, and a kept plan per shape then
 * means a plan built, uploaded and evicted per flush; with devicePlans a pipeline has ONE plan, shaped on the device for every
 * batch (aacg_pipeline_config.plan_mode 1).  Off by default: INTEGRATION.md says when to switch it on.
 * { resident: true, downmix: 'stereo' | 'mono' | { outChannels, matrix } } — every decoder of the engine delivers outChannels (1 or
 * 2) channels instead of its stream's: the standard matrix for the stream's channel count (aacg_mix_standard) or the caller's, one per
 * engine.  A resident pipeline mixes on the device (aacg_pipeline_set_mix: a 5.1 stream then costs the link what a stereo stream
 * costs) and a decoder on the parsing route is mixed on the host by the same rule (mix.js), bit for bit; format.channelsPerFrame says
 * outChannels either way.
 * { resident: true, sampleRate: 16000 } — every decoder of the engine delivers PCM at that rate instead of its stream's: the default
 * table (aacg_resample_design, 32 taps) from the stream's rate, one per pipeline.  A resident pipeline resamples on the device, behind
 * the mix (aacg_pipeline_set_resample: a 48 kHz stream at 16 kHz sends a third of the samples down the link), and readChunk() returns
 * each frame's share of the output, 341 or 342 samples per channel for 1024 at 1 / 3 — a variable length; a decoder on the parsing
 * route is resampled on the host by the same rule (resample.js), bit for bit; format.sampleRate says the new rate either way.  A stream
 * that has the engine's rate already is left alone.
 * { trim: true } — opt-in; without it nothing differs.  Every decoder of the engine then has decoder.setTrim(skip, length): a window in
 * samples of the stream's OWN rate (numbers, exact below 2^53; length left out: all of the rest) — the encoder's priming off the front,
 * the padding off the end.  With sampleRate the engine converts it with the addon's trimDesign (aacg_trim_design: the resampler's
 * group delay compensated, the residual in decoder.trimResidual).  A resident pipeline trims on the device (aacg_pipeline_set_trim:
 * only the kept samples come down) and a batch is sliced frame by frame by aacg_trim_counts' rule (trim.js): a frame that owns no
 * kept sample delivers no chunk, a refused frame's Error is delivered wherever it lies.  Decoders on the parsing route trim on the
 * host by the same rule, so that both routes deliver the same chunks with the same lengths.
 * { resident: true, ragged: true, devicePlans: true, conceal: true | { fadeSteps, holdFrames } } — a frame the device refuses (a cut
 * packet, a bad scalefactor, a changed layout) repeats its stream's last good frame, fadeSteps scalefactor steps (1.5 dB; default 2)
 * further down per lost frame, for at most holdFrames (default 6) frames in a row (aacg_pipeline_set_concealment: the frame's records
 * are substituted on the device, in front of the transform).  readChunk() then delivers that frame's PCM instead of queueing the
 * reference's Error, and stats.concealedFrames counts such frames; a refused frame that was not concealed — no good frame yet, or the
 * run is longer than holdFrames — still throws.  The option needs devicePlans and throws at construction without it.
 * Replaces, per batch, what src/decoder.js:125-216 does per frame.
 */
'use strict';
const host = require('./index.js');

function SharedEngine(opts) {
    opts = opts || {};
    this.opts = opts;
    this.maxStreams = opts.maxStreams || 256;
    this.maxChannels = opts.maxChannels || 8;
    this.groups = new Map();                              // sampleIndex -> { engine, decoders: [], free: [] }
    this.resident = !!opts.resident;                      // bytes -> PCM in one native call per flush (aacg_pipeline_*)
    this.residentPackets = !!opts.residentPackets;        // resident: 'mp4a' decoders too (their blocks found by a walk on the device)
    this.lookahead = opts.lookahead || 16;                // resident: frames per stream and flush
    this.ragged = !!opts.ragged;                          // resident: each stream's own frame count per flush (at most lookahead)
    this.devicePlans = !!opts.devicePlans;                // resident: one plan per pipeline, shaped on the device batch by batch (plan_mode 1)
    /* resident: where a flush's PCM lives.  0 (default): memory of its own, the caller's for as long as it keeps any frame of the
     * flush (what the reference's readChunk() promises: a fresh array per frame) — a page-locked allocation per flush.  K > 0: K
     * page-locked buffers made once and used in turn: a frame is valid until its SharedEngine has flushed K more times, i.e. for
     * at least (K - 1) x lookahead further frames of its stream; a consumer that keeps frames longer copies them (frame.slice()) */
    this.pcmRing = opts.pcmRing | 0;
    /* resident: decode the NEXT flush's batch while the caller consumes this one (addon.pipelineSubmit / pipelineCollect:
     * aacg_pipeline_submit enqueues the batch on one of the pipeline's lanes and returns; no thread of the addon's is involved).
     * A flush then collects the batch submitted by the flush before and submits the one after; streams are read one flush
     * (lookahead frames) further ahead than they are consumed, and with pcmRing a frame is valid for one flush less.  On by
     * default since round 6 ({ overlap: false } for a flush that decodes what it returns). */
    this.overlap = opts.overlap === undefined ? this.resident : !!opts.overlap;
    this.sampleRate = opts.sampleRate ? opts.sampleRate | 0 : 0;      // the rate every decoder delivers (resample.js); 0: its stream's
    this.downmix = opts.downmix || null;                  // 'stereo' | 'mono' | { outChannels, matrix }: what every decoder delivers (mix.js)
    /* resident, devicePlans: refused frames repeat the stream's last good frame, fading (aacg_pipeline_set_concealment) */
    this.conceal = null;
    if (opts.conceal) {
        if (!this.resident || !this.devicePlans) throw new Error('SharedEngine: conceal needs { resident: true, devicePlans: true } (the stage runs on a plan shaped on the device)');
        const c = opts.conceal === true ? {} : opts.conceal;
        this.conceal = { fadeSteps: c.fadeSteps === undefined ? 2 : c.fadeSteps | 0, holdFrames: c.holdFrames === undefined ? 6 : c.holdFrames | 0 };
    }
    this.trim = !!opts.trim;                              // decoder.setTrim(skip, length): trimmed on the device (resident) or by trim.js
    this.stats = { batches: 0, frames: 0, units: 0, engineNs: 0n, retries: 0, flushNs: 0n, concealedFrames: 0 };   // flushNs: resident flushes, host side and native calls
}

/* error codes the engine raises before it has launched anything (include/aacgpu.h): a batch refused with one of these has
 * advanced no stream, and may be retried in parts */
const PARSE_CONCEALED = 0x8;                              // AACG_PARSE_CONCEALED: byte 3 (flags) of a frame's 8-byte result
const BEFORE_LAUNCH = [-1, -4, -5, -6];                   // INVALID_ARG, CAPACITY, UNSUPPORTED, LAYOUT_CHANGE
function refusedBeforeLaunch(err) {
    const m = /failed \((-?\d+)\)/.exec(String(err && err.message));
    return !!m && BEFORE_LAUNCH.indexOf(parseInt(m[1], 10)) >= 0;
}

/* called by GpuAACDecoder.setCookie: the engine for the decoder's sample rate and a stream slot in it */
SharedEngine.prototype.attach = function (dec) {
    const cfg = dec.config;
    if (cfg.chanConfig + dec.maxCoupling > this.maxChannels) throw new Error('SharedEngine: ' + cfg.chanConfig + ' channels exceed maxChannels ' + this.maxChannels);
    if (dec.group) this.detach(dec);                       // a new cookie: a new stream
    /* downmix: the matrix for this stream's channel count; the decoder says what it delivers, and mixes on the host where its
     * frames do not come from a resident pipeline (GpuAACDecoder.deliver) */
    dec.mix = this.downmix ? require('./mix.js').resolve(this.downmix, cfg.chanConfig, this.opts.addon || host.loadAddon()) : null;
    if (dec.mix) dec.format.channelsPerFrame = dec.mix.outChannels;
    /* sampleRate: the table from this stream's rate, and a resampler of the decoder's own — on the parsing route it filters the frames
     * (GpuAACDecoder.deliver), on the resident route only its clock is used: it says each frame's share of a batch's ragged output */
    dec.resampleSpec = this.sampleRate ? require('./resample.js').resolve(this.sampleRate, host.SAMPLE_RATES[cfg.sampleIndex], this.opts.addon || host.loadAddon()) : null;
    dec.resampler = dec.resampleSpec ? new (require('./resample.js').Resampler)(dec.resampleSpec, dec.mix ? dec.mix.outChannels : cfg.chanConfig) : null;
    if (dec.resampleSpec) dec.format.sampleRate = this.sampleRate;
    /* trim: the decoder's window and position in samples of what it delivers (trim.js) — on the parsing route it cuts the chunks, on
     * the resident route it mirrors the slot's on the device and says each frame's share of a batch's kept samples.  submitN0: the
     * resampler's clock where the next batch to be ENQUEUED begins (the decoder's own resampler keeps the one of the next DELIVERED) */
    dec.trimmer = this.trim ? new (require('./trim.js').Trimmer)(dec.mix ? dec.mix.outChannels : cfg.chanConfig, 0) : null;
    dec.submitN0 = 0;
    if (this.trim) { const shared = this; dec.setTrim = function (skip, length) { shared.setTrim(dec, skip, length); }; }
    if (this.takesResident(dec)) return this.attachResident(dec);
    let g = this.groups.get(cfg.sampleIndex);
    if (!g) {
        const o = this.opts;
        const engine = o.engine ? o.engine(cfg.sampleIndex) :
            new host.Engine({ sampleIndex: cfg.sampleIndex, maxStreams: this.maxStreams, maxChannels: this.maxChannels, inputKind: host.INPUT_QUANT_I16,
                              deviceOrdinal: o.deviceOrdinal | 0, tnsMode: o.tnsMode | 0, pnsMode: o.pnsMode | 0, cceMode: o.cceMode | 0 });
        g = { engine: engine, decoders: [], free: [], next: 0 };
        this.groups.set(cfg.sampleIndex, g);
    }
    if ((dec.tnsMode | 0) !== (this.opts.tnsMode | 0) || (dec.pnsMode | 0) !== (this.opts.pnsMode | 0) || (dec.cceMode | 0) !== (this.opts.cceMode | 0))
        throw new Error('SharedEngine: the decoder\'s tnsMode / pnsMode / cceMode differ from the shared engine\'s');
    const slot = g.free.length ? g.free.pop() : g.next++;
    if (slot >= this.maxStreams) { g.next--; throw new Error('SharedEngine: more than ' + this.maxStreams + ' streams at one sample rate'); }
    dec.engine = g.engine; dec.stream = slot; dec.group = g;
    g.decoders.push(dec);
};

/* whether a decoder (its cookie read) takes the resident route: the resident route reads ADTS frame lengths itself, and an 'mp4a'
 * track's samples have none (aurora.js feeds them through feedPacket — ADVICE round 5: such a decoder used to deliver nothing,
 * without an error); with residentPackets its packets are walked on the device instead */
SharedEngine.prototype.takesResident = function (dec) {
    const cfg = dec.config, id = dec.format ? dec.format.formatID : undefined;
    const adts = id === undefined || id === 'aac ', mp4a = this.residentPackets && id === 'mp4a';
    /* the spec-correct stages ride the resident route when the engine was made with them: the decoder's modes must be the engine's
     * (as on the parsing route), and the stages' launches write float32 PCM */
    const o = this.opts, stages = (o.tnsMode | 0) || (o.pnsMode | 0);
    const modes = (dec.tnsMode | 0) === (o.tnsMode | 0) && (dec.pnsMode | 0) === (o.pnsMode | 0) && !(stages && (o.outputKind | 0) === host.OUTPUT_I16);
    /* ... and so does the carried window shape ({ carryWindowShape: true }: the pipelines carry it on the device): a decoder that
     * wants it on an engine made without it, or the other way round, takes the parsing route */
    const shape = !!dec.carryWindowShape === !!o.carryWindowShape;
    return this.resident && (adts || mp4a) && cfg.profile === 2 && cfg.chanConfig >= 1 && cfg.chanConfig <= 8 && modes && !dec.cceMode && shape;
};

/* resident route: one pipeline (engine + parser on the device) per (sample rate, channel count) */
SharedEngine.prototype.attachResident = function (dec) {
    const cfg = dec.config, key = 'r' + cfg.sampleIndex + '/' + cfg.chanConfig;
    let g = this.groups.get(key);
    if (!g) {
        const addon = this.opts.addon || host.loadAddon(), rec = require('./codebooks.js').load(this.opts).toEntryRecords();
        const outI16 = (this.opts.outputKind | 0) === host.OUTPUT_I16;
        const create = { deviceOrdinal: this.opts.deviceOrdinal | 0, sampleIndex: cfg.sampleIndex, maxStreams: this.maxStreams,
                         channels: cfg.chanConfig, maxFrames: this.lookahead, outputKind: this.opts.outputKind | 0,
                         parseOptions: (this.opts.applyPulses ? 1 : 0) | (this.opts.referenceQuirks !== false ? 2 : 0),
                         planMode: this.devicePlans ? 1 : 0,
                         stages: ((this.opts.tnsMode | 0) ? 1 : 0) | ((this.opts.pnsMode | 0) ? 2 : 0) | (this.opts.carryWindowShape ? 4 : 0) };
        if (dec.mix) create.mix = { outChannels: dec.mix.outChannels, matrix: dec.mix.matrix };      // mixed on the device: outChannels leave
        if (dec.resampleSpec) create.resample = dec.resampleSpec;      // resampled on the device, behind the mix: ragged PCM comes back
        if (this.conceal) create.conceal = this.conceal;      // refused frames repeat the stream's last good frame on the device
        if (this.trim) create.trim = true;                    // each slot's window cut on the device, behind the resampler: ragged PCM comes back
        const pipeline = addon.pipelineCreate(create, rec.entries, rec.counts);
        /* channels: of the PCM that comes back — what sizes a flush's PCM and slices it into frames */
        g = { resident: true, trim: this.trim, resample: dec.resampleSpec, addon: addon, pipeline: pipeline, channels: dec.mix ? dec.mix.outChannels : cfg.chanConfig, outI16: outI16, decoders: [], free: [], next: 0, walks: [] };
        this.groups.set(key, g);
    }
    const slot = g.free.length ? g.free.pop() : g.next++;
    if (slot >= this.maxStreams) { g.next--; throw new Error('SharedEngine: more than ' + this.maxStreams + ' streams at one sample rate'); }
    dec.stream = slot; dec.group = g; dec.resident = true;
    dec.rbuf = new Uint8Array(0); dec.rpos = 0;
    /* 'mp4a': the packets in order, each { bytes, at: first byte not walked yet, ready: its blocks found and not yet taken, done,
     * inflight }; a new object per stream, so that a walk still in flight for the stream before is dropped when it comes back */
    dec.packets = dec.format && dec.format.formatID === 'mp4a' ? { q: [] } : null;
    dec.engine = { resetStream: function (s) { g.addon.pipelineResetStream(g.pipeline, s); if (dec.resampler) dec.resampler.reset(); dec.submitN0 = 0; if (dec.trimmer) dec.trimmer.reset(); } };
    if (dec.trimmer) g.addon.pipelineSetStreamTrim(g.pipeline, slot, 0);      // a slot handed on starts with the default window
    g.decoders.push(dec);
};

/* decoder.setTrim(skip, length) of a SharedEngine({ trim: true }): the window in samples of the stream's own rate -> the window of what
 * the decoder delivers (trimDesign where the engine resamples), set on the decoder's trimmer and, resident, on its slot of the pipeline:
 * from the next batch enqueued, the position at 0 */
SharedEngine.prototype.setTrim = function (dec, skip, length) {
    if (!dec.trimmer) throw new Error('SharedEngine: setTrim needs { trim: true }');
    let w = { skip: skip, keep: (length === undefined || length === null) ? null : length, residualNum: 0, residualDen: 1 };
    require('./trim.js').design(w.skip, w.keep, false);      // (the limits, stated once for both routes)
    if (dec.resampleSpec) w = (this.opts.addon || host.loadAddon()).trimDesign(skip, w.keep === null ? undefined : w.keep, false, dec.resampleSpec.L, dec.resampleSpec.M, dec.resampleSpec.taps);
    dec.trimmer.set(w.skip, w.keep);
    dec.trimResidual = { num: w.residualNum, den: w.residualDen };
    if (dec.resident) dec.group.addon.pipelineSetStreamTrim(dec.group.pipeline, dec.stream, w.skip, w.keep === null ? undefined : w.keep);
};

/* a trimmed resident batch, in front of its native call: each frame's share of its stream's kept samples, from the decoders' windows
 * and positions as they stand — which advance here, as the slots' do when the batch is enqueued.  -> what undoes it if the call fails */
SharedEngine.prototype.trimShares = function (g, b) {
    const rs = require('./resample.js'), tr = require('./trim.js'), R = g.resample, saved = [];
    b.kept = new Uint32Array(b.N);
    for (let s = 0; s < b.S; s++) {
        const dec = b.part[s], t = dec.trimmer;
        saved.push([dec, t.position, dec.submitN0]);
        for (let f = 0, i = b.first[s]; f < b.counts[s]; f++, i++) {
            const n = R ? rs.count(R.L, R.M, dec.submitN0, 1024) : 1024;
            if (R) dec.submitN0 = (dec.submitN0 + 1024) % R.M;
            b.kept[i] = tr.span(t.position, t.skip, t.keep, n).kept;
            t.position += n;
        }
    }
    return function () { for (const [dec, position, n0] of saved) { dec.trimmer.position = position; dec.submitN0 = n0; } };
};

SharedEngine.prototype.detach = function (dec) {
    const g = dec.group;
    if (!g) return;
    g.decoders.splice(g.decoders.indexOf(dec), 1);
    g.free.push(dec.stream);
    dec.group = null;
    if (dec.packets) dec.packets = { q: [] };              // a walk in flight for this stream is dropped when it comes back
};

/* GpuAACDecoder.feedPacket on the resident route: a single-sample packet is a frame; a multi-sample packet waits for a walk */
SharedEngine.prototype.pushPacket = function (dec, bytes, multi) {
    dec.packets.q.push(multi ? { bytes: bytes, at: 0, ready: [], done: bytes.length === 0, inflight: false } : { bytes: bytes, at: bytes.length, ready: [bytes], done: true, inflight: false });
};

/* the blocks a stream can hand to a batch now (at most `max`, into `out`): packets in order, up to the first one not walked to its end */
function packetFrames(pk, max, out) {
    let n = 0;
    for (const e of pk.q) {
        for (let i = 0; i < e.ready.length && n < max; i++) out[n++] = e.ready[i];
        if (n >= max || !e.done) break;
    }
    return n;
}
function takePacketFrames(pk, n) {
    while (pk.q.length) {
        const e = pk.q[0], k = Math.min(n, e.ready.length);
        e.ready.splice(0, k); n -= k;
        if (e.done && !e.ready.length) pk.q.shift(); else break;
    }
}

/* one walk over every packet not walked yet of the group's 'mp4a' streams (up to lookahead blocks each: a longer packet resumes at
 * bytes_consumed in the next walk), enqueued on the device (pipelineWalkSubmit) */
SharedEngine.prototype.walkSubmit = function (g) {
    const list = [];
    let total = 0;
    for (const dec of g.decoders) {
        if (!dec.packets) continue;
        for (const e of dec.packets.q) if (!e.done && !e.inflight) { list.push({ dec: dec, pk: dec.packets, e: e, from: e.at, base: total }); total += e.bytes.length - e.at; }
    }
    if (!list.length) return false;
    const M = this.lookahead, bytes = new Uint8Array(total), spans = new Uint32Array(2 * list.length);
    list.forEach(function (w, k) { bytes.set(w.e.bytes.subarray(w.from), w.base); spans[2 * k] = w.base; spans[2 * k + 1] = w.e.bytes.length - w.from; });
    const frames = new Uint32Array(2 * list.length * M), results = new Uint32Array(4 * list.length);
    try { g.addon.pipelineWalkSubmit(g.pipeline, bytes, spans, M, frames, results); }
    catch (err) { this.walkFailed(list, err); return false; }
    for (const w of list) w.e.inflight = true;
    g.walks.push({ list: list, frames: frames, results: results, M: M });
    return true;
};

/* the oldest walk in flight: its blocks to their packets, in order; a block that does not parse is kept with the rest of its packet
 * as its length — the pipeline refuses it with the same status and the reference's message is thrown where the frame is reached —
 * and the packet ends there (as on the parsing route) */
SharedEngine.prototype.walkCollect = function (g) {
    const w = g.walks.shift();
    try { g.addon.pipelineWalkCollect(g.pipeline); }
    catch (err) { this.walkFailed(w.list, err); return; }
    w.list.forEach(function (x, k) {
        const e = x.e;
        e.inflight = false;
        if (x.dec.packets !== x.pk) return;               // the stream was detached or reset since
        const n = w.results[4 * k], status = w.results[4 * k + 1], used = w.results[4 * k + 2];
        for (let f = 0, i = 2 * k * w.M; f < n; f++, i += 2) {
            const off = w.frames[i] - x.base + x.from;
            e.ready.push(e.bytes.subarray(off, off + w.frames[i + 1]));
        }
        e.at = x.from + used;
        e.done = status !== 0 || e.at >= e.bytes.length;
    });
};

SharedEngine.prototype.walkFailed = function (list, err) {
    const e = err instanceof Error ? err : new Error(String(err));
    for (const x of list) {
        x.e.inflight = false; x.e.done = true;
        if (x.dec.packets === x.pk && x.dec.queue.indexOf(e) < 0) x.dec.queue.push(e);
    }
};

/* before a batch is put together: the walks in flight come back, and a stream with no block ready but packets not walked yet is
 * walked now, synchronously (a readChunk() must not return null while a complete block is buffered) */
SharedEngine.prototype.walkReady = function (g, room) {
    while (g.walks.length) this.walkCollect(g);
    const want = new Array(1);
    const starving = g.decoders.some(function (dec) {
        return dec.packets && dec.queue.length < room && packetFrames(dec.packets, 1, want) === 0 && dec.packets.q.some(function (e) { return !e.done; });
    });
    if (starving && this.walkSubmit(g)) this.walkCollect(g);
};

/* how many complete ADTS frames (at most `max`) start at byte `at` of `b`: their lengths into `lens`; -1 where the bytes at a
 * frame boundary are not an ADTS header (the reference's 'Invalid ADTS header.', adts_demuxer.js:29) — or are one whose
 * frame_length is shorter than the header itself: a corrupt length field must not stall the stream silently (ADVICE round 5) */
function scanFrames(b, at, max, lens) {
    let n = 0;
    while (n < max && at + 7 <= b.length) {
        if (b[at] !== 0xff || (b[at + 1] & 0xf0) !== 0xf0) return n ? n : -1;
        const len = ((b[at + 3] & 3) << 11) | (b[at + 4] << 3) | (b[at + 5] >> 5);
        if (len < 7) return n ? n : -1;
        if (at + len > b.length) break;
        lens[n++] = len; at += len;
    }
    return n;
}

/* resident flush: the next frames of every stream that has run dry or has room, ONE native call, views of its PCM handed out */
SharedEngine.prototype.prepareResident = function (g, room) {
    const L = this.lookahead, ragged = this.ragged;
    const part = [], own = [];                             // own[s]: what participant s has buffered (at most L frames)
    let F = L;
    for (const dec of g.decoders) {
        if (dec.queue.length >= room) continue;            // a slow reader's queue does not grow with every flush of its peers
        if (!dec.rlens) dec.rlens = new Uint32Array(L);
        if (dec.packets) {                                 // 'mp4a': the blocks its walks have found
            if (!dec.rblocks) dec.rblocks = new Array(L);
            const n = packetFrames(dec.packets, L, dec.rblocks);
            for (let f = 0; f < n; f++) dec.rlens[f] = dec.rblocks[f].length;
            if (n) { part.push(dec); own.push(n); F = Math.min(F, n); }
            continue;
        }
        const n = scanFrames(dec.rbuf, dec.rpos, L, dec.rlens);
        if (n < 0) { if (!dec.badHeader) { dec.badHeader = true; dec.queue.push(new Error('Invalid ADTS header.')); } continue; }
        if (n === 0) continue;
        part.push(dec); own.push(n); F = Math.min(F, n);
    }
    if (!part.length) return null;
    /* counts[s]: stream s's frames in this batch — its own (ragged) or the fewest any participant has; first[s]: where they begin
     * in the batch's packed order (frames, results and PCM alike) */
    const S = part.length, counts = new Uint32Array(S), first = new Uint32Array(S + 1), slots = new Uint32Array(S), starts = new Uint32Array(S + 1);
    for (let s = 0; s < S; s++) { counts[s] = ragged ? own[s] : F; first[s + 1] = first[s] + counts[s]; }
    const N = first[S], frames = new Uint32Array(2 * N);
    let total = 0;
    for (let s = 0; s < S; s++) {
        const lens = part[s].rlens;
        starts[s] = total; slots[s] = part[s].stream;
        for (let f = 0, i = 2 * first[s]; f < counts[s]; f++, i += 2) { frames[i] = total; frames[i + 1] = lens[f]; total += lens[f]; }
    }
    starts[S] = total;
    const bytes = new Uint8Array(total);
    for (let s = 0; s < S; s++) {
        const dec = part[s], len = starts[s + 1] - starts[s], n = counts[s];
        if (dec.packets) {
            for (let f = 0, at = starts[s]; f < n; f++) { bytes.set(dec.rblocks[f], at); at += dec.rblocks[f].length; }
            for (let f = 0; f < own[s]; f++) dec.rblocks[f] = null;
            takePacketFrames(dec.packets, n);
            continue;
        }
        bytes.set(dec.rbuf.subarray(dec.rpos, dec.rpos + len), starts[s]);
        dec.rpos += len;
    }
    return { part: part, S: S, F: F, N: N, ragged: ragged, counts: counts, first: first, frames: frames, slots: slots, bytes: bytes, results: new Uint8Array(8 * N) };
};

/* the batch's PCM: one array on page-locked memory the device wrote into; a frame is a view of it (the memory returns to the
 * addon's pool when the last of the batch's frames has been collected) */
SharedEngine.prototype.deliverResident = function (g, b, out, failed) {
    const C = g.channels, part = b.part, S = b.S, results = b.results;
    this.stats.batches++; this.stats.units += b.N;
    if (failed) { for (const dec of part) dec.queue.push(failed); return; }
    const pcm = out.pcm, refused = out.refused, per = 1024 * C;
    if (g.trim) {
        /* ragged: stream s's out.lengths[s] kept samples lie behind those of the streams before it, frame f's share of them is
         * b.kept (trimShares).  A frame that owns no kept sample delivers no chunk; a refused frame's Error is delivered wherever it lies */
        for (let s = 0, at = 0; s < S; s++) {
            const q = part[s].queue, r = part[s].resampler;
            let sum = 0;
            for (let f = 0, i = b.first[s]; f < b.counts[s]; f++, i++) {
                const n = b.kept[i];
                if (r) r.n0 = (r.n0 + 1024) % g.resample.M;      // (the delivered clock goes on, as without the trim)
                const concealed = (results[8 * i + 3] & PARSE_CONCEALED) !== 0;
                if (concealed) this.stats.concealedFrames++;
                if (refused && results[8 * i] && !concealed) q.push(new Error(g.addon.parseStatusString(results[8 * i])));
                else if (n) q.push(pcm.subarray(at * C, (at + n) * C));
                at += n; sum += n;
            }
            if (sum !== out.lengths[s]) throw new Error('SharedEngine: the device kept ' + out.lengths[s] + ' samples of a stream where trim.js counts ' + sum);
        }
        this.stats.frames += b.N;
        return;
    }
    if (g.resample) {
        /* ragged: stream s's out.lengths[s] samples lie behind those of the streams before it, and frame f's share of them follows
         * from the stream's clock, which the decoder's resampler keeps (a refused frame was silence: its share is skipped, the clock
         * goes on) */
        const rs = require('./resample.js'), R = g.resample;
        for (let s = 0, at = 0; s < S; s++) {
            const q = part[s].queue, r = part[s].resampler;
            for (let f = 0, i = b.first[s]; f < b.counts[s]; f++, i++) {
                const n = rs.count(R.L, R.M, r.n0, 1024);
                r.n0 = (r.n0 + 1024) % R.M;
                const concealed = (results[8 * i + 3] & PARSE_CONCEALED) !== 0;
                if (concealed) this.stats.concealedFrames++;
                if (refused && results[8 * i] && !concealed) q.push(new Error(g.addon.parseStatusString(results[8 * i])));
                else q.push(pcm.subarray(at * C, (at + n) * C));
                at += n;
            }
        }
        this.stats.frames += b.N;
        return;
    }
    for (let s = 0; s < S; s++) {
        const q = part[s].queue;
        for (let f = 0, i = b.first[s]; f < b.counts[s]; f++, i++) {
            /* a frame the device refused: the reference's message for its status where the frame is reached (it was decoded as
             * silence: the stream goes on); a frame whose elements are not the ones its stream began with has a status of its own
             * (AACG_PARSE_LAYOUT, set where the plan's records are refreshed) */
            /* ... unless the device concealed it (AACG_PARSE_CONCEALED in the result's flags): then its PCM is the stream's last good
             * frame, faded, and is delivered */
            const concealed = (results[8 * i + 3] & PARSE_CONCEALED) !== 0;
            if (concealed) this.stats.concealedFrames++;
            if (refused && results[8 * i] && !concealed) q.push(new Error(g.addon.parseStatusString(results[8 * i])));
            else q.push(pcm.subarray(i * per, (i + 1) * per));
        }
    }
    this.stats.frames += b.N;
};

SharedEngine.prototype.flushResident = function (g) {
    const t = process.hrtime.bigint();
    try { this.flushResidentTimed(g); } finally { this.stats.flushNs += process.hrtime.bigint() - t; }
};

/* how many plans the resident pipelines have built (one per batch shape a pipeline had not kept) */
SharedEngine.prototype.planBuilds = function () {
    let n = 0;
    for (const g of this.groups.values()) if (g.resident && g.addon.pipelinePlanBuilds) n += g.addon.pipelinePlanBuilds(g.pipeline);
    return n;
};

/* the resident pipelines' transform launches, summed: { shaped: batches whose plan was shaped on the device (devicePlans),
 * chained: launches that continued their predecessor through the cross-launch cells, launches } */
SharedEngine.prototype.launchCounts = function () {
    const n = { shaped: 0, chained: 0, launches: 0 };
    for (const g of this.groups.values())
        if (g.resident && g.addon.pipelineLaunchCounts) {
            const c = g.addon.pipelineLaunchCounts(g.pipeline);
            n.shaped += c.shaped; n.chained += c.chained; n.launches += c.launches;
        }
    return n;
};

SharedEngine.prototype.flushResidentTimed = function (g) {
    const L = this.lookahead, C = g.channels;
    /* (a resampled batch: a stream of L frames emits at most ceil(1024 L x L' / M') samples whatever its clock) */
    const ringElems = this.pcmRing ? this.maxStreams * (g.resample ? Math.ceil(L * 1024 * g.resample.L / g.resample.M) : L * 1024) * C : 0;
    const args = (b) => [g.pipeline, b.bytes, b.frames, b.slots, b.ragged ? b.counts : b.F, b.results, C, this.pcmRing, ringElems];
    const t0 = process.hrtime.bigint();
    let b = null, out = null, failed = null;
    if (this.overlap && g.pending) {                       // the batch the flush before this one submitted
        b = g.pending; g.pending = null;
        try { out = g.addon.pipelineCollect(g.pipeline); } catch (err) { failed = err instanceof Error ? err : new Error(String(err)); }
    } else {
        this.walkReady(g, L);
        b = this.prepareResident(g, L);
        if (!b) return;
        const undo = g.trim ? this.trimShares(g, b) : null;
        try { out = g.addon.pipelineDecode.apply(null, args(b)); } catch (err) { failed = err instanceof Error ? err : new Error(String(err)); if (undo) undo(); }
    }
    this.stats.engineNs += process.hrtime.bigint() - t0;
    this.deliverResident(g, b, out, failed);
    if (this.overlap && !failed) {                         // ... and the one after it: decoded while the caller reads this one
        this.walkReady(g, 2 * L);
        const nb = this.prepareResident(g, 2 * L);
        if (nb) {
            const undo = g.trim ? this.trimShares(g, nb) : null;
            try { g.addon.pipelineSubmit.apply(null, args(nb)); g.pending = nb; }
            catch (err) { if (undo) undo(); this.deliverResident(g, nb, null, err instanceof Error ? err : new Error(String(err))); }
        }
    }
    if (!g.walks.length) this.walkSubmit(g);               // the packets not walked yet: on the device while the caller reads this flush
};

/* every registered decoder parses ahead what it has buffered; one batch per engine */
SharedEngine.prototype.flush = function () {
    for (const g of this.groups.values()) this.flushGroup(g);
};

SharedEngine.prototype.flushGroup = function (g) {
    if (g.resident) return this.flushResident(g);
    const tnsList = (this.opts.tnsMode | 0) === host.TNS_SPEC ? [] : null, cceList = (this.opts.cceMode | 0) === host.CCE_SPEC ? [] : null;
    const parts = [];
    let block = 0, pcmAt = 0;
    for (const dec of g.decoders) {
        let part;
        if (dec.failedProfile || dec.queue.length >= dec.lookahead) continue;     // a paused reader's queue does not grow with every flush of its peers
        try { part = dec.collectAhead(block, pcmAt, tnsList, cceList); }
        catch (err) { dec.failedProfile = true; dec.queue.push(err instanceof Error ? err : new Error(String(err))); continue; }    // unsupported profile: that decoder's own error, once
        if (!part.frames.length) { dec.deliver(part, null, 0, null); continue; }
        part.dec = dec; part.blockBase = block; part.pcmBase = pcmAt;
        /* where this part's TNS / coupling records sit in the shared lists is already in its units */
        parts.push(part);
        block += part.nBlocks;
        pcmAt += part.frames.length * 1024 * dec.config.chanConfig;
    }
    if (!parts.length) return;
    const q = new Int16Array(block * 1024), meta = new Uint16Array(block * host.META_WORDS), pcm = new Float32Array(pcmAt);
    let units = [];
    for (const p of parts) { p.dec.fillBatch(p, p.blockBase, q, meta); units = units.concat(p.units); }
    const tns = tnsList && tnsList.length ? host.packTns(tnsList) : null, cce = cceList && cceList.length ? host.packCce(cceList) : null;
    const t0 = process.hrtime.bigint();
    let failed = null;
    try { g.engine.decodeBatch(host.packUnits(units), q, meta, pcm, tns, cce); } catch (err) { failed = err; }
    this.stats.engineNs += process.hrtime.bigint() - t0;
    this.stats.batches++; this.stats.units += units.length;
    if (!failed) {
        for (const p of parts) { p.dec.deliver(p, pcm, p.pcmBase, null); this.stats.frames += p.frames.length; }
        return;
    }
    /* a device error: the launch may have advanced every stream's state — decoding the same frames again would advance it
     * twice and deliver wrong PCM without an error: the error goes to every stream of the batch instead */
    if (!refusedBeforeLaunch(failed)) {
        for (const p of parts) p.dec.deliver(p, pcm, p.pcmBase, failed);
        return;
    }
    /* the engine refused the batch as a whole before launching anything (nothing was decoded, no state advanced): decoder by
     * decoder, so that only the stream whose frames it refuses pays for it */
    this.stats.retries++;
    for (const p of parts) {
        let refused = null;
        try { g.engine.decodeBatch(host.packUnits(p.units), q, meta, pcm, tns, cce); }
        catch (err) { refused = err instanceof Error ? err : new Error(String(err)); }
        p.dec.deliver(p, pcm, p.pcmBase, refused);
        if (!refused) this.stats.frames += p.frames.length;
    }
};

module.exports = { SharedEngine: SharedEngine };
