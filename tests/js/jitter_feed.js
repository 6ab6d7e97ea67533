/*
 * tests/js/jitter_feed.js — jittered arrival on a resident SharedEngine: N decoders, each fed a seeded random 1..16 frames' worth
 * of ADTS bytes per round, about one reader in ten paused for a few rounds, and now and then a stream that ends and starts over on
 * a new decoder (detach, attach: the slot's state is reset).  What a server with many live players sees, unlike a benchmark that
 * feeds every stream whole.  Used by tests/js/test_ragged_shared.js (gpu) and tools/readchunk_rate.js --arrival jitter.
 *
 * Every random draw depends on the seed only, never on what was decoded, so two runs with the same seed feed the same bytes at
 * the same rounds whatever the engine's options: a stream's frames, in order, are the same, and so is its PCM.
 */
'use strict';

function rng32(seed) {                                     // mulberry32
    let a = seed >>> 0;
    return function () {
        a = (a + 0x6D2B79F5) >>> 0;
        let t = a;
        t = Math.imul(t ^ (t >>> 15), t | 1);
        t ^= t + Math.imul(t ^ (t >>> 7), t | 61);
        return ((t ^ (t >>> 14)) >>> 0) / 4294967296;
    };
}

/* opts: host (aac.js_amd/js), shared (a resident SharedEngine), sources ([{ bytes, list: host.adts.frames(bytes) }]), streams,
 * rounds, seed, onFrame(stream, source, frameIndex, pcm) (optional), pauses (default true; false: no reader pauses — the draws are
 * made all the same, so the bytes fed are the same).  Stream i decodes sources[i % sources.length].
 * -> { frames, seconds, instances, sums: per-stream sum of pcm[17] over its frames in order } */
function run(opts) {
    const host = opts.host, shared = opts.shared, sources = opts.sources, S = opts.streams, rnd = rng32(opts.seed | 0);
    const onFrame = opts.onFrame || null, pauses = opts.pauses !== false;
    const streams = [];
    let instances = 0, frames = 0;
    const open = function (i) {
        const src = sources[i % sources.length];
        const dec = new host.GpuAACDecoder({ frontend: null, lookahead: shared.lookahead, shared: shared });
        dec.init();
        dec.setCookie(host.adts.cookie(src.list[0].header));
        instances++;
        return { dec: dec, src: i % sources.length, fed: 0, read: 0, paused: 0 };
    };
    for (let i = 0; i < S; i++) streams.push({ cur: open(i), sum: 0 });
    const take = function (i, x) {
        const pcm = x.dec.readChunk();
        if (!pcm) return false;
        if (onFrame) onFrame(i, x.src, x.read, pcm);
        streams[i].sum += pcm[17];
        x.read++; frames++;
        return true;
    };
    /* a stream's decoder read to its last fed frame (a flush may leave frames in flight: readChunk() then flushes again) */
    const drain = function (i, x) {
        for (let guard = 0; x.read < x.fed; guard++) {
            if (!take(i, x) && guard > 64 * (x.fed - x.read + 1)) throw new Error('jitter: stream ' + i + ' stalls at frame ' + x.read + ' of ' + x.fed);
        }
    };
    const t0 = process.hrtime.bigint();
    for (let r = 0; r < opts.rounds; r++) {
        for (let i = 0; i < S; i++) {
            const st = streams[i];
            let x = st.cur;
            const restart = rnd() < 0.01, k = 1 + Math.floor(rnd() * 16), pause = rnd();
            if (restart && x.fed) {                         // the stream ends here; a new one starts on a new decoder (a new slot state)
                drain(i, x);
                x.dec.close();
                x = st.cur = open(i);
            }
            const list = sources[x.src].list, n = Math.min(k, list.length - x.fed);
            if (n > 0) {
                const a = list[x.fed], b = list[x.fed + n - 1];
                x.dec.feed(sources[x.src].bytes.subarray(a.offset, b.offset + b.length));
                x.fed += n;
            }
            if (x.paused) x.paused--;
            else if (pauses && pause < 0.03) x.paused = 2 + Math.floor(pause * 100);     // about one reader in ten paused, for 2..4 rounds
        }
        for (let i = 0; i < S; i++) {
            const x = streams[i].cur;
            if (x.paused) continue;
            while (take(i, x)) { /* what it has */ }
        }
    }
    for (let i = 0; i < S; i++) drain(i, streams[i].cur);
    const seconds = Number(process.hrtime.bigint() - t0) / 1e9;
    return { frames: frames, seconds: seconds, instances: instances, sums: streams.map(function (s) { return s.sum; }) };
}

module.exports = { run: run, rng32: rng32 };
