/*
 * resident_drive.cpp — the bytes -> PCM route (aacg_pipeline_*) from a tight C loop: what one 4096-frame stereo batch costs
 * one at a time (aacg_pipeline_decode on one lane: round 5's 1.14 ms) and with batches in flight (aacg_pipeline_submit /
 * aacg_pipeline_collect on three lanes), f32 and int16 PCM, into page-locked memory.  VERDICT round 5 item 2: "first find where
 * the other 0.5 ms goes" — run it under `rocprofv3 --kernel-trace --memory-copy-trace --stats` for the per-stage durations.
 *
 *   tools/micro/resident_drive <file.aac> [--streams S] [--frames F] [--batches N] [--lanes L] [--i16] [--sync] [--pageable]
 *                                         [--device-plans] [--new-shapes [--seed N]] [--tns-spec] [--pns-spec] [--pulses]
 *                                         [--carry-shape] [--device-pcm [--planar]] [--mix 1|2] [--rate OUT] [--features]
 *                                         [--loudness [--true-peak]] [--limiter [--limit-tp]] [--conceal] [--drop-every N] [--trim SKIP[:KEEP]]
 *
 * --trim SKIP[:KEEP]: a trim as the last PCM stage (aacg_pipeline_set_trim: every slot's window skips SKIP samples of what the stage
 * receives and keeps KEEP, all of the rest if left out): one more launch per batch (aacg_pcm_trim_*) behind the resampler, none with
 * --features, whose records take the window instead.  The tool feeds every slot one endless stream, so the window's cuts fall into the
 * warm-up or behind the run and a timed batch keeps ALL it receives: the line's time is the stage's cost at its most, and it carries
 * the window and a device-to-device aacg_calib_copy of the bytes the trim kernel reads, timed in the same run.  Combines with
 * everything else.
 *
 * --conceal (with --device-plans): refused frames repeat their stream's last good frame, fading 2 scalefactor steps a frame for at most
 * 6 frames (aacg_pipeline_set_concealment): one more small launch per batch (aacg_units_conceal) between the refresh and the carry.
 * --drop-every N: every N-th frame of the batch (N, 2 N, ... in the packed order) has its table entry cut to 9 bytes, so that the parser
 * refuses it; the line then carries the frames dropped per batch, the refusals are expected and do not fail the run, and with --conceal
 * the frames the pipeline counted as concealed.  Combine them to see what a lossy feed costs; --conceal alone for what a clean one costs.
 *
 * --limiter: a gain per stream and a look-ahead limiter behind the mix and in front of the resampler (aacg_limiter_design at the file's
 * rate with a ceiling of -1 dB and a release of 200 ms; aacg_pipeline_set_limiter; slot s gets the gain 0.5 + 0.5 (s mod 8) through
 * aacg_pipeline_set_gain, so that some streams are boosted into the ceiling): one more launch per batch (aacg_pcm_limit_*).  The line
 * then carries the two settings and the bytes that launch reads and writes.  Combines with everything else.
 * --limit-tp (with --limiter): a true-peak detector in front of the limiter's recurrence (aacg_true_peak_design's four phases of 24 taps
 * with beta 5; aacg_pipeline_set_limiter_true_peak): two launches per batch (aacg_pcm_limit_tp_detect_*, aacg_pcm_limit_tp_*) in the
 * place of the limiter's one.  The line then carries the table's shape and the stage's delay (aacg_pipeline_limiter_delay).
 *
 * --true-peak (with --loudness): the oversampled peak of every hop of the meter beside its records (aacg_true_peak_design's four phases
 * of 24 taps with beta 5; aacg_pipeline_set_true_peak): one more launch per batch (aacg_pcm_truepeak_*) over the transform's PCM, and a
 * float per hop and channel comes down with the meter's records into a buffer named before every submission
 * (aacg_pipeline_true_peak_out).  The line then carries the table's shape.
 *
 * --loudness: a loudness meter beside whatever leaves (aacg_loudness_design at the file's rate, BS.1770's K-weighting, with a hop of a
 * tenth of a second; aacg_pipeline_set_loudness): one more launch per batch (aacg_pcm_loudness_*) over the transform's PCM, and two floats
 * per hop and channel come down with the results into a buffer named before every submission (aacg_pipeline_loudness_out).  The line then
 * carries the hop and the records a batch emits at most.  Combines with everything else.
 *
 * --features: Whisper's front end as the last stage of the way out (aacg_features_design at the rate that leaves: 400-sample frames every
 * 160, 201 bins, 80 Slaney bands, centred with pad_left 200, log10 with a floor of 1e-10; aacg_pipeline_set_features): one more launch
 * per batch (aacg_pcm_features_*), and float32 feature frames leave in the place of one channel of PCM — so it goes behind --mix 1 (or a
 * mono file), usually with --rate 16000.  Buffers are sized for the most a batch can emit (a stream of n samples completes at most
 * n / 160 + 1 frames); planar rows hold that many feature frames.  The line then carries the stage's parameters.
 *
 * --rate OUT: the PCM resampled to OUT Hz on the device (aacg_resample_design from the file's rate with 32 taps and the default roll-off
 * and window; aacg_pipeline_set_resample): one more launch per batch (aacg_pcm_resample_*), behind the mix if there is one, and
 * ceil-ish F x 1024 x OUT / rate samples per stream leave.  Buffers are sized for the most a batch can emit (a stream of F frames emits
 * at most ceil(1024 F L / M) samples whatever its clock); planar rows are that many samples rounded up to whole kilosamples.  The line
 * then carries the rate, L / M, and a device-to-device aacg_calib_copy of the bytes the resample kernel READS, timed in the same run.
 * Combines with everything else.
 *
 * --mix O: the standard downmix to O = 1 or 2 channels on the device (aacg_mix_standard with a surround gain of 1/sqrt 2, normalised;
 * aacg_pipeline_set_mix): one more launch per batch (aacg_pcm_mix_*), and O channels of PCM leave in the place of the stream's.  The
 * line then carries the channels that leave and a device-to-device aacg_calib_copy of the UNMIXED PCM's bytes — what the mix kernel
 * reads — timed in the same run: what its time in a kernel trace is read against.  Combines with everything else.
 *
 * --device-pcm: the PCM left on the device (aacg_pipeline_submit_device, AACG_PCM_PACKED: the transform writes the caller's buffer);
 * with --planar AACG_PCM_PLANAR, stride_frames = F (one more launch per batch, aacg_pcm_planar).  One device buffer per lane; nothing
 * of the PCM is read back inside the timed region (one buffer comes down after it, for output_ok).  Combines with --i16, --lanes,
 * --sync, --device-plans and --new-shapes.  The line then also carries what a device-to-device copy of the batch's PCM bytes takes
 * on this box in this run (aacg_calib_copy, 20 launches between two events): what aacg_pcm_planar's time in a kernel trace is read
 * against.
 *
 * --tns-spec / --pns-spec: aacg_pipeline_config.stages (the spec-correct TNS filters / noise bands; the TNS records are made on the
 * device, every launch is aacg_imdct_run_quant_ex_rv).  --pulses: AACG_PARSE_APPLY_PULSES (streams with pulse data).
 * --carry-shape: AACG_PIPELINE_STAGE_WINDOW_SHAPE (each channel's window shape carried on the device: one more small launch per
 * batch behind the refresh; goes with --i16 and with either plan mode).
 * --device-plans: aacg_pipeline_config.plan_mode 1 (one plan shaped on the device per batch instead of a kept plan per shape).
 * --new-shapes: every batch a NEW seeded shape — each stream brings 1..F frames (aacg_pipeline_submit_ragged) — which is what a
 * jittered feed gives the route; the line then also says how long the host spent inside the submit call alone, per batch.
 *
 * The batch: S streams x F frames taken from the ADTS file's frames in rotation (any sequence of frames decodes; the rate does
 * not depend on whether it is music).  The reference does this per stream and per frame in readChunk(), src/decoder.js:125-216.
 * Measurement aid: the product library through its public C ABI only.
 */
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/aacgpu.h"
#include "../../include/aacgpu_tools.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: resident_drive <file.aac> [--streams S] [--frames F] [--batches N] [--lanes L] [--i16] [--sync] [--pageable]\n"); return 2; }
    uint32_t S = 256, F = 16;
    int batches = 200, lanes = 3;
    bool i16 = false, sync = false, pageable = false, device_plans = false, new_shapes = false, tns_spec = false, pns_spec = false, pulses = false, carry_shape = false, device_pcm = false, planar = false;
    uint64_t seed = 1;
    uint32_t mix = 0, rate = 0;
    bool features = false, loudness = false, limiter = false, limit_tp = false, true_peak = false, conceal = false;
    uint32_t drop_every = 0;
    bool trim = false;
    uint64_t trim_skip = 0, trim_keep = AACG_TRIM_ALL;
    for (int i = 2; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&]() { if (i + 1 >= argc) std::exit(2); return argv[++i]; };
        if (a == "--streams") S = (uint32_t)std::atoi(val());
        else if (a == "--frames") F = (uint32_t)std::atoi(val());
        else if (a == "--batches") batches = std::atoi(val());
        else if (a == "--lanes") lanes = std::atoi(val());
        else if (a == "--i16") i16 = true;
        else if (a == "--sync") sync = true;
        else if (a == "--pageable") pageable = true;
        else if (a == "--device-plans") device_plans = true;
        else if (a == "--new-shapes") new_shapes = true;
        else if (a == "--tns-spec") tns_spec = true;
        else if (a == "--pns-spec") pns_spec = true;
        else if (a == "--pulses") pulses = true;
        else if (a == "--carry-shape") carry_shape = true;
        else if (a == "--device-pcm") device_pcm = true;
        else if (a == "--planar") planar = true;
        else if (a == "--mix") mix = (uint32_t)std::atoi(val());
        else if (a == "--rate") rate = (uint32_t)std::atoi(val());
        else if (a == "--features") features = true;
        else if (a == "--loudness") loudness = true;
        else if (a == "--true-peak") true_peak = true;
        else if (a == "--limiter") limiter = true;
        else if (a == "--limit-tp") limit_tp = true;
        else if (a == "--conceal") conceal = true;
        else if (a == "--drop-every") drop_every = (uint32_t)std::atoi(val());
        else if (a == "--trim") {
            const std::string v = val();
            const size_t colon = v.find(':');
            trim = true;
            trim_skip = std::strtoull(v.c_str(), nullptr, 10);
            if (colon != std::string::npos) trim_keep = std::strtoull(v.c_str() + colon + 1, nullptr, 10);
        }
        else if (a == "--seed") seed = (uint64_t)std::atoll(val());
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (planar && !device_pcm) { std::fprintf(stderr, "--planar goes with --device-pcm\n"); return 2; }
    std::vector<uint8_t> file;
    if (FILE* f = std::fopen(argv[1], "rb")) { uint8_t buf[65536]; size_t k; while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + k); std::fclose(f); }
    std::vector<aacg_parse_frame> src;
    for (size_t off = 0; off + 7 <= file.size();) {
        if (file[off] != 0xff || (file[off + 1] & 0xf0) != 0xf0) break;
        const uint32_t len = ((file[off + 3] & 3u) << 11) | ((uint32_t)file[off + 4] << 3) | (file[off + 5] >> 5);
        if (len < 7 || off + len > file.size()) break;
        src.push_back({(uint32_t)off, len});
        off += len;
    }
    if (src.empty()) { std::fprintf(stderr, "%s: no ADTS frames\n", argv[1]); return 2; }
    const uint32_t channels = ((file[2] & 1u) << 2) | (file[3] >> 6), sample_index = (file[2] >> 2) & 15u;
    /* the batch's bytes: frame (s, f) = source frame (s + f) mod n, packed one behind the other */
    std::vector<uint8_t> bytes;
    std::vector<aacg_parse_frame> frames((size_t)S * F);
    std::vector<uint32_t> slots(S);
    for (uint32_t s = 0; s < S; s++) {
        slots[s] = s;
        for (uint32_t f = 0; f < F; f++) {
            const aacg_parse_frame& g = src[(s + f) % src.size()];
            frames[(size_t)s * F + f] = {(uint32_t)bytes.size(), g.byte_length};
            bytes.insert(bytes.end(), file.begin() + g.byte_offset, file.begin() + g.byte_offset + g.byte_length);
        }
    }
    uint32_t dropped = 0;                                   /* --drop-every: the entries cut to an ADTS header and two bytes */
    if (drop_every) for (size_t i = drop_every; i < frames.size(); i += drop_every) if (frames[i].byte_length > 9u) { frames[i].byte_length = 9u; dropped++; }
    std::vector<aacg_code_entry> entries(AACG_STANDARD_CODEBOOK_ENTRIES);
    uint32_t counts[12];
    aacg_standard_codebooks(entries.data(), counts);
    aacg_pipeline_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = AACG_ABI_VERSION; cfg.sample_index = (int32_t)sample_index; cfg.max_streams = (int32_t)S; cfg.channels = (int32_t)channels; cfg.max_frames = (int32_t)F;
    cfg.output_kind = i16 ? AACG_OUTPUT_I16 : AACG_OUTPUT_F32; cfg.parse_options = AACG_PARSE_REFERENCE_QUIRKS | (pulses ? AACG_PARSE_APPLY_PULSES : 0); cfg.lanes = sync ? 1 : lanes;
    cfg.plan_mode = device_plans ? 1 : 0;
    cfg.stages = (tns_spec ? AACG_PIPELINE_STAGE_TNS : 0) | (pns_spec ? AACG_PIPELINE_STAGE_PNS : 0) | (carry_shape ? AACG_PIPELINE_STAGE_WINDOW_SHAPE : 0);
    aacg_pipeline* p = nullptr;
    int rc = aacg_pipeline_create(&cfg, entries.data(), counts, &p);
    if (rc) { std::fprintf(stderr, "aacg_pipeline_create: %d\n", rc); return 2; }
    if (mix) {
        float m[16];
        if ((rc = aacg_mix_standard(channels, mix, 0.70710678118654752440f, 1, m))) { std::fprintf(stderr, "aacg_mix_standard(%u, %u): %d\n", channels, mix, rc); return 2; }
        if ((rc = aacg_pipeline_set_mix(p, mix, m))) { std::fprintf(stderr, "aacg_pipeline_set_mix: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    const aacg_conceal_config conceal_cfg = {2u, 6u};
    if (conceal && (rc = aacg_pipeline_set_concealment(p, &conceal_cfg))) { std::fprintf(stderr, "aacg_pipeline_set_concealment: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    const uint32_t out_channels = (uint32_t)aacg_pipeline_out_channels(p);      /* what leaves: the mix's rows, or the stream's channels */
    aacg_limiter_config lim_cfg = {0.0f, 0.0f};
    if (limiter) {                                          /* behind the mix, in front of the resampler */
        static const uint32_t rates[16] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350, 0, 0, 0};
        if ((rc = aacg_limiter_design(rates[sample_index], -1.0, 200.0, &lim_cfg))) { std::fprintf(stderr, "aacg_limiter_design(%u): %d\n", rates[sample_index], rc); return 2; }
        if ((rc = aacg_pipeline_set_limiter(p, &lim_cfg))) { std::fprintf(stderr, "aacg_pipeline_set_limiter: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
        for (uint32_t s = 0; s < S; s++)
            if ((rc = aacg_pipeline_set_gain(p, s, 0.5f + 0.5f * (float)(s % 8u)))) { std::fprintf(stderr, "aacg_pipeline_set_gain: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    uint32_t lim_delay = 0;
    if (limit_tp) {                                         /* the detector in front of the limiter's recurrence; in front of the trim, like the limiter */
        if (!limiter) { std::fprintf(stderr, "--limit-tp goes with --limiter\n"); return 2; }
        std::vector<float> table(4u * 24u);
        if ((rc = aacg_true_peak_design(4, 24, 0.95, 5.0, table.data(), table.size()))) { std::fprintf(stderr, "aacg_true_peak_design: %d\n", rc); return 2; }
        const aacg_true_peak_config tc = {4, 24, table.data()};
        if ((rc = aacg_pipeline_set_limiter_true_peak(p, &tc))) { std::fprintf(stderr, "aacg_pipeline_set_limiter_true_peak: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    if (limiter && (rc = aacg_pipeline_limiter_delay(p, &lim_delay))) { std::fprintf(stderr, "aacg_pipeline_limiter_delay: %d\n", rc); return 2; }
    uint32_t rs_L = 1, rs_M = 1;
    if (rate) {
        static const uint32_t rates[16] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350, 0, 0, 0};
        std::vector<float> table(16384);
        if (!rates[sample_index] || (rc = aacg_resample_design(rates[sample_index], rate, 32, 0.0, 0.0, &rs_L, &rs_M, table.data(), table.size()))) { std::fprintf(stderr, "aacg_resample_design(%u -> %u): %d\n", rates[sample_index], rate, rc); return 2; }
        if ((rc = aacg_pipeline_set_resample(p, rs_L, rs_M, 32, table.data()))) { std::fprintf(stderr, "aacg_pipeline_set_resample: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    if (trim) {                                             /* behind the resampler, in front of the feature stage */
        const aacg_trim_config tc = {trim_skip, trim_keep};
        if ((rc = aacg_pipeline_set_trim(p, &tc))) { std::fprintf(stderr, "aacg_pipeline_set_trim: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    const uint32_t ft_K = 400, ft_H = 160, ft_bins = 201, ft_mels = 80;
    if (features) {
        static const uint32_t rates[16] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350, 0, 0, 0};
        std::vector<float> basis((size_t)2 * ft_bins * ft_K), fb((size_t)ft_mels * ft_bins);
        const uint32_t rate_out = rate ? rate : rates[sample_index];
        if ((rc = aacg_features_design(rate_out, ft_K, ft_H, ft_bins, ft_mels, 0.0, 0.0, basis.data(), basis.size(), fb.data(), fb.size()))) { std::fprintf(stderr, "aacg_features_design(%u): %d\n", rate_out, rc); return 2; }
        const aacg_features_config fc = {ft_K, ft_H, ft_K / 2, 2 * ft_bins, ft_mels, 1u, 1e-10f, basis.data(), fb.data()};
        if ((rc = aacg_pipeline_set_features(p, &fc))) { std::fprintf(stderr, "aacg_pipeline_set_features: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    uint32_t ld_hop = 0;
    if (loudness) {
        static const uint32_t rates[16] = {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350, 0, 0, 0};
        aacg_loudness_config lc;
        lc.hop = ld_hop = rates[sample_index] / 10u;
        if (!ld_hop || (rc = aacg_loudness_design(rates[sample_index], lc.coeffs))) { std::fprintf(stderr, "aacg_loudness_design(%u): %d\n", rates[sample_index], rc); return 2; }
        if ((rc = aacg_pipeline_set_loudness(p, &lc))) { std::fprintf(stderr, "aacg_pipeline_set_loudness: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    /* the most samples a stream of F frames emits, and the planar row that holds them; without --rate: F x 1024 and F.  --features: the most
     * feature frames those samples complete, which is the planar row too, and ft_mels floats each whatever the PCM's element */
    const size_t most = ((size_t)F * 1024 * rs_L + rs_M - 1) / rs_M, most_ft = most / ft_H + 1;
    const uint32_t stride_frames = features ? (uint32_t)most_ft : (uint32_t)((most + 1023) / 1024);
    const size_t pcm_bytes = features ? (size_t)S * most_ft * ft_mels * 4 : (size_t)S * (planar ? (size_t)stride_frames * 1024 : most) * out_channels * (i16 ? 2 : 4);
    const size_t unmixed_bytes = (size_t)S * F * 1024 * channels * (i16 ? 2 : 4);
    const size_t resample_in_bytes = (size_t)S * F * 1024 * out_channels * (i16 ? 2 : 4);
    const int n_out = 4;
    void* out[n_out];
    const uint32_t tp_L = 4, tp_T = 24;
    if (true_peak) {
        if (!loudness) { std::fprintf(stderr, "--true-peak requires --loudness\n"); return 2; }
        std::vector<float> table((size_t)tp_L * tp_T);
        if ((rc = aacg_true_peak_design(tp_L, tp_T, 0.95, 5.0, table.data(), table.size()))) { std::fprintf(stderr, "aacg_true_peak_design: %d\n", rc); return 2; }
        const aacg_true_peak_config tc = {tp_L, tp_T, table.data()};
        if ((rc = aacg_pipeline_set_true_peak(p, &tc))) { std::fprintf(stderr, "aacg_pipeline_set_true_peak: %d %s\n", rc, aacg_pipeline_last_error(p)); return 2; }
    }
    /* --loudness: the most records a batch emits (a stream of F frames completes at most F x 1024 / hop + 1 hops), per PCM buffer */
    const size_t ld_most = loudness ? (size_t)S * ((size_t)F * 1024 / ld_hop + 1) : 0, ld_floats = ld_most * channels * 2;
    std::vector<std::vector<float>> ld_rec((size_t)n_out, std::vector<float>(ld_floats));
    const size_t tp_floats = true_peak ? ld_most * channels : 0;      /* --true-peak: a float where the meter has two */
    std::vector<std::vector<float>> tp_rec((size_t)n_out, std::vector<float>(tp_floats));
    for (auto& o : out) { o = pageable ? std::malloc(pcm_bytes) : aacg_host_alloc(pcm_bytes); if (!o) { std::fprintf(stderr, "allocation failed\n"); return 2; } std::memset(o, 0, pcm_bytes); }
    /* --device-pcm: a device buffer per lane (a batch in flight keeps its own until it is collected); planar rows of F frames */
    const int n_dev = device_pcm ? (sync ? 1 : lanes) : 0;
    std::vector<void*> dev((size_t)n_dev, nullptr);
    for (auto& d : dev) if (hipMalloc(&d, pcm_bytes) != hipSuccess || hipMemset(d, 0, pcm_bytes) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 2; }
    if (n_dev && hipDeviceSynchronize() != hipSuccess) { std::fprintf(stderr, "hipDeviceSynchronize failed\n"); return 2; }
    std::vector<aacg_parse_result> results((size_t)S * F * n_out);
    uint32_t refused[n_out] = {};
    auto fail = [&](const char* what, int code) { std::fprintf(stderr, "%s: %d %s\n", what, code, aacg_pipeline_last_error(p)); std::exit(2); };
    /* --new-shapes: the batch's counts (1..F per stream, a new draw per batch) and its frame table, packed stream after stream */
    std::vector<uint32_t> counts_of(S), rect_counts;
    std::vector<aacg_parse_frame> ragged((size_t)S * F);
    uint64_t lcg = seed * 0x9E3779B97F4A7C15ull + 1;
    double submit_s = 0;
    uint64_t fed = 0;                                       /* frames submitted */
    auto run = [&](int n) {
        std::vector<uint64_t> t((size_t)n);
        const int depth = sync ? 0 : lanes - 1;                 /* batches submitted ahead of the one being collected */
        for (int b = 0; b < n + depth; b++) {
            if (b < n) {
                const int k = b % n_out;
                if (loudness && (rc = aacg_pipeline_loudness_out(p, ld_rec[(size_t)k].data(), ld_floats, nullptr))) fail("aacg_pipeline_loudness_out", rc);
                if (true_peak && (rc = aacg_pipeline_true_peak_out(p, tp_rec[(size_t)k].data(), tp_floats))) fail("aacg_pipeline_true_peak_out", rc);
                aacg_pcm_device_out where;
                if (device_pcm) { where.d_pcm = dev[(size_t)(b % n_dev)]; where.d_pcm_bytes = pcm_bytes; where.layout = planar ? AACG_PCM_PLANAR : AACG_PCM_PACKED; where.stride_frames = planar ? stride_frames : 0u; }
                if (new_shapes) {
                    size_t at = 0;
                    for (uint32_t s = 0; s < S; s++) {
                        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                        counts_of[s] = 1u + (uint32_t)((lcg >> 33) % F);
                        std::memcpy(&ragged[at], &frames[(size_t)s * F], counts_of[s] * sizeof(aacg_parse_frame));
                        at += counts_of[s];
                    }
                    const double t0 = now_s();
                    if (device_pcm) {
                        if ((rc = aacg_pipeline_submit_device(p, bytes.data(), bytes.size(), ragged.data(), slots.data(), S, counts_of.data(), &where, &results[(size_t)k * S * F], &refused[k], &t[(size_t)b]))) fail("aacg_pipeline_submit_device", rc);
                        if (sync && (rc = aacg_pipeline_collect(p, t[(size_t)b]))) fail("aacg_pipeline_collect", rc);
                    }
                    else if (sync) { if ((rc = aacg_pipeline_decode_ragged(p, bytes.data(), bytes.size(), ragged.data(), slots.data(), S, counts_of.data(), out[k], &results[(size_t)k * S * F], &refused[k]))) fail("aacg_pipeline_decode_ragged", rc); }
                    else if ((rc = aacg_pipeline_submit_ragged(p, bytes.data(), bytes.size(), ragged.data(), slots.data(), S, counts_of.data(), out[k], &results[(size_t)k * S * F], &refused[k], &t[(size_t)b]))) fail("aacg_pipeline_submit_ragged", rc);
                    submit_s += now_s() - t0;
                    fed += at;
                }
                else if (device_pcm) {
                    rect_counts.assign(S, F);
                    if ((rc = aacg_pipeline_submit_device(p, bytes.data(), bytes.size(), frames.data(), slots.data(), S, rect_counts.data(), &where, &results[(size_t)k * S * F], &refused[k], &t[(size_t)b]))) fail("aacg_pipeline_submit_device", rc);
                    if (sync && (rc = aacg_pipeline_collect(p, t[(size_t)b]))) fail("aacg_pipeline_collect", rc);
                }
                else if (sync) { if ((rc = aacg_pipeline_decode(p, bytes.data(), bytes.size(), frames.data(), slots.data(), S, F, out[k], &results[(size_t)k * S * F], &refused[k]))) fail("aacg_pipeline_decode", rc); }
                else if ((rc = aacg_pipeline_submit(p, bytes.data(), bytes.size(), frames.data(), slots.data(), S, F, out[k], &results[(size_t)k * S * F], &refused[k], &t[(size_t)b]))) fail("aacg_pipeline_submit", rc);
            }
            if (!sync && b >= depth && (rc = aacg_pipeline_collect(p, t[(size_t)(b - depth)]))) fail("aacg_pipeline_collect", rc);
        }
    };
    run(10);                                                /* warm: plans, staging, page-locked memory */
    std::vector<double> ms;
    submit_s = 0; fed = 0;
    for (int r = 0; r < 5; r++) { const double t0 = now_s(); run(batches); ms.push_back((now_s() - t0) * 1e3 / batches); }
    const double submit_ms = submit_s * 1e3 / (5.0 * batches);
    uint64_t shaped = 0, chained = 0, launches = 0;
    (void)aacg_pipeline_launch_counts(p, &shaped, &chained, &launches);
    std::sort(ms.begin(), ms.end());
    /* --device-pcm: what a device-to-device copy of a batch's PCM bytes takes here and now, and — outside the timed region — the last
     * warm buffer down for the output check (planar rows are as long as the packed frames of a stream when every stream brings F) */
    double copy_us = 0, unmixed_copy_us = 0;
    /* a device-to-device aacg_calib_copy of `bytes` between two spare buffers (or from `from`), 20 launches between two events */
    auto calib = [&](size_t bytes, const void* from) -> double {
        void *spare = nullptr, *src = nullptr;
        hipEvent_t e0, e1;
        float span = 0;
        if (hipMalloc(&spare, bytes) != hipSuccess || (!from && (hipMalloc(&src, bytes) != hipSuccess || hipMemset(src, 0, bytes) != hipSuccess)) ||
            hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); std::exit(2); }
        if (!from) from = src;
        (void)aacg_calib_copy(spare, from, bytes, nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int i = 0; i < 20; i++) (void)aacg_calib_copy(spare, from, bytes, nullptr);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&span, e0, e1) != hipSuccess) { std::fprintf(stderr, "the calibration copy failed\n"); std::exit(2); }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(spare); if (src) (void)hipFree(src);
        return span * 1e3 / 20.0;
    };
    if (device_pcm) {
        copy_us = calib(pcm_bytes, dev[0]);
        if (hipMemcpy(out[0], dev[0], pcm_bytes, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 2; }
    }
    if (mix) unmixed_copy_us = calib(unmixed_bytes, nullptr);
    const double resample_in_copy_us = rate ? calib(resample_in_bytes, nullptr) : 0.0;
    const size_t trim_in_bytes = (size_t)S * most * out_channels * (i16 ? 2 : 4);      /* what the trim kernel reads at most: what the stage before it emits */
    const double trim_in_copy_us = trim && !features ? calib(trim_in_bytes, nullptr) : 0.0;
    bool finite = true, nonzero = false;
    uint32_t bad = 0;
    for (int k = 0; k < n_out; k++) bad += refused[k];
    if (!i16 || features) { const float* w = (const float*)out[0]; for (size_t i = 0; i < pcm_bytes / 4; i += 97) { finite = finite && std::isfinite(w[i]); nonzero = nonzero || w[i] != 0.0f; } }
    else { const int16_t* w = (const int16_t*)out[0]; for (size_t i = 0; i < pcm_bytes / 2; i += 97) nonzero = nonzero || w[i] != 0; }
    char copy_key[64] = "";                                 /* only where it was measured: the host-PCM modes' lines are as they were */
    if (device_pcm) std::snprintf(copy_key, sizeof copy_key, "\"d2d_copy_of_pcm_us\": %.2f, ", copy_us);
    char mix_key[128] = "";                                 /* --mix only */
    if (mix) std::snprintf(mix_key, sizeof mix_key, "\"mix_out_channels\": %u, \"unmixed_pcm_bytes_per_batch\": %zu, \"d2d_copy_of_unmixed_pcm_us\": %.2f, ", out_channels, unmixed_bytes, unmixed_copy_us);
    char rate_key[192] = "";                                /* --rate only */
    if (rate) std::snprintf(rate_key, sizeof rate_key, "\"rate_out\": %u, \"resample_L\": %u, \"resample_M\": %u, \"resample_taps\": 32, \"resample_in_bytes_per_batch\": %zu, \"d2d_copy_of_resample_in_us\": %.2f, ", rate, rs_L, rs_M, resample_in_bytes, resample_in_copy_us);
    char loudness_key[288] = "";                            /* --loudness only, and behind it --true-peak's */
    if (loudness) {
        for (float v : ld_rec[0]) finite = finite && std::isfinite(v);
        int at = std::snprintf(loudness_key, sizeof loudness_key, "\"loudness\": \"bs1770\", \"loudness_hop\": %u, \"loudness_records_per_batch_most\": %zu, ", ld_hop, ld_most);
        if (true_peak) {
            float largest = 0.0f;
            for (float v : tp_rec[0]) { finite = finite && std::isfinite(v); largest = v > largest ? v : largest; }
            std::snprintf(loudness_key + at, sizeof loudness_key - (size_t)at, "\"true_peak\": \"kaiser\", \"true_peak_phases\": %u, \"true_peak_taps\": %u, \"true_peak_largest\": %.6g, ", tp_L, tp_T, largest);
        }
    }
    char limiter_key[320] = "";                             /* --limiter only: what aacg_pcm_limit_* reads and writes is 2 n Oc 1024 E */
    if (limiter) std::snprintf(limiter_key, sizeof limiter_key, "\"limiter\": \"-1 dB, 200 ms\", \"limiter_ceiling\": %.6f, \"limiter_release\": %.6g, \"limiter_bytes_moved_per_batch\": %zu, ",
                               (double)lim_cfg.ceiling, (double)lim_cfg.release, 2 * resample_in_bytes);
    if (limit_tp) std::snprintf(limiter_key + std::strlen(limiter_key), sizeof limiter_key - std::strlen(limiter_key), "\"limiter_true_peak\": \"kaiser\", \"limiter_true_peak_phases\": 4, \"limiter_true_peak_taps\": 24, \"limiter_delay\": %u, ", lim_delay);
    char features_key[192] = "";                            /* --features only */
    if (features) std::snprintf(features_key, sizeof features_key, "\"features\": \"log-mel\", \"frame_length\": %u, \"hop\": %u, \"n_bins\": %u, \"n_mels\": %u, \"feature_frames_per_stream_most\": %zu, ", ft_K, ft_H, ft_bins, ft_mels, most_ft);
    char conceal_key[192] = "";                             /* --conceal / --drop-every only */
    if (conceal || drop_every) {
        uint64_t concealed = 0;
        (void)aacg_pipeline_concealed(p, &concealed);
        std::snprintf(conceal_key, sizeof conceal_key, "\"conceal\": %s, \"conceal_fade_steps\": %u, \"conceal_hold_frames\": %u, \"drop_every\": %u, \"frames_dropped_per_batch\": %u, \"frames_concealed\": %llu, ",
                      conceal ? "true" : "false", conceal_cfg.fade_steps, conceal_cfg.hold_frames, drop_every, dropped, (unsigned long long)concealed);
    }
    char trim_key[192] = "";                                /* --trim only */
    if (trim) std::snprintf(trim_key, sizeof trim_key, "\"trim_skip\": %llu, \"trim_keep\": %s, \"trim_in_bytes_per_batch\": %zu, \"d2d_copy_of_trim_in_us\": %.2f, ", (unsigned long long)trim_skip,
                            trim_keep == AACG_TRIM_ALL ? "\"all\"" : std::to_string(trim_keep).c_str(), trim_in_bytes, trim_in_copy_us);
    if (drop_every) bad = 0;                                /* (the refusals are the dropped frames': expected) */
    std::printf("{\"tool\": \"resident_drive\", \"mode\": \"%s\", \"lanes\": %d, \"streams\": %u, \"frames_per_stream\": %u, \"channels\": %u, \"pcm\": \"%s\", \"pcm_memory\": \"%s\", %s%s%s%s%s%s%s%s"
                "\"bytes_per_batch\": %zu, \"pcm_bytes_per_batch\": %zu, \"ms_per_batch_median\": %.4f, \"ms_per_batch_min\": %.4f, \"ms_per_batch_max\": %.4f, \"frames_per_s\": %.4g, "
                "\"pcm_GBs\": %.2f, \"plan_mode\": %d, \"stages\": %d, \"shapes\": \"%s\", \"submit_host_ms_per_batch\": %.4f, \"plan_builds\": %llu, \"batches_shaped_on_device\": %llu, "
                "\"launches\": %llu, \"launches_continued\": %llu, \"refused\": %u, \"output_ok\": %s}\n",
                device_pcm ? (sync ? "aacg_pipeline_submit_device + collect, one batch at a time" : "aacg_pipeline_submit_device / collect, batches in flight")
                           : sync ? "aacg_pipeline_decode, one batch at a time" : "aacg_pipeline_submit / collect, batches in flight", sync ? 1 : lanes, S, F, channels, i16 ? "int16" : "f32",
                device_pcm ? (planar ? "device, planar" : "device, packed") : pageable ? "pageable" : "page-locked", copy_key, mix_key, limiter_key, rate_key, features_key, loudness_key, conceal_key, trim_key, bytes.size(), pcm_bytes, ms[ms.size() / 2], ms.front(), ms.back(), (new_shapes ? (double)fed / (5.0 * batches) : (double)S * F) / (ms[ms.size() / 2] * 1e-3),
                (double)pcm_bytes / (ms[ms.size() / 2] * 1e-3) / 1e9, device_plans ? 1 : 0, (int)cfg.stages, new_shapes ? "a new seeded shape per batch, 1..F frames per stream" : "one",
                new_shapes ? submit_ms : 0.0, (unsigned long long)aacg_pipeline_plan_builds(p), (unsigned long long)shaped, (unsigned long long)launches, (unsigned long long)chained, bad, (finite && nonzero && !bad) ? "true" : "false");
    aacg_pipeline_destroy(p);
    for (void* d : dev) (void)hipFree(d);
    return (finite && nonzero && !bad) ? 0 : 1;
}
