/*
 * aacgpu.h — C ABI of the MI355X-native AAC-LC synthesis engine.
 *
 * This library replaces ONE seam of audiocogs/aac.js: everything that
 * `AACDecoder.prototype.process(elements)` does plus the channel interleave that
 * follows it in `readChunk` (reference src/decoder.js:201-215, 218-404), i.e.
 *
 *     inverse quantisation      src/ics.js:222-227,244-256  (+ tables src/tables.js:168-191)
 *     mid/side stereo           src/decoder.js:379-404
 *     intensity stereo          src/decoder.js:337-376
 *     TNS                       src/tns.js:105-177   (identity as the reference runs, see AACG_TNS_REFERENCE)
 *     IMDCT + window + OLA      src/filter_bank.js:88-204, src/mdct.js:62-115, src/fft.js:105-192
 *     interleave, /32768        src/decoder.js:203-215
 *
 * The serial part (ADTS demux, raw_data_block parse, Huffman) stays in the JavaScript
 * host, exactly where the reference has it; the host hands batches of parsed
 * elements ("units") across this ABI.  Plain C: pointers and sizes only, int status
 * (0 = OK, <0 = error), no exceptions, no torch/HIP types in any signature.
 *
 * Vocabulary (follows the reference's data model):
 *   channel-frame  one channel x one 1024-sample frame
 *   unit           one syntactic element of one frame: SCE/LFE (1 channel,
 *                  reference `processSingle`, decoder.js:250) or CPE (2 channels,
 *                  `processPair`, decoder.js:285)
 *   stream         one decoder instance's worth of state: the reference keeps
 *                  `FilterBank.overlaps[ch]` (filter_bank.js:38-41) per decoder; the
 *                  engine keeps it per (stream slot, channel) in HBM — in sixteen rotating buffers
 *                  (a launch reads one and writes the next, so that consecutive launches can overlap:
 *                  aacg_decode_pipelined), plus as much again for the hand-over between launches:
 *                  128 KB per (stream slot, channel) in all.
 */
#ifndef AACGPU_H
#define AACGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AACG_ABI_VERSION 6

#define AACG_FRAME_LEN      1024   /* decoder.js:86 frameLength                       */
#define AACG_MAX_SECTIONS   120    /* ics.js:49 MAX_SECTIONS (bandTypes/scaleFactors) */
#define AACG_MAX_CHANNELS   8
#define AACG_RUN_FRAMES     16     /* frames per workgroup run        */

/* ---- status codes ------------------------------------------------------------ */
enum {
    AACG_OK                 = 0,
    AACG_ERR_INVALID_ARG    = -1,
    AACG_ERR_NO_DEVICE      = -2,   /* no HIP device / HIP call failed                 */
    AACG_ERR_OUT_OF_MEMORY  = -3,
    AACG_ERR_CAPACITY       = -4,   /* batch larger than the engine was created for    */
    AACG_ERR_UNSUPPORTED    = -5,   /* reference throws here too (pulse, gain, PNS...) */
    AACG_ERR_LAYOUT_CHANGE  = -6,   /* element layout of a stream changes inside one batch */
    AACG_ERR_STALE_PLAN     = -7,   /* plan does not match the engine's overlap parity */
    AACG_ERR_TIMEOUT        = -8    /* a host wait for the GPU passed the engine's wait limit (aacg_set_wait_limit_ms): the call
                                       returns instead of hanging, aacg_last_error says what was in flight (launch counts, every
                                       stream's and completion event's state, the rendezvous cells' state words).  The work may
                                       still complete later; the engine's state is then undefined — destroy it (aacg_destroy does
                                       not wait again and leaves the engine's device memory allocated)                        */
};

/* ---- window sequences, ics.js:44-47 ------------------------------------------- */
enum {
    AACG_ONLY_LONG_SEQUENCE   = 0,
    AACG_LONG_START_SEQUENCE  = 1,
    AACG_EIGHT_SHORT_SEQUENCE = 2,
    AACG_LONG_STOP_SEQUENCE   = 3
};

/* ---- band types, ics.js:37-42 -------------------------------------------------- */
enum {
    AACG_ZERO_BT       = 0,
    AACG_FIRST_PAIR_BT = 5,
    AACG_ESC_BT        = 11,
    AACG_NOISE_BT      = 13,
    AACG_INTENSITY_BT2 = 14,
    AACG_INTENSITY_BT  = 15
};

/* ---- what the host hands over for the spectrum ------------------------------------ */
enum {
    AACG_INPUT_SPEC_F32  = 0,  /* the spectrum exactly as FilterBank.process receives it
                                  (filter_bank.js:88 `input`): f32[1024] per channel, dequantised,
                                  MS/IS already applied by the host — the filterbank seam       */
    AACG_INPUT_QUANT_I16 = 1   /* the integers Huffman.decodeSpectralData produced
                                  (huffman.js:1462-1490), int16[1024] per channel, same index
                                  order as ICStream.data, + aacg_band_meta per channel — the
                                  process(elements) seam: dequant, MS and IS run on the device   */
};

/* ---- TNS behaviour ------------------------------------------------------------- */
enum {
    AACG_TNS_REFERENCE = 0,    /* what aac.js executes: TNS.process leaves the data untouched
                                  (tns.js:106,122 NaN loop bounds); TNS side
                                  info, if any, is ignored                                       */
    AACG_TNS_SPEC      = 1     /* what tns.js:105-177 was meant to do (and a standard decoder does):
                                  the all-pole filter of its `decode` branch (tns.js:155-163) over the
                                  band range of every filter, per window.  Not aac.js behaviour: an
                                  explicit, separately tested mode                                 */
};

/* ---- PNS behaviour ------------------------------------------------------------- */
enum {
    AACG_PNS_REFERENCE = 0,    /* NOISE_BT bands are refused (AACG_ERR_UNSUPPORTED): aac.js's generator
                                  degenerates to NaN output after 11 draws (ics.js:234,239, SURVEY.md
                                  §8a row 4), there is no reference behaviour to reproduce            */
    AACG_PNS_SPEC      = 1     /* what ics.js:228-243 was meant to do: the generator
                                  state * 1664525 + 1013904223, restarted for every channel of every
                                  frame as the reference's fresh ICStream does, values normalised to the
                                  band's energy scalefactor per window.  Not aac.js behaviour: an explicit,
                                  separately tested mode (QUANT_I16 engines; units flag AACG_UNIT_HAS_PNS) */
};

enum {                          /* aacg_config.cce_mode (ABI version 4)                              */
    AACG_CCE_REFERENCE = 0,     /* coupling channel elements are not part of a batch: aac.js parses them and
                                   never applies them (`1 === true` at decoder.js:418, coupling point 3 at
                                   cce.js:69-70, undefined `swb` at cce.js:149 — SURVEY.md §8a row 9), so the
                                   host drops them; a unit with AACG_UNIT_CCE is refused                   */
    AACG_CCE_SPEC      = 1      /* what cce.js:121-158 + decoder.js:406-433 were written to do: a CCE's own
                                   spectrum, scaled by per-band gains, added to the channels it names —
                                   before or after their TNS (dependent coupling, spectral domain) or, after
                                   its own IMDCT with its own overlap state, to their PCM (independent
                                   coupling).  Not aac.js behaviour: an explicit, separately tested mode
                                   (float32 output engines)                                                */
};

/* ---- coupling side info (AACG_CCE_SPEC), the fields of the reference's CCEElement (cce.js:25-31) after
 * the host has resolved which output channels an element pair / id / select triple means ---- */
#define AACG_CCE_BEFORE_TNS   0      /* CCEElement.BEFORE_TNS  (cce.js:33) */
#define AACG_CCE_AFTER_TNS    1      /* CCEElement.AFTER_TNS   (cce.js:34) */
#define AACG_CCE_AFTER_IMDCT  2      /* CCEElement.AFTER_IMDCT (cce.js:35) */
#define AACG_CCE_MAX_TARGETS  16
typedef struct aacg_cce_target {
    uint8_t channel;           /* output channel of the stream that receives the coupled signal   */
    uint8_t gain_list;         /* which of gain[] applies to it (cce.gain[index], cce.js:77-107)   */
} aacg_cce_target;
typedef struct aacg_cce_info {
    uint8_t coupling_point;    /* AACG_CCE_*                                                       */
    uint8_t n_targets;         /* <= AACG_CCE_MAX_TARGETS                                          */
    uint8_t reserved[2];
    aacg_cce_target target[AACG_CCE_MAX_TARGETS];
    float   gain[AACG_CCE_MAX_TARGETS][AACG_MAX_SECTIONS];   /* dependent: per band, index g * max_sfb + sfb
                                  of the CCE's own ICS; independent: [list][0] for the whole frame      */
} aacg_cce_info;

/* ---- TNS side info (AACG_TNS_SPEC), the fields of the reference's TNS object (tns.js:22-44) ---- */
#define AACG_TNS_MAX_ORDER 12  /* AAC-LC limit; tns.js:84 accepts up to 20, orders 13..20 are refused */
typedef struct aacg_tns_filter {
    uint8_t length;            /* tns.length[w][filt], in scalefactor bands                    */
    uint8_t order;             /* tns.order[w][filt]; 0 = filter absent                        */
    uint8_t direction;         /* tns.direction[w][filt]: 1 = downwards                        */
    uint8_t reserved;
    float   coef[AACG_TNS_MAX_ORDER];   /* tns.coef[w][filt][i] as looked up from TNS_TABLES (tns.js:89-97) */
} aacg_tns_filter;
/* One per channel that has AACG_CHAN_TNS_PRESENT.  Long windows: n_filt[0] <= 3 filters in filt[0..2];
 * EIGHT_SHORT: window w has n_filt[w] <= 1 filter in filt[w] (bit widths of tns.js:47-48).   */
typedef struct aacg_tns_info {
    uint8_t n_filt[8];
    aacg_tns_filter filt[8];
} aacg_tns_info;

/* The ICSInfo fields the path reads (ics.js:270-314), one per channel, 16 bytes. */
typedef struct aacg_chan_info {
    uint8_t window_sequence;    /* info.windowSequence                                         */
    uint8_t window_shape;       /* info.windowShape[1]: 0 sine, 1 KBD                          */
    uint8_t window_shape_prev;  /* info.windowShape[0]; aac.js always has 0 here because it
                                   builds a fresh ICSInfo per frame (decoder.js:145,153)       */
    uint8_t max_sfb;            /* info.maxSFB                                                 */
    uint8_t group_count;        /* info.groupCount (1 for long windows)                        */
    uint8_t flags;              /* AACG_CHAN_*                                                 */
    uint8_t reserved[2];
    uint8_t group_len[8];       /* info.groupLength[g]                                         */
} aacg_chan_info;

#define AACG_CHAN_TNS_PRESENT    0x01   /* ics.tnsPresent (ics.js:71); only read in AACG_TNS_SPEC mode */
#define AACG_UNIT_COMMON_WINDOW 0x01   /* cpe.commonWindow (cpe.js:43)  */
#define AACG_UNIT_MASK_PRESENT  0x02   /* cpe.maskPresent  (cpe.js:47)  */
#define AACG_UNIT_CCE           0x08   /* a coupling channel element (AACG_CCE_SPEC engines): one channel; `channel` is a
                                          stream channel beyond the n_out_ch output channels (it owns overlap state when the
                                          coupling is independent — such an element must then be present in every frame of the
                                          stream's batch, like any element with state — it is never interleaved); reserved1 =
                                          index of its aacg_cce_info                                                     */
#define AACG_UNIT_HAS_PNS       0x04   /* some band of the unit is NOISE_BT (the parser knows, ics.js:84-121):
                                          AACG_PNS_SPEC engines route such batches through the PNS stage,
                                          AACG_PNS_REFERENCE engines refuse them                          */

/* One SCE/LFE/CPE of one frame, 64 bytes.  Units of one stream must be listed in
 * decode order; units that share `stream` and `pcm_offset` form one frame.          */
typedef struct aacg_unit_desc {
    uint32_t stream;        /* stream slot: owner of the overlap state                         */
    uint32_t pcm_offset;    /* float offset of this frame's [1024][n_out_ch] block in pcm_out  */
    uint16_t channel;       /* first output channel of the element (decoder.js:233-247)        */
    uint16_t n_out_ch;      /* channels per frame of this stream = interleave stride
                               (config.chanConfig, decoder.js:219)                             */
    uint8_t  n_ch;          /* 1 = SCE/LFE, 2 = CPE                                            */
    uint8_t  flags;         /* AACG_UNIT_*                                                     */
    uint16_t reserved0;
    uint32_t coef_offset;   /* channel c's spectrum starts at (coef_offset + c) * 1024 elements */
    uint32_t meta_offset;   /* channel c's aacg_band_meta is meta[meta_offset + c] (QUANT only) */
    aacg_chan_info ch[2];   /* [0] = left / the single channel, [1] = right                    */
    uint32_t tns_offset;    /* channel c's aacg_tns_info is tns[tns_offset + c] (if TNS present)  */
    uint32_t reserved1;
} aacg_unit_desc;

/* Per-channel band side info for AACG_INPUT_QUANT_I16, 240 bytes: one 16-bit word per
 * (group, sfb), index g*max_sfb + sfb exactly like ICStream.bandTypes / scaleFactors
 * (ics.js:217).
 *   bits 0..8   index into SCALEFACTOR_TABLE (tables.js:168-176), 0..427
 *   bit  9      negate the looked-up value (noise bands store -SF, ics.js:159)
 *   bit  10     ms_used[idx] (cpe.js:50-63); read from the LEFT channel's meta
 *   bits 12..15 band type (ics.js:37-42)                                            */
typedef struct aacg_band_meta {
    uint16_t band[AACG_MAX_SECTIONS];
} aacg_band_meta;

#define AACG_META_SF_MASK   0x01FFu
#define AACG_META_NEGATE    0x0200u
#define AACG_META_MS_USED   0x0400u
#define AACG_META_BT_SHIFT  12

enum {                          /* aacg_config.output_kind (ABI version 4)                          */
    AACG_OUTPUT_F32 = 0,        /* the reference's output: interleaved float in [-1, 1) (decoder.js:203-215)   */
    AACG_OUTPUT_I16 = 1         /* the same samples as int16: round-to-nearest(x * 32768), saturated — half the
                                   bytes of the path's dominant stream, for hosts that feed 16-bit sinks.  Every
                                   `pcm` pointer of such an engine is an int16_t*, every PCM count is in samples.
                                   Not aac.js behaviour: an explicit output format.  A NaN
                                   sample (the reference's out-of-range IQ read, |q| >= 8191) becomes -32768: the
                                   clamp is v_med3_f32, whose result with a NaN operand is the least of the other
                                   two (tests/test_output_edges.py pins it on the device and in the emulator)     */
};

typedef struct aacg_config {
    int32_t abi_version;       /* AACG_ABI_VERSION                                             */
    int32_t device_ordinal;    /* HIP device                                                   */
    int32_t sample_index;      /* config.sampleIndex (decoder.js:63); selects SWB tables, 3 = 48 kHz */
    int32_t max_streams;       /* stream slots with overlap state                              */
    int32_t max_channels;      /* channels per stream, <= AACG_MAX_CHANNELS                    */
    int32_t max_batch_units;   /* capacity of the host-buffer path (aacg_decode_batch)         */
    int32_t input_kind;        /* AACG_INPUT_*                                                 */
    int32_t tns_mode;          /* AACG_TNS_*                                                   */
    int32_t pns_mode;          /* AACG_PNS_* (ABI version 2)                                   */
    int32_t output_kind;       /* AACG_OUTPUT_* (ABI version 4)                                */
    int32_t cce_mode;          /* AACG_CCE_* (ABI version 4)                                   */
} aacg_config;

typedef struct aacg_engine aacg_engine;
typedef struct aacg_plan   aacg_plan;

/* ---- lifetime ------------------------------------------------------------------ */
/* new FilterBank(false, channels) for every stream slot (filter_bank.js:24-44): builds the
 * window / twiddle tables on the device and zeroes all overlap state.                  */
int  aacg_create(const aacg_config* cfg, aacg_engine** out);
void aacg_destroy(aacg_engine* e);
const char* aacg_last_error(const aacg_engine* e);   /* text of the last failure            */
int  aacg_abi_version(void);
/* Every wait of the host for the GPU behind this ABI — aacg_synchronize, aacg_wait, aacg_get/set_overlap, aacg_reset_stream,
 * aacg_plan_destroy, the back-pressure of aacg_decode_pipelined, aacg_decode_batch* — is bounded: after `ms` milliseconds
 * (default 30 000) it returns AACG_ERR_TIMEOUT.  A wait polls for a few microseconds and then sleeps between polls: it does not
 * hold the caller's core.  (`readChunk()` in the reference returns or throws, decoder.js:125-216; it never blocks.)        */
int  aacg_set_wait_limit_ms(aacg_engine* e, uint32_t ms);

/* ---- overlap state (filter_bank.js:38-41) ------------------------------------------ */
int aacg_reset_stream(aacg_engine* e, uint32_t stream);                       /* zero = new FilterBank */
int aacg_get_overlap(aacg_engine* e, uint32_t stream, uint32_t channel, float* dst1024);
int aacg_set_overlap(aacg_engine* e, uint32_t stream, uint32_t channel, const float* src1024);
/* The other half of a stream's filterbank state: the window shape (0 sine, 1 KBD) of the channel's last frame, which the first
 * half of its next frame is windowed with.  The engine keeps it where aacg_plan_carry_window_shape carries it (0 at create and
 * after aacg_reset_stream); a checkpoint of a stream holds both halves.  Bounded waits, as aacg_get / aacg_set_overlap. */
int aacg_get_window_shape(aacg_engine* e, uint32_t stream, uint32_t channel, uint8_t* shape);
int aacg_set_window_shape(aacg_engine* e, uint32_t stream, uint32_t channel, uint8_t shape);

/* ---- the hot path, host buffers ---------------------------------------------------- */
/* Synchronous equivalent of  process(elements) + interleave  for a whole batch:
 * uploads units/coefficients, runs the kernels, downloads PCM.
 *   coeffs  float[...] (SPEC_F32) or int16_t[...] (QUANT_I16), n_coef_blocks * 1024 elements
 *   meta    aacg_band_meta[n_meta] or NULL (SPEC_F32)
 *   pcm_out float[n_pcm_floats] (int16_t[n_pcm_floats] for AACG_OUTPUT_I16 engines); every frame block [1024][n_out_ch] is fully written
 *           (channels no unit covers are zero, decoder.js:229-231), scale 1/32768.   */
int aacg_decode_batch(aacg_engine* e,
                      const aacg_unit_desc* units, uint32_t n_units,
                      const void* coeffs, uint32_t n_coef_blocks,
                      const aacg_band_meta* meta, uint32_t n_meta,
                      void* pcm_out, size_t n_pcm_floats);

/* Asynchronous pair of the same call, for pipelining: aacg_submit enqueues upload, kernels and
 * download of one batch on one of two internal HIP streams and returns a ticket; aacg_wait blocks
 * until that batch's pcm_out is complete.  Two batches may be in flight: the PCIe transfers of one
 * overlap the kernels of the other, while the kernels themselves run in submission order (they
 * chain through the overlap state).  Buffers must stay valid until the wait; transfers are truly
 * asynchronous only from/to pinned memory (aacg_host_alloc).  Tickets must be waited in order. */
int aacg_submit(aacg_engine* e,
                const aacg_unit_desc* units, uint32_t n_units,
                const void* coeffs, uint32_t n_coef_blocks,
                const aacg_band_meta* meta, uint32_t n_meta,
                void* pcm_out, size_t n_pcm_floats, uint64_t* ticket);
int aacg_wait(aacg_engine* e, uint64_t ticket);
/* The same three calls with TNS side info (AACG_TNS_SPEC engines; tns may be NULL otherwise). */
int aacg_decode_batch_tns(aacg_engine* e,
                          const aacg_unit_desc* units, uint32_t n_units,
                          const void* coeffs, uint32_t n_coef_blocks,
                          const aacg_band_meta* meta, uint32_t n_meta,
                          const aacg_tns_info* tns, uint32_t n_tns,
                          void* pcm_out, size_t n_pcm_floats);
int aacg_submit_tns(aacg_engine* e,
                    const aacg_unit_desc* units, uint32_t n_units,
                    const void* coeffs, uint32_t n_coef_blocks,
                    const aacg_band_meta* meta, uint32_t n_meta,
                    const aacg_tns_info* tns, uint32_t n_tns,
                    void* pcm_out, size_t n_pcm_floats, uint64_t* ticket);
/* ... and with coupling side info as well (AACG_CCE_SPEC engines): every array of a batch in one record. */
typedef struct aacg_batch {
    const aacg_unit_desc* units;  uint32_t n_units;
    const void* coeffs;           uint32_t n_coef_blocks;
    const aacg_band_meta* meta;   uint32_t n_meta;
    const aacg_tns_info* tns;     uint32_t n_tns;      /* NULL / 0: none */
    const aacg_cce_info* cce;     uint32_t n_cce;      /* NULL / 0: none */
    void* pcm_out;                size_t n_pcm_floats;
} aacg_batch;
int aacg_decode_batch_ex(aacg_engine* e, const aacg_batch* b);
int aacg_submit_ex(aacg_engine* e, const aacg_batch* b, uint64_t* ticket);
/* Pinned (page-locked) host memory for the calls above and for aacg_pipeline_*'s PCM.  Blocks under 8 MiB: hipHostMalloc.  Larger
 * ones — a batch's PCM, fresh for every batch of a host that keeps what it was given — are mapped as huge pages, faulted in by a
 * few threads at once and registered with the runtime (32 MiB: 0.6 ms instead of 3.5-6), zero-filled, 2 MiB aligned; both kinds
 * go back through aacg_host_free, from any thread. */
void* aacg_host_alloc(size_t bytes);
void  aacg_host_free(void* p);

/* ---- the hot path, device-resident ------------------------------------------------- */
/* A plan is the uploaded unit table plus the run table the kernel walks.  It can be
 * launched repeatedly: every launch continues the streams where the previous launch of
 * the same plan left them (the next batch of the same shape).                          */
int  aacg_plan_create(aacg_engine* e, const aacg_unit_desc* units, uint32_t n_units, aacg_plan** out);
/* with TNS side info (host pointer; becomes part of the plan like the unit table) */
int  aacg_plan_create_tns(aacg_engine* e, const aacg_unit_desc* units, uint32_t n_units,
                          const aacg_tns_info* tns, uint32_t n_tns, aacg_plan** out);
int  aacg_plan_create_ex(aacg_engine* e, const aacg_unit_desc* units, uint32_t n_units,
                         const aacg_tns_info* tns, uint32_t n_tns, const aacg_cce_info* cce, uint32_t n_cce, aacg_plan** out);
void aacg_plan_destroy(aacg_plan* p);
/* Launch on `hip_stream` (a hipStream_t passed as void*, NULL = the engine's own stream);
 * returns after enqueueing.  d_coeffs / d_meta / d_pcm are DEVICE pointers.
 * Every call is a NEW launch: the overlap-buffer parity and — for plans whose chains are longer than a run — the epoch of the
 * run-to-run rendezvous are arguments of that launch.  Do not capture a launch in a hipGraph and replay it: call again.
 * Launches of ONE plan are ordered on the device also when they go to different HIP streams (the engine inserts an event
 * wait when the stream changes).  Two PLANS that advance the same audio streams are the caller's to order (same HIP
 * stream, or an event between them): the engine checks their logical order (AACG_ERR_STALE_PLAN), not the device's.      */
int aacg_decode_device(aacg_engine* e, aacg_plan* p,
                       const void* d_coeffs, const aacg_band_meta* d_meta,
                       void* d_pcm, void* hip_stream);
/* Spectral stage only (dequant + MS + IS): writes float[(coef_offset + c) * 1024 ...] so
 * that tests can gate this stage bit-exact.  QUANT_I16 engines only.                   */
int aacg_spectral_device(aacg_engine* e, aacg_plan* p,
                         const void* d_coeffs, const aacg_band_meta* d_meta,
                         float* d_spec_out, void* hip_stream);
/* Waits (on the host) for hip_stream — NULL: the engine's own stream — and for every launch aacg_decode_pipelined has in flight. */
int aacg_synchronize(aacg_engine* e, void* hip_stream);

/* ---- the hot path, device-resident, consecutive launches OVERLAPPED ------------------------------------------------
 * aacg_decode_device puts every launch of a plan behind the one before it: the next batch's first frame needs the last
 * frame's tail (filter_bank.js:38-41, the only state the path carries; filter_bank.js:105-118 is the hand-over).  But that
 * dependency is per (stream, element) chain, not per launch: chain c of launch k + 1 needs chain c's tail of launch k and
 * nothing else.  aacg_decode_pipelined launches on engine-owned HIP streams taken in turn (three, or two for plans whose
 * launches are several rounds of workgroups anyway), so that launch k + 1 starts on the compute units launch k has already
 * left and a unit that is done with launch k + 1 finds work of launch k + 2; consecutive launches' chains meet in rendezvous
 * cells in global memory —
 * whichever side of a chain arrives first publishes what it has (launch k: the windowed tail = the new overlap state;
 * launch k + 1: its windowed first half and where the finished samples go) and leaves, the second finishes the frame.
 * Nobody waits for another workgroup, no dispatch order is assumed, and both arrival orders add the same two rounded
 * numbers: the PCM is bit-identical to aacg_decode_device's.
 *   - Plain batches (float or int16 PCM, no AACG_TNS_SPEC / AACG_PNS_SPEC stage, no coupling element) overlap; every other plan
 *     is accepted and runs behind the launch before it, as aacg_decode_device would run it.
 *   - Inputs must be complete when the call is made, or be produced on a stream the pipeline has been forked from
 *     (aacg_pipeline_fork) since; outputs are complete for work on hip_stream after aacg_pipeline_join(e, hip_stream) and
 *     for the host after aacg_pipeline_join(e, NULL) / aacg_synchronize.
 *   - Launches through other entry points (aacg_decode_device, aacg_submit*, another plan) are ordered behind the
 *     pipeline's by the engine; mixing costs the overlap, never the result.
 *   - BACK-PRESSURE: at most fifteen launches of a sequence are in flight.  A launch reuses the overlap buffers and cells of
 *     the launch sixteen before it, and instead of ordering that on the GPU (a wait in a queue costs what the overlap gains)
 *     the call itself waits — on the host, every second round of launches — until the round four (three streams) or six (two)
 *     rounds back is complete.  A caller that enqueues faster than the GPU decodes is slowed to the GPU's pace; nothing else
 *     changes (aacg_pipeline_order in aacg_routes.cpp is the rule, tests/test_routes.py walks it).
 * Replaces: one `readChunk()` worth of process() + interleave (decoder.js:201-215) per stream and frame, batch after batch. */
int aacg_decode_pipelined(aacg_engine* e, aacg_plan* p, const void* d_coeffs, const aacg_band_meta* d_meta, void* d_pcm);
/* the pipeline's later launches start after everything enqueued on hip_stream so far (inputs produced there) */
int aacg_pipeline_fork(aacg_engine* e, void* hip_stream);
/* work enqueued on hip_stream from now on starts after the pipeline's launches so far; NULL: the host waits for them */
int aacg_pipeline_join(aacg_engine* e, void* hip_stream);
/* What a caller of aacg_decode_pipelined should know about the engine's internal streams: *streams_used = how many of them the
 * current sequence of launches takes in turn (0 before the first pipelined launch); *concurrent = 1 if they were seen to run
 * side by side when the pipeline was set up, 0 if the runtime put them on one hardware queue — pipelined launches are then
 * correct but run one behind the other (the first successful aacg_decode_pipelined also leaves a note in aacg_last_error) —
 * -1 before the pipeline has been set up.  Either pointer may be NULL. */
int aacg_pipeline_info(const aacg_engine* e, int* streams_used, int* concurrent);

/* ---- introspection ---------------------------------------------------------------------------------------------- */
/* Copies the engine's host-built tables (what the device kernels read) for table KATs.
 * which: 0 IQ[8191], 1 SF[428], 2 sine1024, 3 kbd1024, 4 sine128, 5 kbd128               */
int aacg_get_table(aacg_engine* e, int which, float* dst, size_t n);
/* Name of the dominant kernel of the headline route (for matching rocprofv3 rows).      */
const char* aacg_kernel_name(void);
/* The launches aacg_decode_device makes for this plan, by kernel name, " + " between them (dst: n bytes);
 * _ex with pipelined != 0: the launches aacg_decode_pipelined makes. */
int aacg_plan_kernels(aacg_engine* e, const aacg_plan* p, char* dst, size_t n);
int aacg_plan_kernels_ex(aacg_engine* e, const aacg_plan* p, int pipelined, char* dst, size_t n);
/* (measurement and diagnostic entry points — timing marks, the copy calibration, stage-by-stage transforms, hand-made route
 * choices — are declared in aacgpu_tools.h: same library, nothing a host needs) */

/* ---- the bitstream front end on the device (optional; independent of aacg_engine) ---------------
 * One GPU lane parses one frame: what aac.js does serially per frame between `stream.peek(12)` and
 * `this.process(elements)` (decoder.js:126-201 element loop, ics.js:56-201,279-314, cpe.js:37-75,
 * tns.js:68-103, cce.js:45-119 parse-and-discard, huffman.js:1425-1490) for a whole batch of frames at
 * once, writing the records aacg_decode_* / aacg_plan_create* take.  The host keeps what is trivial and
 * serial: finding frame boundaries (ADTS frame_length, MP4 sample sizes) and numbering streams.
 *
 * The parser takes the 12 codebooks as (length, code word, values) lists — book 0 = scalefactors
 * (v[0] = 0..120, huffman.js HCB_SF), books 1..11 = spectral (huffman.js HCB1..HCB11; v[0..3] for books 1-4,
 * v[0..1] for 5-11; magnitudes for the unsigned books 3,4,7..11).  aacg_standard_codebooks() supplies the
 * ones of ISO/IEC 14496-3 (tables 4.A.1-4.A.12), which is what every AAC stream uses; a caller may pass any
 * other complete prefix codes over the same alphabets (the tests do).                                   */
typedef struct aacg_code_entry {
    uint32_t code;             /* the code word, right-aligned                                     */
    uint8_t  len;              /* its length in bits, 1..24                                        */
    int8_t   v[4];
    uint8_t  reserved[3];
} aacg_code_entry;

#define AACG_STANDARD_CODEBOOK_ENTRIES 1362   /* 121 + 4*81 + 2*81 + 2*64 + 2*169 + 289 */
/* Fills entries[AACG_STANDARD_CODEBOOK_ENTRIES] (book after book) and counts[12]; either may be NULL.
 * Returns the number of entries.  Replaces the private tables of src/huffman.js:22-1418.               */
uint32_t aacg_standard_codebooks(aacg_code_entry* entries, uint32_t counts[12]);

typedef struct aacg_parse_frame {
    uint32_t byte_offset;      /* of the frame in `bytes`: an ADTS frame (header included, decoder.js:129-130)
                                  or a bare raw_data_block                                         */
    uint32_t byte_length;
} aacg_parse_frame;

enum {                         /* aacg_parse_result.status; the reference's message for each in
                                  aacg_parse_status_string()                                       */
    AACG_PARSE_OK = 0,
    AACG_PARSE_INSUFFICIENT_DATA = 1,  /* the frame ended inside an element (AV.Bitstream underflow)   */
    AACG_PARSE_BAND_TYPE = 2,          /* ics.js:96  'Invalid band type: 12'                            */
    AACG_PARSE_TOO_MANY_BANDS = 3,     /* ics.js:105 'Too many bands'                                   */
    AACG_PARSE_SCALEFACTOR = 4,        /* ics.js:165 'Scalefactor out of range' (also below -100, where
                                          the reference reads outside its table)                        */
    AACG_PARSE_PULSE_IN_SHORT = 5,     /* ics.js:65  'Pulse tool not allowed in eight short sequence.'  */
    AACG_PARSE_PULSE_RANGE = 6,        /* ics.js:180,193,198 'Pulse SWB / offset out of range'          */
    AACG_PARSE_PULSE_DATA = 7,         /* ics.js:264 'TODO: add pulse data' (without AACG_PARSE_APPLY_PULSES) */
    AACG_PARSE_TNS_ORDER = 8,          /* tns.js:85  'TNS filter out of range' (> 20; > 12 when TNS records
                                          are requested, AACG_TNS_MAX_ORDER)                            */
    AACG_PARSE_PREDICTION = 9,         /* ics.js:318 'Prediction not implemented.'                      */
    AACG_PARSE_GAIN_CONTROL = 10,      /* ics.js:76  'TODO: decode gain control/SSR'                    */
    AACG_PARSE_PCE = 11,               /* decoder.js:184 'TODO: PCE_ELEMENT'                            */
    AACG_PARSE_MAX_SFB = 12,           /* max_sfb beyond the sampling rate's band count (the reference reads
                                          outside its offset table)                                     */
    AACG_PARSE_MS_MASK = 13,           /* cpe.js:66  'Reserved ms mask type: 3'                         */
    AACG_PARSE_ESCAPE = 14,            /* escape sequence longer than the standard's 13 bits            */
    AACG_PARSE_CAPACITY = 15,          /* more elements / channels in the frame than the caller allowed */
    AACG_PARSE_LAYOUT = 16             /* never written by the parser: aacg_plan_refresh_from_parse_ex marks a frame that parsed
                                          well but does not have the elements its stream's plan was made for (the reference decodes
                                          whatever elements a frame brings, decoder.js:233-247; a kept plan cannot)              */
};
#define AACG_PARSE_APPLY_PULSES      0x1u   /* add pulse data to the spectrum (ISO/IEC 14496-3 4.6.3.3) instead
                                               of failing the frame as the reference does              */
#define AACG_PARSE_REFERENCE_QUIRKS  0x2u   /* coupling channel elements consume the bits cce.js consumes
                                               (AFTER_IMDCT never matches, the band index only steps on coded
                                               bands) rather than the standard's syntax                  */
#define AACG_PARSE_SKIP_ZERO_FILL    0x4u   /* aacg_parse_device: do not zero d_q first; positions outside the coded bands then
                                               hold whatever was there — the transform never reads them (bands of type ZERO /
                                               NOISE / INTENSITY and bands beyond max_sfb are not taken from the spectrum) */
#define AACG_PARSE_HAS_PNS 0x1
#define AACG_PARSE_HAS_TNS 0x2
#define AACG_PARSE_HAS_CCE 0x4   /* the frame held a coupling channel element: parsed and dropped (what aac.js executes); a host that
                                    applies coupling (AACG_CCE_SPEC) takes such a frame's records from a front end that keeps them */
#define AACG_PARSE_CONCEALED 0x8 /* never written by the parser: the conceal stage (aacg_plan_conceal_refused, aacg_pipeline_set_concealment)
                                    marks a refused frame whose records it replaced by its stream's last good frame, faded; status,
                                    n_units and bits_used still tell of the refusal */
typedef struct aacg_parse_result {
    uint8_t  status;           /* AACG_PARSE_*; a failed frame's output records are unspecified
                                  (partially written; never uninitialised memory)                  */
    uint8_t  n_units;          /* SCE/LFE/CPE elements found = records written for this frame      */
    uint8_t  n_channels;
    uint8_t  flags;            /* AACG_PARSE_HAS_*, AACG_PARSE_CONCEALED                           */
    uint32_t bits_used;        /* consumed from byte_offset on, byte-aligned at the end            */
} aacg_parse_result;

typedef struct aacg_parser aacg_parser;
/* counts[b] entries of book b, concatenated in `entries`; every book must be a complete prefix code.  */
int aacg_parser_create(int device_ordinal, int sample_index, const aacg_code_entry* entries,
                       const uint32_t counts[12], aacg_parser** out);
void aacg_parser_destroy(aacg_parser* p);
const char* aacg_parser_last_error(const aacg_parser* p);
const char* aacg_parse_status_string(int status);
/* aacg_parse_batch's waits for the GPU are bounded like the engine's (aacg_set_wait_limit_ms): AACG_ERR_TIMEOUT after `ms`
 * milliseconds, default 30 000. */
int aacg_parser_set_wait_limit_ms(aacg_parser* p, uint32_t ms);

/* Frame f's element e lands in units[f * max_units + e]; its channels in q / meta / tns block
 * f * max_channels + (running channel index), which is what the record's coef_offset / meta_offset /
 * tns_offset say.  Left for the caller to fill before decoding: stream, pcm_offset, n_out_ch
 * (window_shape_prev is written as 0, as aac.js has it).  reserved0 carries (element type << 4) | id.
 * tns may be NULL: TNS side info is then consumed and dropped (AACG_TNS_REFERENCE engines).
 *
 * aacg_parse_batch: host pointers, returns when the results are there.
 * aacg_parse_device: DEVICE pointers, asynchronous on hip_stream; d_bytes 16-byte aligned with >= 32 readable
 * bytes after the last frame; zero-fills d_units, d_q, d_meta (and d_tns) itself, so a refused frame's records and
 * the element slots beyond a frame's count read as zero.  A parser may be used from several streams in turn: a launch
 * on another stream waits (on the device) for the parser's previous launch, whose lane-order scratch it reuses.   */
int aacg_parse_batch(aacg_parser* p, const uint8_t* bytes, size_t n_bytes,
                     const aacg_parse_frame* frames, uint32_t n_frames,
                     uint32_t max_units, uint32_t max_channels, uint32_t options,
                     aacg_unit_desc* units, int16_t* q, aacg_band_meta* meta, aacg_tns_info* tns,
                     aacg_parse_result* results);
int aacg_parse_device(aacg_parser* p, const void* d_bytes, const aacg_parse_frame* d_frames, uint32_t n_frames,
                      uint32_t max_units, uint32_t max_channels, uint32_t options,
                      aacg_unit_desc* d_units, int16_t* d_q, aacg_band_meta* d_meta, aacg_tns_info* d_tns,
                      aacg_parse_result* d_results, void* hip_stream);
const char* aacg_parse_kernel_name(void);

/* Where the raw_data_blocks lie in MP4 sample runs (decoder.js:125-133,199: a chunk buffer holds several samples back to
 * back, and only a parse of block k finds where block k + 1 starts).  A span is one such run: it starts at a block boundary
 * and holds whole blocks (a block it cuts off is refused: AACG_PARSE_INSUFFICIENT_DATA).  One GPU lane walks one span with the
 * frame parser's syntax and every store off; span s's blocks land in frames[s * max_frames + k], k < results[s].n_frames, as
 * (byte_offset in `bytes`, byte_length) — the frame table aacg_parse_batch / aacg_pipeline_decode take.  A lane stops at the
 * span's end, after max_frames blocks, or at the first block that does not parse: that block is listed too, with the rest of
 * the span as its length (what the frame parser is then given: it refuses the block with the same status), and its status
 * becomes the span's.  A block that starts with 0xFFF is read as an ADTS frame, as by the frame parser (decoder.js:129-130).
 * options: AACG_PARSE_APPLY_PULSES / AACG_PARSE_REFERENCE_QUIRKS as for the parse that follows (they decide which blocks parse).
 *
 * aacg_parse_walk: host pointers, returns when the results are there (bounded wait: AACG_ERR_TIMEOUT).
 * aacg_parse_walk_device: DEVICE pointers, asynchronous on hip_stream; d_bytes 16-byte aligned with >= 32 readable bytes after
 * the last span and fewer than 2^29 bytes in all.  Shares the lane-order scratch (and its rules) with aacg_parse_device. */
typedef struct aacg_walk_result {
    uint32_t n_frames;         /* blocks listed for the span, a refused one included                          */
    uint32_t status;           /* AACG_PARSE_OK: the span's end or max_frames was reached; else the last block's */
    uint32_t bytes_consumed;   /* from the span's start to the end of its last block that parsed: a span that
                                  stopped at max_frames resumes at byte_offset + bytes_consumed                 */
    uint32_t reserved;
} aacg_walk_result;
int aacg_parse_walk(aacg_parser* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* spans, uint32_t n_spans,
                    uint32_t max_frames, uint32_t options, aacg_parse_frame* frames, aacg_walk_result* results);
int aacg_parse_walk_device(aacg_parser* p, const void* d_bytes, const aacg_parse_frame* d_spans, uint32_t n_spans,
                           uint32_t max_frames, uint32_t options, aacg_parse_frame* d_frames, aacg_walk_result* d_results,
                           void* hip_stream);

/* Parser -> transform without the host in between.  A plan's run tables depend on which streams bring how many frames
 * of which element layout, not on what the frames contain; batch after batch of the same streams can therefore keep
 * ONE plan (built once from unit records that carry the structure: stream, pcm_offset, channel, n_out_ch, n_ch and the
 * coef / meta block offsets aacg_parse_device will use: block = frame * max_channels + channel) and
 * have its device unit records rewritten from aacg_parse_device's output: window info and flags
 * come from d_parsed_units (plan unit i <- parsed record i, so the plan's units must be listed frame by frame
 * with max_units per frame), the rest stays.  A frame the parser refused, an element that is not the one the plan
 * expects (other channels, other blocks), or a unit with noise bands (their stage is chosen when a plan is built) becomes a silent unit and is counted in *d_refused (device
 * counter, caller zeroes it).  Asynchronous on hip_stream; follow with aacg_decode_device on the same stream.
 * QUANT_I16 engines; with AACG_TNS_SPEC / AACG_PNS_SPEC for plans made for aacg_decode_pipelined_stages only (any other plan's
 * TNS records and noise-band route were prepared on the host, when it was built).                              */
int aacg_plan_refresh_from_parse(aacg_engine* e, aacg_plan* p, const aacg_unit_desc* d_parsed_units,
                                 const aacg_parse_result* d_results, uint32_t max_units, uint32_t* d_refused,
                                 void* hip_stream);
/* The same for plans that (a) list only the elements their streams have and (b) are refreshed while earlier launches of theirs
 * are still in flight — what a host does that keeps several batches of the same streams between bytes and PCM at a time.
 *   d_map (device, one per plan unit, or NULL = plan unit i <- parsed record i): where the parser put the unit's element
 *     (frame * max_units + element) and how many elements its frame must have.  The units of a frame must be listed next to
 *     each other in the frame's order.  A frame is then taken or refused AS A WHOLE: wrong element count, an element of other
 *     channels or blocks, a parse error -> every unit of it silent, *d_refused += 1 per frame, and d_results[frame].status
 *     becomes AACG_PARSE_LAYOUT where the parser had said OK (d_results is written).
 *   set: which of the plan's sets of unit records to rewrite (aacg_plan_set_unit_sets); the plan's next launch reads that set.
 *     With more than one set the call does not wait for the plan's launches in flight — the CALLER guarantees that no launch
 *     still reads `set` (e.g. its previous user's output has been waited for on hip_stream) — and a sequence of
 *     aacg_decode_pipelined launches is not interrupted by it: consecutive batches still overlap through the rendezvous cells. */
typedef struct aacg_refresh_map {
    uint32_t parsed_index;     /* frame * max_units + element                                                     */
    uint32_t frame_units;      /* bits 0..7: elements (SCE / CPE / LFE) the frame must have; 0: not checked, refusal per unit.
                                  bits 8..15: how many of them (the first ones) the plan lists, 0 = all — the reference drops
                                  the elements beyond chanConfig channels (decoder.js:233)                               */
} aacg_refresh_map;
int aacg_plan_set_unit_sets(aacg_engine* e, aacg_plan* p, uint32_t n_sets);     /* 1..8, before the plan's first launch */
int aacg_plan_refresh_from_parse_ex(aacg_engine* e, aacg_plan* p, const aacg_unit_desc* d_parsed_units,
                                    aacg_parse_result* d_results, uint32_t max_units, const aacg_refresh_map* d_map,
                                    uint32_t set, uint32_t* d_refused, void* hip_stream);
/* window_shape_prev carried on the device.  The parser writes window_shape_prev = 0 (a fresh ICSInfo per frame, decoder.js:145,153)
 * and the refresh copies it; a standard decoder windows a frame's first half with the PREVIOUS frame's shape.  This call, behind
 * aacg_plan_refresh_from_parse_ex on the same hip_stream and in front of the launch, sets it in the records of `set` (the same
 * caller's word about `set` as the refresh): for each stream of the plan, its frames in order, each unit's channel k (output
 * channel c = channel + k) takes the window_shape of the frame before as refreshed — 0 behind a frame the refresh made silent —
 * and the stream's first frame takes the engine's state of (stream, c), which the stream's last frame then replaces
 * (aacg_get / aacg_set_window_shape; 0 at create and after aacg_reset_stream).  Channels without a unit in the plan keep their state;
 * no other byte of a record changes.  One small launch (aacg_units_carry_shape); consecutive calls are ordered on the device
 * whatever their streams, and a call repeated before any launch has taken the records — the refresh of a plan that turned out
 * stale, done again, on the same plan or on the one made in its place — starts from the state its first attempt started from.
 * That is the engine's only notion of "the same batch": EVERY carry between two launches of the engine repeats the one before it.
 * So the records a carry prepared are launched (aacg_decode_pipelined, aacg_decode_pipelined_stages, aacg_decode_device) before the
 * next batch is carried, on whatever plan: two different batches carried back to back with no launch in between would both start
 * from the state in front of the first.
 *   d_map: the map the set was refreshed through (required: it says how many units a frame has).
 * Kept plans (with or without unit sets), shaped plans and plans for aacg_decode_pipelined_stages; QUANT_I16 engines.  A plan that
 * does not list each stream's frames one behind the other with the same elements next to each other in every frame is refused:
 * AACG_ERR_UNSUPPORTED, the reason in aacg_last_error. */
int aacg_plan_carry_window_shape(aacg_engine* e, aacg_plan* p, const aacg_refresh_map* d_map, uint32_t set, void* hip_stream);

/* ---- refused frames concealed on the device -------------------------------------------------------------------------------------
 * A frame the parser or the refresh refuses is a silent unit: 1024 zeros per channel that move the stream's overlap state on.  This
 * call, behind aacg_plan_refresh_from_parse_ex on the same hip_stream and in front of aacg_plan_carry_window_shape and the launch,
 * repeats the stream's last good frame in its place with a fade — by substituting RECORDS: the transform then produces exactly what
 * it would produce for a stream that held the substituted frame.  One small launch (aacg_units_conceal).
 *
 * THE RULE.  Each stream slot holds G, the records of its last good frame, or nothing, and r, the number of refused frames since G.
 * G is empty and r is 0 in a new state block's slots and for a stream whose record says `fresh`.  Take a stream's frames of the batch
 * in order; the stream has `kept` decoded elements (a stream with kept = 0 — no layout learnt — has no unit and is not touched, its
 * state neither).  A frame is REFUSED iff d_results[frame].status != AACG_PARSE_OK after the refresh: parse errors,
 * AACG_PARSE_LAYOUT, and on an engine without AACG_PNS_SPEC a frame whose unit has noise bands.
 *   A good frame.     G := the frame's kept elements — for each kept unit its refreshed flags and ch[0..1]; for each of its channels
 *                     the 1024 int16 of its spectrum block and the 120 words of its aacg_band_meta block.  r := 0.  The frame itself
 *                     is untouched.
 *   A refused frame.  r := min(r + 1, hold_frames + 1).  If G exists and r <= hold_frames the frame is CONCEALED:
 *                     - each kept element's plan unit takes G's flags and ch[] verbatim — window sequence, shape, max_sfb, grouping,
 *                       the MS flags; window_shape_prev is left to the carry stage — and the group map derived from them.  The
 *                       planner's fields stay: stream, pcm_offset, channel, n_out_ch, n_ch, coef_offset, meta_offset; tns_offset
 *                       stays 0;
 *                     - the frame's OWN spectrum blocks are overwritten with G's, all 1024 values per channel;
 *                     - its own band-word blocks are overwritten with G's words, all 120: in every word whose band type (bits
 *                       12..15) is 1..11 the scalefactor field (bits 0..8) becomes max(0, sf - r * fade_steps); words of band type
 *                       0, 13, 14 and 15 are copied unchanged; bits 9..11 are kept;
 *                     - d_results[frame].flags gains AACG_PARSE_CONCEALED.
 *                     Otherwise the frame stays the silent unit the refresh made.  status, n_units, bits_used and the refusal count
 *                     are NOT changed: the host still learns of every refusal.
 * Sources are good frames or G, never a concealed frame: a run of refused frames repeats ONE frame, each time fade_steps further
 * down (one step is the scalefactor table's 2^(1/4), 1.5 dB), and falls silent after hold_frames.
 *
 * d_state: aacg_conceal_state_bytes(n_slots, parse_channels) bytes of device memory, 16-byte aligned, zero when first used — two sides
 * per slot; a stream's record names the side its batch READS (bit 0 of `state`), the launch writes the other (the batch's last good
 * frame, or the old G carried over with the new r), and the caller flips the bit for the slot's next batch once this one is enqueued
 * (what a call that failed wrote lies in the side the slot does not read).  Consecutive calls are ordered on the device whatever
 * their streams: the engine records an event behind every launch and puts the next one behind it.
 * d_streams: one record per stream of the batch, in the batch's order (device memory; e.g. brought up with the batch's bytes).
 * longest: the largest `frames` among them.  d_results / d_q / d_meta: what aacg_parse_device wrote for the batch (parse_channels its
 * max_channels) and the refresh has marked; the blocks of refused frames and the results' flags are written.
 * fade_steps 0..64, hold_frames 1..255 (AACG_ERR_INVALID_ARG otherwise).  Shaped plans (aacg_plan_create_shaped) and the set shaped
 * and refreshed last only — a kept plan's refresh may be repeated when the plan has gone stale, and the stage is not idempotent:
 * AACG_ERR_UNSUPPORTED, as on an engine with AACG_TNS_SPEC or AACG_PNS_SPEC (the TNS records of a repeated frame and repeated noise
 * bands are not served); the reason in aacg_last_error. */
typedef struct aacg_conceal_stream {
    uint32_t frame_first;      /* the stream's first frame in the batch's packed order (aacg_shape_stream)                       */
    uint32_t frames;           /* its frames in this batch                                                                       */
    uint32_t unit_first;       /* its first plan unit                                                                            */
    uint32_t frame_units;      /* bits 0..7: the elements of its frames; bits 8..15: how many of them are decoded (kept)         */
    uint32_t slot;             /* the stream slot: owner of the state                                                            */
    uint32_t nch;              /* 2 bits per element 0..7: its channels (1 or 2), in the frame's order                           */
    uint32_t state;            /* bit 0: the side of the slot's state this batch reads; bit 1: fresh — that side counts as empty */
    uint32_t reserved;         /* zero                                                                                           */
} aacg_conceal_stream;
size_t aacg_conceal_state_bytes(uint32_t n_slots, uint32_t parse_channels);
int aacg_plan_conceal_refused(aacg_engine* e, aacg_plan* p, uint32_t set, aacg_parse_result* d_results, int16_t* d_q, aacg_band_meta* d_meta,
                              uint32_t parse_channels, const aacg_conceal_stream* d_streams, uint32_t n_streams, uint32_t longest,
                              void* d_state, uint32_t n_slots, uint32_t fade_steps, uint32_t hold_frames, void* hip_stream);

/* ---- TNS records made on the device (AACG_TNS_SPEC) ---------------------------------------------------------------------------
 * What the host planner makes of an aacg_tns_info before a launch can run its filters — per filter the sample range, the
 * direction and the direct-form coefficients (tns.js:111-152) — made where aacg_parse_device left its outputs instead: one small
 * launch on hip_stream and, behind it, the records' transition matrices.  The bytes are those of the host-made records.
 *   d_parsed_units, d_results, d_tns_info: aacg_parse_device's outputs of n_frames frames (max_units elements and parse_channels
 *     channel blocks per frame; d_tns_info must have been requested from the parser);
 *   d_records: aacg_tns_records_bytes(n_frames * parse_channels) bytes of device memory, 256-byte aligned.  Record
 *     tns_offset + c of a parsed unit is its channel c's, as in a host-made array; the record of a block no accepted frame's unit
 *     owns, or whose channel has no AACG_CHAN_TNS_PRESENT, is empty (order 0 in every slot).  Every record is written.
 * A frame the parser refused is not read.  TNS orders above AACG_TNS_MAX_ORDER never arrive (AACG_PARSE_TNS_ORDER refuses the
 * frame when TNS records are requested); a filter count or order beyond the syntax leaves its slots empty. */
size_t aacg_tns_records_bytes(uint32_t n_records);
int aacg_tns_records_from_parse(aacg_engine* e, const aacg_unit_desc* d_parsed_units, const aacg_parse_result* d_results,
                                const aacg_tns_info* d_tns_info, uint32_t n_frames, uint32_t max_units, uint32_t parse_channels,
                                void* d_records, void* hip_stream);
/* The optional stages between parser and transform without the host: on an engine with AACG_TNS_SPEC and / or AACG_PNS_SPEC
 * (AACG_INPUT_QUANT_I16, float32 PCM, no coupling) a plan made FOR THIS ROUTE holds structure only, and what a batch's frames
 * hold arrives with the launch — unit records through aacg_plan_refresh_from_parse_ex (TNS flags and tns_offset as parsed on
 * AACG_TNS_SPEC engines, units with noise bands taken on AACG_PNS_SPEC engines), TNS records through d_tns_records.
 *   aacg_plan_create_stages: a kept plan from units that carry the structure (as for aacg_plan_refresh_from_parse; no TNS flag,
 *     no noise-band flag).
 *   aacg_plan_create_shaped_stages: aacg_plan_create_shaped (below) for this route — the same capacity, sets and shaping calls.
 *     aacg_plan_create_shaped itself refuses an engine with optional stages, as it always did.
 *   aacg_decode_pipelined_stages: aacg_decode_pipelined with the batch's TNS records (aacg_tns_records_from_parse's buffer of
 *     n_tns_records records; NULL / 0 on an engine without AACG_TNS_SPEC).  The caller orders the launch behind the work that
 *     made them (aacg_pipeline_fork) and keeps them until the launch is complete.
 * Such a plan always launches aacg_imdct_run_quant_ex_rv on two pipeline streams (aacg_plan_kernels), whether or not a batch
 * holds a filter or a noise band: route, stream count and the rule which launches continue their predecessor do not depend on
 * a batch's content.  aacg_decode_device / aacg_decode_pipelined refuse it (AACG_ERR_UNSUPPORTED). */
int aacg_plan_create_stages(aacg_engine* e, const aacg_unit_desc* units, uint32_t n_units, aacg_plan** out);
int aacg_plan_create_shaped_stages(aacg_engine* e, uint32_t max_streams, uint32_t max_frames, uint32_t max_elems, uint32_t n_sets, aacg_plan** out);
int aacg_decode_pipelined_stages(aacg_engine* e, aacg_plan* plan, const void* d_coeffs, const aacg_band_meta* d_meta,
                                 const void* d_tns_records, uint32_t n_tns_records, void* d_pcm);

/* ---- a plan with a capacity instead of a shape: shaped on the device, batch by batch --------------------------------------
 * On the resident route a plan is a pure function of the batch's shape — the stream slots in order, each one's frame count
 * and element layout — and of the engine's overlap-buffer rotation.  aacg_plan_create builds it on the host, uploads it and
 * keeps it per shape; a plan made by aacg_plan_create_shaped has device buffers for the LARGEST batch instead (at most
 * max_streams streams of at most max_frames frames, max_elems decoded elements per frame; n_sets (1..8) sets of unit records,
 * run and link tables — a set is shaped for the next batch while launches that read another are in flight — and the in-launch
 * rendezvous cells, 16 KB per link and pipeline stream: none at max_frames <= 16), and every batch shapes one set with ONE
 * small launch (aacg_plan_shape) from a table of 48 bytes per stream: no host planner, no allocation, no
 * upload of O(units) bytes, no per-shape object to evict.  AACG_ERR_OUT_OF_MEMORY, with the sizes in aacg_last_error, if the
 * buffers cannot be had.
 * Per batch:  1. fill the caller's words of the table, one record per stream in the batch's order;
 *             2. aacg_plan_shape_table: the engine checks them (AACG_ERR_CAPACITY / AACG_ERR_INVALID_ARG before anything is
 *                enqueued or changed), adds run_first / link_first / rot from its current overlap rotation and books the
 *                shape for `set`; *n_units: the plan units of the shape (0: no stream has a layout — nothing to launch);
 *             3. bring the completed table to the device on hip_stream (e.g. with the batch's bytes);
 *             4. aacg_plan_shape_launch on the same stream: the refresh map into d_map (max_units: the parser's elements per
 *                frame), the unit records' planner part, run and link records into the set;
 *             5. aacg_plan_refresh_from_parse_ex with d_map and `set`, then aacg_decode_pipelined: it launches the set shaped
 *                last.  The caller guarantees that no launch still reads `set` (as for aacg_plan_set_unit_sets).
 * Such a plan holds the rendezvous cut of the run table only: aacg_decode_pipelined serves it; aacg_decode_device,
 * aacg_plan_refresh_units, aacg_spectral_device and aacg_plan_set_unit_sets refuse it (AACG_ERR_UNSUPPORTED), and it exists
 * on AACG_INPUT_QUANT_I16 engines without optional stages only (the resident route's).
 * Consecutive launches overlap through the cross-launch cells only if they were shaped from identical tables (the same slots
 * in the same order, the same counts and layouts; the rotation words apart) with nothing in between; any other launch opens a
 * new sequence behind everything in flight, as a launch of another plan object does. */
typedef struct aacg_shape_stream {
    /* the caller's words */
    uint32_t frame_first;      /* the stream's first frame in the batch's packed order: the sum of `frames` over the streams before it */
    uint32_t frames;           /* its frames in this batch, 1..max_frames                                                       */
    uint32_t unit_first;       /* its first plan unit: the sum of frames * kept over the streams before it                      */
    uint32_t frame_units;      /* bits 0..7: the elements of its frames (n); bits 8..15: how many of them are decoded (kept);
                                  kept = 0: no layout yet, no unit (aacg_refresh_map.frame_units)                              */
    uint32_t slot;             /* the stream slot: owner of the overlap state                                                   */
    /* the engine's words (aacg_plan_shape_table) */
    uint32_t run_first;        /* the stream's first run in generation order (chains by slot, then channel)                     */
    uint32_t link_first;       /* ... and its first link                                                                        */
    uint32_t rot;              /* 4 bits per channel 0..7: the overlap buffer that holds the channel's state                    */
    /* the caller's again */
    uint32_t nch;              /* 2 bits per element 0..7: its channels (1 or 2), in the frame's order                          */
    uint32_t reserved[3];      /* zero                                                                                          */
} aacg_shape_stream;
int aacg_plan_create_shaped(aacg_engine* e, uint32_t max_streams, uint32_t max_frames, uint32_t max_elems, uint32_t n_sets, aacg_plan** out);
int aacg_plan_shape_table(aacg_engine* e, aacg_plan* p, uint32_t set, aacg_shape_stream* table, uint32_t n_streams,
                          uint32_t parse_channels, uint32_t* n_units);
int aacg_plan_shape_launch(aacg_engine* e, aacg_plan* p, const aacg_shape_stream* d_table, uint32_t max_units,
                           aacg_refresh_map* d_map, void* hip_stream);

/* The host's counterpart of aacg_plan_refresh_from_parse, for callers that parse on the CPU (the JavaScript front end) but
 * keep spectra and PCM on the device: batch after batch of the same streams keeps ONE plan, and the next batch's unit
 * records — same streams, frames, elements and PCM positions; new window sequences, shapes, grouping, flags and block
 * offsets — replace the plan's (validated like aacg_plan_create validates them, then one asynchronous copy on hip_stream;
 * follow with aacg_decode_device on the same stream).  AACG_ERR_LAYOUT_CHANGE if the structure differs (nothing is
 * changed then: build a new plan); plans with TNS records, noise bands or coupling elements are built per batch
 * (AACG_ERR_UNSUPPORTED).  Replaces decoder.js:138-198's per-frame `new ICStream` bookkeeping for a whole batch.
 * A plan with ONE set of unit records only: after aacg_plan_set_unit_sets(n > 1) the plan's launches read the set a device
 * refresh chose, the host's records have no set to go to, and the call is refused (AACG_ERR_UNSUPPORTED, the reason in
 * aacg_last_error; nothing is changed). */
int aacg_plan_refresh_units(aacg_engine* e, aacg_plan* p, const aacg_unit_desc* units, uint32_t n_units, void* hip_stream);

/* ---- bytes in, PCM out: front end and transform resident, ONE call per batch, several batches in flight ---------------
 * What a host of the reference does per stream and per frame in readChunk() (decoder.js:125-216: parse the raw_data_block,
 * process(elements), interleave) for a batch of streams at once: the frames' bytes go up, aacg_parse_device writes the
 * records in HBM, aacg_plan_refresh_from_parse_ex turns them into a kept plan's unit records, aacg_decode_pipelined runs the
 * transform, the PCM comes down; nothing but the frame boundaries (ADTS frame_length) and the stream slots is the host's.
 * A batch takes one of `lanes` sets of device buffers and a HIP stream of its own: batch k's PCM is on its way down PCIe
 * while batch k + 1's bytes go up and are parsed, and the transform launches of consecutive batches of one shape are
 * consecutive launches of ONE plan through aacg_decode_pipelined (they overlap through the rendezvous cells).
 * channels 1 / 2: every frame one SCE / one CPE (channel_configuration 1 / 2; any other frame is refused).  channels 3..8: the
 * reference's chanConfig (decoder.js:77,219: the number of output channels); a stream's element layout — the SCE / CPE / LFE
 * elements of a frame in order, channels dealt out in element order, elements beyond `channels` dropped (decoder.js:233-247) —
 * is learnt from the first frame it submits after aacg_pipeline_reset_stream, and a later frame with other elements is
 * refused as a whole (AACG_PARSE_LAYOUT).  Coupling channel elements are parsed and dropped, as the reference executes them.
 * A pipeline owns an engine (AACG_INPUT_QUANT_I16; AACG_TNS_REFERENCE / AACG_PNS_REFERENCE unless aacg_pipeline_config.stages says
 * otherwise) and a parser; it is not re-entrant. */
typedef struct aacg_pipeline aacg_pipeline;
typedef struct aacg_pipeline_config {
    int32_t abi_version;       /* AACG_ABI_VERSION                                                          */
    int32_t device_ordinal;
    int32_t sample_index;      /* config.sampleIndex (decoder.js:63)                                        */
    int32_t max_streams;       /* stream slots with overlap state                                           */
    int32_t channels;          /* 1..8: channels of a frame's PCM (the reference's chanConfig)               */
    int32_t max_frames;        /* frames per stream in one batch, at most                                   */
    int32_t output_kind;       /* AACG_OUTPUT_*                                                             */
    int32_t parse_options;     /* AACG_PARSE_* (AACG_PARSE_REFERENCE_QUIRKS for what aac.js reads)          */
    int32_t lanes;             /* batches in flight at most, 1..8; 0 = 5 (ABI version 6)                     */
    int32_t plan_mode;         /* 0: kept plans per batch shape (aacg_plan_create per new shape).  1: device plans — ONE plan
                                  shaped on the device for every batch (aacg_plan_create_shaped): no plan build, no allocation
                                  and no host wait on the submit path when a batch has a shape not seen before.  A scaffold for
                                  one round: mode 0 is what existing callers get and what the tests compare mode 1's bits
                                  against; once mode 1 is measured the switch and mode 0's path (plan_for, its LRU, the
                                  stale-plan retry) go.  (reserved[0] until now: zero selects today's path)                */
    int32_t stages;            /* AACG_PIPELINE_STAGE_*: the spec-correct optional stages on this route.  Bit 0: AACG_TNS_SPEC —
                                  the parser writes TNS side info, aacg_tns_records_from_parse makes the records on the lane's
                                  stream behind the parse, the transform runs the filters.  Bit 1: AACG_PNS_SPEC — a frame with
                                  noise bands is decoded instead of refused.  With either the engine is created in those modes
                                  and every launch goes through aacg_decode_pipelined_stages (aacg_imdct_run_quant_ex_rv), in
                                  both plan modes.  Needs AACG_OUTPUT_F32 (AACG_ERR_UNSUPPORTED with AACG_OUTPUT_I16: that route is
                                  the staged spectral launch, which needs a spectrum buffer per plan and does not overlap).
                                  Unchanged: TNS orders 13..20 refuse the frame (AACG_PARSE_TNS_ORDER), coupling elements are
                                  parsed and dropped.  Bit 2: AACG_PIPELINE_STAGE_WINDOW_SHAPE — each channel's window shape is
                                  carried from frame to frame and batch to batch (aacg_plan_carry_window_shape, one small launch
                                  per batch behind the refresh): a frame's first half is windowed with the previous frame's
                                  shape, as a standard decoder does, where the reference always takes sine.  Independent of
                                  bits 0 and 1: it selects no engine mode and no other kernel, and it goes with AACG_OUTPUT_I16.
                                  With the bit clear window_shape_prev is 0.  (reserved[0] until now: zero selects today's
                                  path, call for call)                                                                     */
    int32_t reserved[1];       /* zero                                                                      */
} aacg_pipeline_config;
#define AACG_PIPELINE_STAGE_TNS 1
#define AACG_PIPELINE_STAGE_PNS 2
#define AACG_PIPELINE_STAGE_WINDOW_SHAPE 4
int  aacg_pipeline_create(const aacg_pipeline_config* cfg, const aacg_code_entry* entries, const uint32_t counts[12], aacg_pipeline** out);
void aacg_pipeline_destroy(aacg_pipeline* p);
const char* aacg_pipeline_last_error(const aacg_pipeline* p);
int  aacg_pipeline_reset_stream(aacg_pipeline* p, uint32_t slot);                 /* new FilterBank for that slot (and sine for its carried window shapes) */
/* One batch, synchronous: n_streams streams (slots[s]: the stream slot that owns stream s's overlap state; each slot at most
 * once per batch: AACG_ERR_INVALID_ARG otherwise), the next
 * frames_per_stream frames of each; frames[s * frames_per_stream + f] = frame f of stream s in `bytes` (an ADTS frame,
 * header included, or a bare raw_data_block).  pcm_out: [stream][frame][1024][channels] (float, or int16 for
 * AACG_OUTPUT_I16 pipelines), any host memory — page-locked memory (aacg_host_alloc) receives the PCM straight from the
 * device, other memory through the pipeline's staging and one more host copy.  results (optional): one aacg_parse_result per frame; a frame the parser
 * refused (or whose element is not the one the pipeline was made for) is decoded as silence — its stream's state moves on
 * through a silent frame — and counted in *n_refused: the caller raises the reference's error for it
 * (aacg_parse_status_string) where the frame is reached. */
int  aacg_pipeline_decode(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                          const uint32_t* slots, uint32_t n_streams, uint32_t frames_per_stream,
                          void* pcm_out, aacg_parse_result* results, uint32_t* n_refused);
/* The asynchronous pair of the same call.  aacg_pipeline_submit stages the bytes (they may be reused when it returns),
 * enqueues the batch on the next lane and returns a ticket; pcm_out / results / n_refused are written by the time
 * aacg_pipeline_collect(ticket) returns and must stay valid until then.  Batches decode in submission order (consecutive
 * batches of a stream chain through its overlap state); up to `lanes` may be in flight — submitting one more first finishes
 * the oldest (its outputs are then complete, collecting it later returns at once).  Tickets count from 1.
 * aacg_pipeline_collect waits at most the wait limit (aacg_pipeline_set_wait_limit_ms, default 30 s): AACG_ERR_TIMEOUT, with
 * the lanes' and the engine's state in aacg_pipeline_last_error.  Replaces decoder.js:125-216 for a batch, without the
 * caller's thread waiting for PCIe. */
int  aacg_pipeline_submit(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                          const uint32_t* slots, uint32_t n_streams, uint32_t frames_per_stream,
                          void* pcm_out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket);
int  aacg_pipeline_collect(aacg_pipeline* p, uint64_t ticket);
/* Ragged batches: each stream brings its own number of frames (what one decoder per stream decodes of whatever its stream has,
 * decoder.js:125-216).  Stream s brings frames_of[s] consecutive frames (1 <= frames_of[s] <= max_frames), listed at
 * frames[first_s .. first_s + frames_of[s]), first_s = frames_of[0] + ... + frames_of[s - 1]; pcm_out is
 * [first_s + f][1024][channels] and results one record per frame, both in that same packed order.  The batch's frames, the
 * sum of the counts, are at most max_streams x max_frames.  A count of 0 or a slot listed twice is AACG_ERR_INVALID_ARG, a count
 * over max_frames or a total over capacity AACG_ERR_CAPACITY: nothing is enqueued then, no ticket is taken and
 * aacg_pipeline_last_error says why.  Otherwise as aacg_pipeline_decode / aacg_pipeline_submit, which are the case of every
 * count equal to frames_per_stream (frames[s * F + f] is frames[first_s + f] then) and give the same bits.  A kept plan serves
 * the batches of one shape: the same slots in the same order with the same counts. */
int  aacg_pipeline_decode_ragged(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                 const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                 void* pcm_out, aacg_parse_result* results, uint32_t* n_refused);
int  aacg_pipeline_submit_ragged(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                 const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                 void* pcm_out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket);
/* PCM left on the device: aacg_pipeline_submit_ragged in every respect — bytes, frames, slots, counts, results, the refusal count,
 * tickets, lanes, both plan modes, every `stages` bit, both output kinds (the element is float, or int16 for AACG_OUTPUT_I16
 * pipelines) — except where the PCM goes: into device memory of the caller's, for a consumer that computes on the card it decodes
 * on.  Nothing of the PCM crosses the link and no host PCM staging is allocated or touched for such a batch; results and the
 * refusal count still come down, and aacg_pipeline_collect serves these tickets too: the PCM is complete in d_pcm when it returns.
 *   AACG_PCM_PACKED: d_pcm is what the transform is launched with, in the place of the lane's own buffer — no extra pass, no extra
 *     traffic.  The batch needs n x 1024 x channels elements, n the sum of the counts.
 *   AACG_PCM_PLANAR: the transform writes the lane's buffer as ever and one more launch on the lane's stream (aacg_pcm_planar_*)
 *     writes the caller's tensor, padding included: every element of the n_streams x channels x stride_frames x 1024 block, once.
 * The batch writes d_pcm on a stream of the pipeline's own, ordered behind nothing of the caller's: whatever the caller has queued
 * that reads or writes d_pcm — a consumer of the memory's previous contents, a fill, a stream-ordered allocator that has just handed
 * the block out again — must have COMPLETED when this call is made (synchronise that stream, or an event of it, first).  From
 * then on d_pcm must stay valid, and unwritten by the caller, until aacg_pipeline_collect(ticket) has returned or the stream given
 * to aacg_pipeline_wait_device has passed the wait (a batch's predecessor may write the batch's first frames before the batch's
 * own launch starts).  Bytes of d_pcm behind what the batch needs are never written.
 * Refused before anything is enqueued, with no ticket taken and the reason in aacg_pipeline_last_error — AACG_ERR_INVALID_ARG: a null
 * `out` or d_pcm; a d_pcm that is not 16-byte aligned; a d_pcm that is not device memory of the pipeline's device (pageable or
 * page-locked host memory, another device's memory); a layout that is not one of the two; AACG_PCM_PLANAR with stride_frames below the
 * largest count; AACG_PCM_PACKED with stride_frames != 0.  AACG_ERR_CAPACITY: d_pcm_bytes smaller than the batch needs.  And whatever aacg_pipeline_submit_ragged refuses. */
#define AACG_PCM_PACKED 0   /* the host call's layout: [first_s + f][1024][channels], streams packed one behind the other */
#define AACG_PCM_PLANAR 1   /* [stream s][channel c][stride_frames * 1024]: stream s's frames_of[s] * 1024 samples of channel c,
                               then zeros up to the row's end — a (B, C, T) tensor with its padding written */
typedef struct aacg_pcm_device_out {
    void*    d_pcm;          /* device memory on the pipeline's device, 16-byte aligned */
    size_t   d_pcm_bytes;    /* what the caller owns there: the call refuses a batch that does not fit */
    int32_t  layout;         /* AACG_PCM_* */
    uint32_t stride_frames;  /* PLANAR: frames per row, >= every frames_of[s]; PACKED: 0 */
} aacg_pcm_device_out;
int  aacg_pipeline_submit_device(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                 const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                 const aacg_pcm_device_out* out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket);
/* Puts hip_stream (a hipStream_t of the pipeline's device; NULL: the null stream) behind the ticket's batch: hipStreamWaitEvent on
 * the lane's completion event, the host does not wait — a consumer queues its own kernels on the PCM while further batches are
 * submitted.  A ticket that is already complete or collected: AACG_OK with nothing enqueued; a ticket never given out:
 * AACG_ERR_INVALID_ARG.  The results and the refusal count are the host's only after aacg_pipeline_collect. */
int  aacg_pipeline_wait_device(aacg_pipeline* p, uint64_t ticket, void* hip_stream);
int  aacg_pipeline_set_wait_limit_ms(aacg_pipeline* p, uint32_t ms);
/* Span walks on the pipeline's device (aacg_parse_walk's semantics and outputs, the pipeline's parse_options): where the blocks of
 * MP4 sample runs lie, ahead of the batches that decode them.  aacg_pipeline_walk_submit stages the bytes (they may be reused when
 * it returns) and enqueues the walk on a stream of its own — bytes up and results down through page-locked staging, no synchronous
 * copy and, once the buffers have grown, no allocation; frames[s * max_frames + k] (k < results[s].n_frames; the slots behind
 * are unspecified) and results are written by the time aacg_pipeline_walk_collect(ticket) returns and must stay valid until
 * then.  Up to two walks in flight: submitting a third first finishes the oldest.  Tickets count from 1, apart from the
 * batches'.  aacg_pipeline_walk_collect waits at most the wait limit: AACG_ERR_TIMEOUT with the lanes' and the engine's state. */
int  aacg_pipeline_walk_submit(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* spans, uint32_t n_spans,
                               uint32_t max_frames, aacg_parse_frame* frames, aacg_walk_result* results, uint64_t* ticket);
int  aacg_pipeline_walk_collect(aacg_pipeline* p, uint64_t ticket);
/* The element layout learnt for a stream slot: returns the number of SCE / CPE / LFE elements of its frames (0: not learnt
 * yet), their channel counts in element_channels[0..7] and how many of them (the first ones) fit `channels` in *kept. */
int  aacg_pipeline_stream_layout(aacg_pipeline* p, uint32_t slot, uint8_t element_channels[8], uint32_t* kept);
/* The window shape each output channel of a stream slot carries into its next frame (AACG_PIPELINE_STAGE_WINDOW_SHAPE; all 0
 * without it): shapes[c] for c < channels, 0 behind them.  Finishes the batches in flight first (bounded, as
 * aacg_pipeline_reset_stream). */
int  aacg_pipeline_stream_window_shape(aacg_pipeline* p, uint32_t slot, uint8_t shapes[8]);
/* A mix on the device: O = out_channels (1 or 2) channels leave a pipeline made for C = channels, so that a surround stream costs the
 * link what a stereo stream costs.  matrix is M, O rows of C floats, row-major.  THE RULE, bit for bit: for every sample t of every
 * frame a batch decodes and every output channel o, in float32 throughout,
 *     acc = M[o][0] * x[0]                           (rounded to float)
 *     acc = acc + (M[o][c] * x[c])    c = 1 .. C-1   (the product rounded, then the sum rounded: NOT fused, in this order)
 * Every term is computed, also those with a zero coefficient.  x[c] is the sample the unmixed pipeline would have delivered in channel
 * c, by position: channel c of a frame's PCM, whatever the stream's layout covers — a stream whose learnt layout covers fewer
 * channels than `channels` is mixed by position all the same, its uncovered channels are zeros.  numpy float32 arithmetic reproduces
 * the result exactly.
 *   AACG_OUTPUT_F32: out[o] = acc, no clamp.
 *   AACG_OUTPUT_I16: x[c] is the int16 sample converted to float (exact) — the ALREADY ROUNDED int16 the unmixed pipeline delivers, not
 *     the transform's float before its rounding — and out[o] is acc rounded to nearest even and saturated to [-32768, 32767].
 * Output layouts: as described above with O in the place of `channels` — host PCM and AACG_PCM_PACKED [first_s + f][1024][O],
 * AACG_PCM_PLANAR [stream][O][stride_frames * 1024] with its padding written; d_pcm_bytes and the host buffer need n x 1024 x O
 * (n_streams x O x stride_frames x 1024) elements.  A refused frame and a frame of an unlearnt stream are the mix of zeros.
 * Results, refusal counts, tickets, lanes, plan modes, `stages`, ragged batches and span walks are untouched: one more launch per
 * batch (aacg_pcm_mix_*) on the lane's stream, behind the transform, and with no mix set nothing differs.
 * Called once, before the pipeline's first submitted batch.  AACG_ERR_INVALID_ARG, with the reason in aacg_pipeline_last_error and the
 * pipeline exactly as it was: out_channels not 1 or 2, a null matrix, a coefficient that is not finite, a call after the first batch,
 * a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the lanes' mixed PCM; the pipeline stays unmixed. */
int  aacg_pipeline_set_mix(aacg_pipeline* p, uint32_t out_channels, const float* matrix);
/* The channels of the PCM the pipeline delivers: O with a mix set, `channels` otherwise. */
int  aacg_pipeline_out_channels(const aacg_pipeline* p);
/* The project's standard downmix for aacg_pipeline_set_mix, host code only (no device, no pipeline): matrix receives out_channels x
 * channels floats for the positions the resident route deals out, the element order of channel_configuration:
 *     channels 1: [C]            2: [L R]            3: [C L R]            4: [C L R Cs]
 *              5: [C L R Ls Rs]  6: [C L R Ls Rs LFE]                      8: [C Lc Rc L R Ls Rs LFE]        (7: AACG_ERR_INVALID_ARG)
 * Left row, with a = surround_gain: L and Lc 1, C 1/sqrt(2), Ls a, Cs a/sqrt(2), everything else 0 — the LFE included; the right row
 * mirrors it (R, Rc, C, Rs, Cs).  normalise != 0 divides each row by its sum (5.1 with a = 1/sqrt(2): the familiar 1 / (1 + 1/sqrt(2)
 * + 1/sqrt(2))).  out_channels 1: the one row (left + right) / 2.  Computed in double, each coefficient rounded to float once.  The
 * table is positional, like the mix.  AACG_ERR_INVALID_ARG: channels 0, 7 or above 8, out_channels not 1 or 2, a null matrix, a gain
 * that is not finite (or, with normalise, one that leaves a row without a positive sum). */
int  aacg_mix_standard(uint32_t channels, uint32_t out_channels, float surround_gain, int normalise, float* matrix);
/* A resampler on the device: the pipeline's PCM leaves at L / M times the streams' sample rate, so that a 16 kHz consumer of a 48 kHz
 * stream pulls a third of the samples across the link.  table is the polyphase table h[L][taps], row-major float32: row p holds the
 * `taps` coefficients of phase p (aacg_resample_design makes the usual one).  THE RULE, bit for bit.  Each stream slot has a clock N,
 * the input samples per channel it has consumed since aacg_pipeline_reset_stream (or create).  Output sample m = 0, 1, 2, ... of a
 * slot's channel since then is, with i = floor(m M / L) and p = (m M) mod L, in float32 throughout,
 *     acc = h[p][0] * x[i]                             (rounded to float)
 *     acc = acc + (h[p][t] * x[i - t])   t = 1 .. taps-1   (the product rounded, then the sum rounded: NOT fused, in this order)
 * Every term is computed, whatever its coefficient; x[j] = 0 for j < 0.  x is the slot's PCM as the pipeline would have delivered it
 * without a resampler, batch after batch — AFTER the mix if one is set, so the resampler works on the out_channels mixed channels; a
 * refused frame and a frame of an unlearnt stream are 1024 zeros, and they advance the clock like any other.  numpy float32 arithmetic
 * reproduces the result exactly.
 *   AACG_OUTPUT_F32: out = acc, no clamp.
 *   AACG_OUTPUT_I16: x is the ALREADY ROUNDED int16 sample converted to float (exact), and out is acc rounded to nearest even and
 *     saturated to [-32768, 32767] — the mix's int16 rule.
 * What a batch emits: a stream that brings F frames moves its clock from N to N' = N + 1024 F and emits the outputs m with
 * N <= i(m) < N', ceil(N' L / M) - ceil(N L / M) samples (frame f of the batch owns those with i(m) inside it).  The count depends on
 * N mod M only; aacg_pipeline_out_samples tells it for the next batch, aacg_resample_counts for any clock.  Any split of a stream's
 * frames into batches gives the same bits.  A reset sets N = 0, and the history is then zero by the rule.
 * Output layouts, with n_out[s] the samples of the batch's stream s and O the channels that leave: host PCM and AACG_PCM_PACKED
 * [stream s][n_out[s]][O], tight, the streams one behind the other (sum n_out[s] x O elements); AACG_PCM_PLANAR
 * [stream][O][stride_frames * 1024] with the padding behind n_out[s] written as zeros — stride_frames x 1024 must be at least every
 * n_out[s], and need not reach the frame counts.
 * Limits: taps a multiple of 4 in 4..64; L and M in 1..1024; L x taps <= 16384; 1/8 <= L / M <= 8; max_streams x max_frames x 1024 x
 * L / M below 2^31.  The group delay of a linear-phase table is (L taps - 1) / (2 L) input samples.
 * Results, refusal counts, tickets, lanes, plan modes, `stages`, ragged batches, span walks and the mix are untouched: one more launch
 * per batch (aacg_pcm_resample_*) on the lane's stream, behind the transform and the mix, ordered behind the previous batch's; with no
 * resampler set nothing differs.  Called once, before the pipeline's first submitted batch and after aacg_pipeline_set_mix if both
 * are used.  AACG_ERR_INVALID_ARG, with the reason in aacg_pipeline_last_error and the pipeline exactly as it was: a limit broken, a
 * null table, a coefficient that is not finite, a call after the first batch, a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory
 * for the table, the histories and the lanes' output; the pipeline stays as it was. */
int  aacg_pipeline_set_resample(aacg_pipeline* p, uint32_t L, uint32_t M, uint32_t taps, const float* table);
/* What the NEXT submission of these streams with these frame counts will emit, per stream: n_out[s] samples per channel, from the
 * slots' clocks as they stand (frames_of[s] x 1024 without a resampler).  The caller sizes pcm_out / d_pcm_bytes with it.  The clocks
 * advance when a batch has been enqueued; a refused submission leaves them alone.  AACG_ERR_INVALID_ARG: a null pointer, a slot out of
 * range, a count above max_frames. */
int  aacg_pipeline_out_samples(aacg_pipeline* p, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, uint32_t* n_out);
/* Host code only (no device, no pipeline): what `frames` consecutive frames emit at L / M from the clock n0 (any value; only n0 mod M
 * counts), frame by frame: per_frame[f] = ceil((n0 + 1024 (f + 1)) L / M) - ceil((n0 + 1024 f) L / M) (per_frame may be null), and
 * n0_after = (n0 + 1024 frames) mod M, the clock to continue with.  AACG_ERR_INVALID_ARG: L or M outside 1..1024. */
int  aacg_resample_counts(uint32_t L, uint32_t M, uint32_t n0, uint32_t frames, uint32_t* per_frame, uint32_t* n0_after);
/* The project's default table for aacg_pipeline_set_resample, host code only: L / M = out_rate / in_rate reduced, and into table (room
 * for `capacity` floats, at least L x taps) a Kaiser-windowed sinc: the prototype g[n], n = 0 .. L taps - 1, centred at (L taps - 1) /
 * 2, is sinc(2 fc (n - centre)) under a Kaiser window of shape beta, with the cutoff fc = 0.5 rolloff / max(L, M) cycles per upsampled
 * sample; h[p][t] = g[p + t L], each phase row divided by its sum, so that DC passes with gain 1 in every phase.  Computed in double,
 * each coefficient rounded to float once.  rolloff 0: 0.95; beta 0: 9.  Group delay: (L taps - 1) / (2 L) input samples.  With table
 * null and capacity 0 only L and M are written (to size the table).  AACG_ERR_INVALID_ARG: a rate of 0, a null L or M, taps or the
 * reduced L / M outside aacg_pipeline_set_resample's limits, rolloff outside (0, 1], beta outside (0, 30], a capacity below L x taps. */
int  aacg_resample_design(uint32_t in_rate, uint32_t out_rate, uint32_t taps, double rolloff, double beta, uint32_t* L, uint32_t* M, float* table, size_t capacity);
/* A feature stage on the device, the LAST stage of the way out: (log-)mel feature frames leave in the place of PCM, for a model that
 * computes on the card it decodes on (Whisper-style front ends: 400-sample frames every 160 samples of 16 kHz mono, 80 or 128 bands).
 * The stage is set by caller-supplied tables (aacg_features_design makes the usual ones), all row-major float32, every entry finite:
 *     K = frame_length, a multiple of 4 in 32..1024;  H = hop, 1..K;  P = pad_left, 0..K-1, the zeros assumed in front of the stream
 *     (P = 0: an un-centred STFT; P = K / 2: a centred one with zero padding on the left);  R = n_rows, even, 2..1026, the rows of
 *     basis[R][K], B = R / 2 bins whose two quadrature rows are rows 2b and 2b+1;  n_mels in 1..128 with fb[n_mels][B];  floor > 0
 *     and finite;  log, a flag.
 * The input x is the slot's PCM as the pipeline would have delivered it without the stage, batch after batch — after the mix and after
 * the resampler if they are set — and it must be ONE channel: channels == 1, or a mix with out_channels 1.  On an AACG_OUTPUT_I16
 * pipeline x is the already rounded int16 times 2^-15 (exact), so that both output kinds feed the stage the same scale.  x[n] = 0 for
 * n < 0; a refused frame and a frame of an unlearnt stream are zeros, and they advance the clock like any other.
 * THE RULE, bit for bit, in float32 throughout.  Feature frame j = 0, 1, ... of a slot since its reset covers x[j H - P + k], k = 0..K-1:
 *     lin[r] = fmaf(basis[r][K-1], x[jH-P+K-1], ... fmaf(basis[r][1], x[jH-P+1], fmaf(basis[r][0], x[jH-P], +0)) ...)
 *              one k-ordered FUSED chain from +0, every term computed
 *     pw[b]  = lin[2b] * lin[2b] + lin[2b+1] * lin[2b+1]          each product rounded, then the sum rounded: nothing fused
 *     mel[m] = the b-ordered fmaf chain of fb[m][b] * pw[b] from +0, over all B bins whatever their coefficient
 *     out[m] = mel[m], or with log: log10f(max(mel[m], floor)), the library function (within its 3 ulp, not bit-exact across libraries)
 * The output is float32 whatever the pipeline's output kind.
 * Counts: after N consumed samples a slot has emitted count(N) = max(0, floor((N + P - K) / H) + 1) frames; a batch that moves the
 * clock from N to N' emits count(N') - count(N), possibly none.  aacg_pipeline_out_samples answers in FEATURE FRAMES when the stage is
 * set, aacg_features_counts for any clock.  Any split of a stream's frames into batches gives the same bits.  A reset sets N = 0.
 * State per slot: the clock and the last K - 1 input samples, handed from batch to batch across lanes as the resampler's.
 * Output layouts, with n_out[s] the feature frames of the batch's stream s: host memory and AACG_PCM_PACKED [stream s][n_out[s]][n_mels],
 * tight, the streams one behind the other; AACG_PCM_PLANAR [stream][n_mels][stride_frames], a (B, n_mels, T) tensor — stride_frames
 * then counts FEATURE frames per row, 1..2^21 and at least every n_out[s], and the padding behind n_out[s] is written with the value
 * the rule gives for mel = 0: 0, or log10f(floor) with log.  Every element of the block is written exactly once, nothing outside it.
 * Limit: max_streams x max_frames x 1024 x (L / M) / H x n_mels below 2^31.
 * Results, refusal counts, tickets, lanes, plan modes, `stages`, ragged batches, span walks, the mix and the resampler are untouched:
 * one more launch per batch (aacg_pcm_features_*) on the lane's stream, ordered behind the previous batch's; with no stage set nothing
 * differs.  Called once, before the pipeline's first submitted batch and after aacg_pipeline_set_mix / aacg_pipeline_set_resample.
 * AACG_ERR_INVALID_ARG, with the reason in aacg_pipeline_last_error and the pipeline exactly as it was: a limit broken, a null table,
 * an entry that is not finite, a floor that is not positive and finite, more than one output channel, a call after the first batch, a
 * second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the tables, the histories and the lanes' output; the pipeline stays as it was. */
typedef struct aacg_features_config {
    uint32_t frame_length;   /* K */
    uint32_t hop;            /* H */
    uint32_t pad_left;       /* P */
    uint32_t n_rows;         /* R = 2 B */
    uint32_t n_mels;
    uint32_t log;            /* != 0: out = log10f(max(mel, floor)) */
    float    floor;
    const float* basis;      /* [n_rows][frame_length] */
    const float* fb;         /* [n_mels][n_rows / 2] */
} aacg_features_config;
int  aacg_pipeline_set_features(aacg_pipeline* p, const aacg_features_config* cfg);
/* Host code only: the feature frames that `samples` further samples complete at the clock n0, count(n0 + samples) - count(n0).
 * AACG_ERR_INVALID_ARG: frame_length, hop or pad_left outside aacg_pipeline_set_features's limits, a null n_frames. */
int  aacg_features_counts(uint32_t frame_length, uint32_t hop, uint32_t pad_left, uint64_t n0, uint64_t samples, uint64_t* n_frames);
/* The usual tables for aacg_pipeline_set_features, host code only: into basis (room for basis_capacity floats, at least 2 n_bins x
 * frame_length) the periodic Hann window w[k] = 0.5 - 0.5 cos(2 pi k / K) on a Fourier basis, basis[2b][k] = w[k] cos(2 pi b k / K) and
 * basis[2b+1][k] = -w[k] sin(2 pi b k / K) (the angle taken from (b k) mod K), and into fb (fb_capacity, at least n_mels x n_bins) the
 * Slaney mel filterbank with Slaney's area normalisation: the mel scale is 200 / 3 Hz per mel below 1 kHz and steps of ln(6.4) / 27
 * above it; n_mels + 2 edges f[] equally spaced in mel from f_min to f_max (0: rate / 2); row m is the triangle over f[m], f[m+1],
 * f[m+2] at the bins' frequencies b rate / K, scaled by 2 / (f[m+2] - f[m]).  Computed in double, each entry rounded to float once.
 * hop takes no part in the tables and is checked only.  Whisper's: rate 16000, frame_length 400, hop 160, n_bins 201, n_mels 80 or 128.
 * AACG_ERR_INVALID_ARG: a rate of 0, a null table, a parameter outside aacg_pipeline_set_features's limits (n_rows = 2 n_bins), f_min
 * negative, f_max not above f_min or above rate / 2, a capacity too small. */
int  aacg_features_design(uint32_t rate, uint32_t frame_length, uint32_t hop, uint32_t n_bins, uint32_t n_mels, double f_min, double f_max,
                          float* basis, size_t basis_capacity, float* fb, size_t fb_capacity);
/* A loudness meter on the device: a TAP, not a stage.  It reads the PCM the pipeline's TRANSFORM delivers and writes a few floats per
 * hop beside it, for a consumer that normalises what it decodes (EBU R 128 / ReplayGain) without pulling the full-rate, full-channel
 * PCM across the link; the PCM's own way out — the mix, the resampler, the feature stage, every destination — is untouched.
 *     hop: samples, 1..2^20;  coeffs[2][5]: two biquad sections {b0, b1, b2, a1, a2}, all finite (aacg_loudness_design makes BS.1770's).
 * The input x of channel c of a slot is the sample the transform delivers in channel c: BEFORE the mix, the resampler and the feature
 * stage, at the stream's own rate, in all `channels` channels by position.  On an AACG_OUTPUT_I16 pipeline x is the already rounded
 * int16 times 2^-15 (exact).  A refused frame and a frame of an unlearnt stream are 1024 zeros; they pass through the filters like any
 * other and advance the clock.
 * THE RULE, bit for bit, in float32 throughout, every operation rounded on its own, nothing fused, subnormals kept.  Per sample, for
 * section i = 0 then 1, with v = x going into section 0:
 *     y  = (b0 v) + z1
 *     z1 = ((b1 v) - (a1 y)) + z2
 *     z2 = (b2 v) - (a2 y)
 *     v  = y
 * then  e = e + (v v)  and  peak = max(peak, |x|).  After every `hop` samples since the slot's reset one record per channel leaves,
 * {e, peak}, two floats, and e and peak restart at +0.  A reset (aacg_pipeline_reset_stream) zeroes the clock, the four z of every
 * channel, e and peak.  Counts: count(N) = floor(N / hop); a batch that moves a slot's clock from N to N' emits count(N') - count(N)
 * records per channel, possibly none (aacg_pipeline_loudness_counts; aacg_loudness_counts for any clock).  Any split of a stream's
 * frames into batches gives the same bits.
 * Records of a submission: packed [stream s][n_out[s]][channels][2] float32, the streams one behind the other, in HOST memory that the
 * caller names with aacg_pipeline_loudness_out before every submission; they are there when the submission's ticket has been collected.
 * State per slot: the clock on the host; z1, z2 of both sections, the partial e and the partial peak per channel on the device, handed
 * from batch to batch across lanes as the resampler's history.  One more launch per batch (aacg_pcm_loudness_*) on the lane's stream
 * behind the transform; it goes with both output kinds, every `stages` bit, both plan modes, ragged and device batches and span walks,
 * and is independent of aacg_pipeline_set_mix / _set_resample / _set_features in order and in effect.  With no meter set nothing differs.
 * Called once, before the pipeline's first submitted batch.  AACG_ERR_INVALID_ARG, with the reason in aacg_pipeline_last_error and the
 * pipeline exactly as it was: a null config, a hop outside 1..2^20, a coefficient that is not finite, a call after the first batch, a
 * second call; and a pipeline beyond the meter's limits — max_streams x (max_frames x 1024 / hop + 1) x channels of 2^27 records or
 * more, max_streams x max_frames frames of PCM of 64 GiB or more.  AACG_ERR_OUT_OF_MEMORY: no device memory for the slots' state and the lanes' records; the pipeline stays as it was.
 * Not here: short-term windows and loudness range, a meter behind the mix or the resampler.  True (oversampled) peak: aacg_pipeline_set_true_peak, below. */
typedef struct aacg_loudness_config {
    uint32_t hop;
    float    coeffs[2][5];
} aacg_loudness_config;
int  aacg_pipeline_set_loudness(aacg_pipeline* p, const aacg_loudness_config* cfg);
/* Where the NEXT enqueued submission's records go: `records`, host memory with room for capacity_floats floats, valid until that
 * submission's ticket has been collected (the records are written at the collect); n_out_of (may be null) receives, when the
 * submission is enqueued, stream s's record count per channel at n_out_of[s].  One call arms one submission.  A submission on a
 * metered pipeline with no destination named is refused with AACG_ERR_INVALID_ARG, one whose destination is smaller than the sum of
 * n_out[s] x channels x 2 floats with AACG_ERR_CAPACITY: nothing is enqueued, no ticket is taken, no clock moves, and the destination
 * stays armed.  AACG_ERR_INVALID_ARG: a pipeline without a meter, null records with a capacity above 0. */
int  aacg_pipeline_loudness_out(aacg_pipeline* p, float* records, size_t capacity_floats, uint32_t* n_out_of);
/* What the NEXT submission of these streams with these frame counts will emit, per stream: n_out[s] records per channel, from the
 * slots' clocks as they stand.  aacg_pipeline_out_samples keeps its meaning.  AACG_ERR_INVALID_ARG: a null pointer, a pipeline without
 * a meter, a slot out of range, a count above max_frames. */
int  aacg_pipeline_loudness_counts(aacg_pipeline* p, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, uint32_t* n_out);
/* Host code only: the records per channel that `samples` further samples complete at the clock n0, floor((n0 + samples) / hop) -
 * floor(n0 / hop).  AACG_ERR_INVALID_ARG: a hop outside 1..2^20, a null n. */
int  aacg_loudness_counts(uint32_t hop, uint64_t n0, uint64_t samples, uint64_t* n);
/* Host code only: ITU-R BS.1770's K-weighting re-derived for any rate, in double, each value rounded to float once.  Row 0, the shelf:
 * f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / rate), Vh = 10^(G / 20),
 * Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;  b = {(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0},
 * a = {2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0}.  Row 1, the high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, b = {1, -2, 1},
 * a of the same form.  At 48000 these are the standard's published coefficients.  AACG_ERR_INVALID_ARG: a rate of 0, null coeffs. */
int  aacg_loudness_design(uint32_t rate, float coeffs[2][5]);
/* Host code only, in double: gated loudness of one stream's records ([n_hops][channels][2] floats as the meter emits them; only e is
 * read).  Blocks are four consecutive hops, advancing one hop at a time, n_hops - 3 of them (none with fewer than four hops):
 * z = sum over c of w_c (sum of e_c over the four) / (4 hop), l = -0.691 + 10 log10 z (-inf for z = 0).  The absolute gate keeps the
 * blocks with l > -70; the relative gate lies 10 LU below -0.691 + 10 log10(mean z of those).  *integrated_lufs = -0.691 + 10 log10
 * of the mean z over the blocks above both gates, or -inf if there are none.  Null weights: all 1 (BS.1770 gives the surround channels
 * 1.41 and leaves the LFE out: 0).  momentary_lufs, if not null, receives l of every block (with hop = rate / 10: the 400 ms momentary
 * loudness every 100 ms).  AACG_ERR_INVALID_ARG: null records with hops, a null integrated_lufs, channels outside 1..8, a hop outside 1..2^20. */
int  aacg_loudness_integrate(const float* records, size_t n_hops, uint32_t channels, uint32_t hop, const double* weights,
                             double* integrated_lufs, double* momentary_lufs);
/* True peak on the device, the third member of the R 128 triplet beside the meter's energy and sample peak: the largest magnitude of
 * the signal OVERSAMPLED by a polyphase FIR, one float per hop and channel, for a consumer whose ceiling is stated in dBTP.  It is set on
 * a pipeline that already has a meter (aacg_pipeline_set_loudness) and shares the meter's input, hop, counts and clock.
 *     phases L: 1..8;  taps T: a multiple of 4 in 4..64;  table: h[L][T], row-major float32, every entry finite (aacg_true_peak_design
 *     makes the usual one).
 * The input x of channel c of a slot is exactly the meter's: the sample the transform delivers, BEFORE the mix, the limiter, the
 * resampler and the feature stage, in all `channels` channels by position; on an AACG_OUTPUT_I16 pipeline the already rounded int16
 * times 2^-15 (exact); a refused frame and a frame of an unlearnt stream are 1024 zeros that advance the clock; x[j] = 0 for j < 0 since
 * the slot's reset.
 * THE RULE, bit for bit, in float32 throughout.  For input index i and phase p = 0 .. L-1,
 *     acc = h[p][0] * x[i]                             (rounded to float)
 *     acc = acc + (h[p][t] * x[i - t])   t = 1 .. T-1   (the product rounded, then the sum rounded: NOT fused, in this order)
 * every term computed whatever its coefficient, subnormals kept: aacg_pipeline_set_resample's rule with M = 1.  tp of hop k is the
 * largest |acc| over i in [k hop, (k + 1) hop) and all L phases — a NaN if any of those acc is a NaN (which NaN is not defined).  A
 * maximum does not depend on order, so nothing in the result depends on how the device splits the work.  numpy float32 arithmetic
 * reproduces the result exactly.
 * One float per hop and channel leaves whenever the meter emits a record: the same counts (aacg_pipeline_loudness_counts), the same
 * clock, hop `hop` of the meter.  Any split of a stream's frames into batches gives the same bits.  A reset (aacg_pipeline_reset_stream)
 * zeroes the history and the partial maximum.
 * The filter is causal: a hop's tp sees the signal (L T - 1) / (2 L) samples LATE, the group delay of a linear-phase table, so a peak
 * in a hop's last samples is reported by the next hop.  Phase 0 is NOT the identity — a designed table has no phase that passes the
 * samples through — so tp may lie a little below the hop's sample peak where a sample sits on a crest: a consumer takes
 * max(peak, tp) of the meter's record and this one.
 * Records of a submission: packed [stream s][n_out[s]][channels] float32, n_out the meter's count, in HOST memory that the caller names
 * with aacg_pipeline_true_peak_out before every submission; they are there when the submission's ticket has been collected.
 * State per slot: the last T - 1 input samples and the partial maximum per channel on the device, handed from batch to batch across
 * lanes as the resampler's history.  One more launch per batch (aacg_pcm_truepeak_*) on the lane's stream beside the meter's, in front
 * of it a clear of the batch's records; it goes with everything the meter goes with.  With no true-peak stage set nothing differs, call
 * for call.
 * Called once, before the pipeline's first submitted batch, on a pipeline with a meter.  AACG_ERR_INVALID_ARG, with the reason in
 * aacg_pipeline_last_error and the pipeline exactly as it was: no meter, a null config or table, phases or taps outside the limits, an
 * entry that is not finite, a call after the first batch, a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the table, the
 * slots' state and the lanes' records; the pipeline stays as it was.
 * Not here: short-term windows, a metered true peak behind the mix or the limiter (the limiter's own detector is
 * aacg_pipeline_set_limiter_true_peak, below), a table of more than 8 phases. */
typedef struct aacg_true_peak_config {
    uint32_t phases;         /* L */
    uint32_t taps;           /* T */
    const float* table;      /* [phases][taps] */
} aacg_true_peak_config;
int  aacg_pipeline_set_true_peak(aacg_pipeline* p, const aacg_true_peak_config* cfg);
/* Where the NEXT enqueued submission's true-peak records go: `peaks`, host memory with room for capacity_floats floats, valid until
 * that submission's ticket has been collected (the records are written at the collect).  One call arms one submission, as
 * aacg_pipeline_loudness_out does for the meter's.  A submission on a pipeline with the stage and no destination named is refused with
 * AACG_ERR_INVALID_ARG, one whose destination is smaller than the sum of n_out[s] x channels floats with AACG_ERR_CAPACITY — behind the
 * meter's own two refusals, which come first: nothing is enqueued, no ticket is taken, no clock moves, and both destinations stay
 * armed.  AACG_ERR_INVALID_ARG: a pipeline without the stage, null peaks with a capacity above 0. */
int  aacg_pipeline_true_peak_out(aacg_pipeline* p, float* peaks, size_t capacity_floats);
/* The project's default table for aacg_pipeline_set_true_peak, host code only: float for float the table that
 * aacg_resample_design(1, phases, taps, rolloff, beta, ...) writes — a Kaiser-windowed sinc with its cutoff at rolloff x the input's
 * Nyquist, every phase row of sum 1 — with the same defaults for 0 (rolloff 0.95, beta 9) and the same refusals, and phases and taps
 * within aacg_pipeline_set_true_peak's limits.  `table` has room for `capacity` floats, at least phases x taps.  Four phases of 24 taps
 * with beta 5 read a sine of any frequency up to 20 kHz at 48 kHz within +0.2 / -0.4 dB (EBU Tech 3341's tolerance). */
int  aacg_true_peak_design(uint32_t phases, uint32_t taps, double rolloff, double beta, float* table, size_t capacity);

/* A gain per stream and a look-ahead limiter on the device: a STAGE of the way out, BEHIND the mix and IN FRONT of the resampler and the
 * feature stage, for a consumer that has a gain for a stream (from the meter above, from ReplayGain tags) and wants it applied, with
 * full scale protected, before the PCM leaves — a 5.1 -> stereo mix without `normalise` exceeds full scale on ordinary material, and on
 * a float pipeline nothing else catches that.  The same gain goes to every channel of a stream (the limiter is channel-linked).
 *     ceiling c: finite and above 0, in full-scale units for both output kinds;  release r: in (0, 1];
 *     per slot a gain G (aacg_pipeline_set_gain): finite, 0 <= G <= 1024, 1 until it is set.
 * The input x of a slot is its PCM as the pipeline would have delivered it without the stage, after the mix if one is set: Oc =
 * out_channels or `channels` channels, at the stream's own rate, so every stream brings a multiple of 1024 samples.  Blocks are
 * AACG_LIMIT_BLOCK = 64 samples x Oc channels and never straddle a frame.  A refused frame and a frame of an unlearnt stream are zeros
 * and pass through like any other.  On an AACG_OUTPUT_I16 pipeline x is the already rounded int16 times 2^-15 (exact).
 * THE RULE, bit for bit, in float32 throughout, every operation rounded on its own, nothing fused, subnormals kept.  Per slot the stage
 * holds one block xh, the node gain a0 at its start and the block's target th.  For every arriving block xk of the slot, in order:
 *     p  = max over the block's 64 x Oc samples of |x|      (fmaxf from +0: a NaN sample is ignored here)
 *     tk = (G p > c) ? c / p : G                            (the product rounded, then compared)
 *     u  = a0 + (r (G - a0))
 *     a1 = fminf(fminf(th, tk), u)
 *     d  = a1 - a0
 *     out[i][ch] = (a0 + (d w[i])) xh[i][ch]                i = 0..63, w[i] = i / 64 (exact)
 *     xh = xk;  a0 = a1;  th = tk
 * AACG_OUTPUT_F32: out as computed, no clamp.  AACG_OUTPUT_I16: out x 2^15 rounded to nearest even and saturated, the mix's int16 rule.
 * A fresh slot (create, aacg_pipeline_reset_stream) holds a block of zeros, with a0 = th = G as G stands at the slot's next batch.  A
 * batch emits exactly as many samples as it brings, delayed by 64: the last 64 samples of a stream stay inside, as the resampler's
 * group delay keeps its share, and there is no flush.  Any split of a stream's frames into batches gives the same bits.
 * What follows from the rule: (a) for finite input |out| <= c (1 + 2^-21) — the gain inside a block lies between its two nodes, both
 * are <= th <= c / p, and four roundings of 2^-24 each lie between the exact bound and the stored sample; (b) a fall of G, or a peak
 * that arrives, reaches the output within one block, as a linear ramp; (c) a rise approaches G at the rate r per block;  (d) a limiter
 * behind an int16 transform or mix cannot undo THEIR saturation: it serves a boost there, not a rescue.
 * State per slot: G on the host; xh, a0 and th on the device, handed from batch to batch across lanes as the resampler's history.  One
 * more launch per batch (aacg_pcm_limit_*) on the lane's stream behind the mix; it goes with both output kinds, every `stages` bit, both
 * plan modes, ragged, device and host batches, span walks, the mix, the resampler, the feature stage and the meter — which taps the
 * transform's PCM in front of all this and does not see it.  aacg_pipeline_out_samples and every buffer size keep their values: the
 * stage emits what it receives.  With no limiter set nothing differs, call for call.
 * Called once, before the pipeline's first submitted batch, and after aacg_pipeline_set_mix if both are used (a mix set behind it is
 * refused); its order relative to _set_resample, _set_features and _set_loudness is free.  AACG_ERR_INVALID_ARG, with the reason in
 * aacg_pipeline_last_error and the pipeline exactly as it was: a null config, a ceiling or release outside the limits, a call after
 * the first batch, a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the slots' state and the lanes' buffer; the pipeline
 * stays as it was.
 * A true-peak (oversampled) ceiling: aacg_pipeline_set_limiter_true_peak, below.  Not here: a limiter behind the resampler, a flush of
 * the last 64 samples. */
#define AACG_LIMIT_BLOCK 64
typedef struct aacg_limiter_config {
    float ceiling;
    float release;
} aacg_limiter_config;
int  aacg_pipeline_set_limiter(aacg_pipeline* p, const aacg_limiter_config* cfg);
/* A slot's gain G.  May be called at any time on a pipeline with a limiter; it takes effect with the next batch ENQUEUED that holds the
 * slot and does not wait for batches in flight (the gain travels with the launch).  It survives aacg_pipeline_reset_stream: it is the
 * caller's setting, not the stream's state.  AACG_ERR_INVALID_ARG: a pipeline without a limiter, a slot out of range, a gain that is
 * not finite or outside 0..1024. */
int  aacg_pipeline_set_gain(aacg_pipeline* p, uint32_t slot, float gain);
/* ... and reads it back.  AACG_ERR_INVALID_ARG: a pipeline without a limiter, a slot out of range, a null gain. */
int  aacg_pipeline_gain(const aacg_pipeline* p, uint32_t slot, float* gain);
/* Host code only, in double, each value rounded to float once: ceiling = 10^(ceiling_db / 20), release = 1 - exp(-64 / (rate x
 * release_ms / 1000)) — the share of the way back to G that a block of 64 samples covers at a time constant of release_ms.
 * AACG_ERR_INVALID_ARG: a rate of 0, a null cfg, a result outside aacg_pipeline_set_limiter's limits. */
int  aacg_limiter_design(uint32_t rate, double ceiling_db, double release_ms, aacg_limiter_config* cfg);
/* A TRUE-PEAK ceiling for the limiter: a detector in front of its recurrence, for a consumer whose delivery specification states the
 * ceiling in dBTP — the plain limiter holds a sample-peak ceiling, and a sine at fs / 4 whose samples are 0.707 passes it with a true
 * peak of 1.  It takes aacg_pipeline_set_true_peak's configuration and limits:
 *     phases L: 1..8;  taps T: a multiple of 4 in 4..64;  table: h[L][T], row-major float32, every entry finite (aacg_true_peak_design
 *     makes the usual one).
 * THE RULE, bit for bit, in float32 throughout, every operation rounded on its own, nothing fused, subnormals kept.  x[j] is the slot's
 * limiter input since its reset as aacg_pipeline_set_limiter defines it (after the mix, Oc channels, int16 as the sample times 2^-15),
 * x[j] = 0 for j < 0.  D = T / 2, and z[j] = x[j - D] is the audio path: x delayed by the detector's group delay rounded up.  For block
 * k, the indices j = 64 k .. 64 k + 63:
 *     ps = max over the block's 64 x Oc samples of |z[j][ch]|
 *     acc_ph[j][ch] = h[ph][0] * x[j][ch]                                      (rounded to float)
 *     acc_ph[j][ch] = acc_ph[j][ch] + (h[ph][t] * x[j - t][ch])   t = 1 .. T-1  (the product rounded, then the sum rounded, in this order)
 *     pt = max over the block's 64 x L x Oc values of |acc_ph[j][ch]|           (aacg_pipeline_set_true_peak's accumulation, on x)
 *     p  = fmaxf(ps, pt)
 * every maximum an fmaxf from +0 in which a NaN is ignored, as the plain rule ignores a NaN sample.  Then the limiter's rule unchanged
 * with xk := block k of z and this p: tk, u, a1, the ramp, xh = xk; a0 = a1; th = tk.  A maximum does not depend on order, so nothing in
 * the result depends on how the device splits the work.  numpy float32 arithmetic reproduces the result exactly.
 * What follows from the rule.  A batch emits exactly as many samples as it brings, delayed by 64 + T / 2 (aacg_pipeline_limiter_delay);
 * buffer sizes, aacg_pipeline_out_samples and every copy keep their values.  Any split of a stream's frames into batches gives the same
 * bits.  A fresh slot (create, aacg_pipeline_reset_stream) holds zeros for the held block and for the T - 1 samples of history, with
 * a0 = th = G.  Since p >= ps, guarantee (a) of the plain limiter holds: |out| <= c (1 + 2^-21) for finite input.  The detector at block k
 * covers the signal times [64 k - D + 1 / (2 L), 64 k + 63 - D + 1), which lie inside the span of the audio block it governs, so both node
 * gains around a held block are <= c / p of that block, as before.  The TRUE-PEAK bound is NOT exact: while the gain moves inside the
 * filter's window the delivered signal is not a scaled copy of the measured one.  With a gain at rest the delivered true peak, read with
 * the detector's own table, is <= c (1 + 2^-20); under a moving gain it has been measured a little above c (DESIGN.md section 8 has the
 * figures), and a reading with another table differs by what the two tables differ.
 * State per slot: the plain limiter's, and the last T - 1 input samples per channel, on the device, handed from batch to batch across
 * lanes alike.  Two launches per batch (aacg_pcm_limit_tp_detect_*, aacg_pcm_limit_tp_*) on the lane's stream in the place of the plain
 * limiter's one, and per lane a scratch of one float per block of 64; it goes with everything the limiter goes with.  The meter's
 * true-peak stage (aacg_pipeline_set_true_peak) is independent of it: that one taps the transform's PCM, this one sits in the chain.
 * With the call unused nothing differs, call for call.
 * Called once, on a pipeline that has a limiter, before the first submitted batch and in front of aacg_pipeline_set_trim, like the
 * limiter; its order relative to _set_resample, _set_features, _set_loudness and _set_true_peak is free.  AACG_ERR_INVALID_ARG, with the
 * reason in aacg_pipeline_last_error and the pipeline exactly as it was: no limiter, a null config or table, phases or taps outside the
 * limits, an entry that is not finite, a call after the first batch, a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the
 * table, the slots' state or the lanes' scratch; the pipeline keeps its plain limiter.
 * Not here: an exact dBTP bound under a moving gain, a table of more than 8 phases, a limiter behind the resampler, a flush of the held
 * samples. */
int  aacg_pipeline_set_limiter_true_peak(aacg_pipeline* p, const aacg_true_peak_config* cfg);
/* The limiter's delay in samples per channel: AACG_LIMIT_BLOCK = 64, or 64 + T / 2 with the detector (what aacg_trim_design_delay
 * takes).  AACG_ERR_INVALID_ARG: a pipeline without a limiter, a null pointer. */
int  aacg_pipeline_limiter_delay(const aacg_pipeline* p, uint32_t* samples);

/* ---- the resident route: refused frames concealed ----------------------------------------------------------------------------------
 * An optional stage in front of the transform: a frame the parser or the refresh refused repeats its stream's last good frame, fading
 * fade_steps scalefactor steps (1.5 dB each) per lost frame, for at most hold_frames frames in a row; then silence as before.  THE RULE
 * is aacg_plan_conceal_refused's, above: G and r per stream slot, empty / 0 at create and after aacg_pipeline_reset_stream — which
 * takes effect with the slot's next batch, as the resampler's and the limiter's histories are reset.  One more launch per batch
 * (aacg_units_conceal) on the lane's stream behind the refresh and in front of the window-shape carry: the shape carried behind a
 * concealed frame is G's.  A concealed frame's result keeps its status, n_units and bits_used and gains AACG_PARSE_CONCEALED in
 * `flags`; *n_refused counts it as ever.  A stream without a learnt layout is not touched; a submission refused before anything is
 * enqueued changes no state.  With no concealment set nothing differs, call for call.
 * It goes with AACG_PIPELINE_STAGE_WINDOW_SHAPE, both output kinds, every delivery (host, device packed or planar) and every exit
 * stage (mix, limiter, resampler, features, meter, true peak), which see the concealed PCM.
 * Called once, before the pipeline's first submitted batch.  AACG_ERR_UNSUPPORTED, with the reason in aacg_pipeline_last_error and the
 * pipeline exactly as it was: plan_mode 0 (its retry of a stale plan would run the stage twice for one batch; plan_mode 1's shaped
 * set is never stale), AACG_PIPELINE_STAGE_TNS or AACG_PIPELINE_STAGE_PNS (the TNS records of a repeated frame and repeated noise
 * bands are not served).  AACG_ERR_INVALID_ARG: a null config, fade_steps above 64, hold_frames outside 1..255, a call after the
 * first batch, a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the slots' state. */
typedef struct aacg_conceal_config {
    uint32_t fade_steps;       /* 0..64 scalefactor steps per lost frame; 2 is a usual value (3 dB a frame)  */
    uint32_t hold_frames;      /* 1..255 frames in a row that repeat G; 6 is a usual value (128 ms at 48 kHz) */
} aacg_conceal_config;
int  aacg_pipeline_set_concealment(aacg_pipeline* p, const aacg_conceal_config* cfg);
/* The frames concealed so far in batches that have been collected.  AACG_ERR_INVALID_ARG: a null pipeline or count. */
int  aacg_pipeline_concealed(const aacg_pipeline* p, uint64_t* count);

/* ---- the resident route: trim, a skip and a length per stream ----------------------------------------------------------------------
 * Every AAC stream begins with samples that are not programme — the encoder's priming, 2112 samples commonly, 1024 otherwise — and
 * ends with padding up to a whole frame; containers say how much (MP4 edit lists, iTunSMPB, a server's index), and the CALLER knows it:
 * nothing here reads it from the bit stream.  A pipeline may carry a TRIM, the last PCM stage of the way out: behind the resampler (or
 * the limiter, the mix or the transform, whichever wrote last) and in front of the feature stage.  Only the kept samples cross the link.
 * THE RULE.  Each stream slot has a window (skip S, keep K) and a position Q, all three in samples per channel OF WHAT THE STAGE
 * RECEIVES — the outgoing rate, after the limiter's delay —, 64-bit, held on the host.  K = AACG_TRIM_ALL: no end; S and a finite K
 * are below 2^40.  A batch in which the slot's stream brings n_in samples (1024 x frames, or the resampler's n_out) keeps the received
 * samples with index q in [Q, Q + n_in) n [S, S + K): one contiguous range of n_keep samples, possibly none, copied bit for bit.  Q
 * advances by n_in when the batch has been enqueued; a refused or failed submission leaves it alone, like the resampler's clock.  A
 * refused frame, a concealed frame and a frame of an unlearnt stream count their samples like any other.  Any split of a stream's frames
 * into batches gives the same bits.  A pipeline with the stage and every window at its default (0, AACG_TRIM_ALL) delivers, bit for bit
 * and count for count, what it delivers without the stage; a pipeline without the stage differs in nothing, call for call.
 * Output layouts are the resampler's with n_keep[s] in the place of n_out[s]: host PCM and AACG_PCM_PACKED [stream s][n_keep[s]][O],
 * tight; AACG_PCM_PLANAR [stream][O][stride_frames x 1024] with the padding behind n_keep[s] written as zeros, every element of the block
 * written exactly once and nothing outside it — stride_frames in 1..2^21, stride_frames x 1024 at least every n_keep[s].  A stream may
 * emit nothing in a batch and a batch nothing at all (host and packed memory are then untouched, a planar block is zeros); results,
 * statuses, refusal counts and tickets are the untrimmed batch's.  aacg_pipeline_out_samples reports the trimmed counts — with a feature
 * stage the feature frames that follow from them: that stage then takes each stream's kept range as its input, its clock counts kept
 * samples only, and the trim launches nothing.  The meter and the true-peak stage tap the transform's PCM and do not see the trim.
 * One more launch per batch (aacg_pcm_trim_*) on the lane's stream, with no device state: nothing orders it behind the previous batch's.
 * Limit: max_streams x max_frames x 1024 (x L / M) below 2^31.  Device memory: every lane gets a buffer for a HOST batch's trimmed PCM, sized
 * for the largest untrimmed batch (max_streams x max_frames x 1024 (x L / M) x O elements) — device batches do not use it; it is not
 * made when a feature stage is set already, and stays when one is set afterwards.
 * aacg_pipeline_set_trim: cfg holds the window every slot starts with.  Called once, before the pipeline's first submitted batch and
 * after aacg_pipeline_set_mix, aacg_pipeline_set_limiter and aacg_pipeline_set_resample where those are used (they refuse behind it);
 * its order relative to aacg_pipeline_set_features, _set_loudness and _set_concealment is free.  AACG_ERR_INVALID_ARG, with the reason in
 * aacg_pipeline_last_error and the pipeline exactly as it was: a null config, a value outside the limits, a call after the first batch,
 * a second call.  AACG_ERR_OUT_OF_MEMORY: no device memory for the lanes' trimmed PCM; the pipeline stays as it was.
 * JavaScript: SharedEngine({ trim: true }) and decoder.setTrim(skip, length) (aac.js_amd/js/shared_engine.js).
 * Not here: windows of more than one segment, fades at the cuts, a flush of what the limiter and the resampler still hold at a stream's
 * end, a trim in the stream's own samples in front of those stages (aacg_trim_design converts instead). */
#define AACG_TRIM_ALL UINT64_MAX
typedef struct aacg_trim_config {
    uint64_t skip;             /* S of every slot until aacg_pipeline_set_stream_trim says otherwise */
    uint64_t keep;             /* K; AACG_TRIM_ALL: no end */
} aacg_trim_config;
int  aacg_pipeline_set_trim(aacg_pipeline* p, const aacg_trim_config* cfg);
/* A slot's window: sets (S, K) and Q = 0.  May be called at any time on a pipeline with a trim; it takes effect with the next batch
 * ENQUEUED that holds the slot and does not wait for batches in flight (a batch's ranges went up with its launch).
 * aacg_pipeline_reset_stream sets Q = 0 and LEAVES the window: it is the caller's setting, like a gain.  AACG_ERR_INVALID_ARG: a
 * pipeline without a trim, a slot out of range, a value outside the limits. */
int  aacg_pipeline_set_stream_trim(aacg_pipeline* p, uint32_t slot, uint64_t skip, uint64_t keep);
/* ... and reads the three back (any of the pointers may be null).  AACG_ERR_INVALID_ARG: a pipeline without a trim, a slot out of range. */
int  aacg_pipeline_stream_trim(const aacg_pipeline* p, uint32_t slot, uint64_t* skip, uint64_t* keep, uint64_t* position);
/* Host code only (no device, no pipeline): the share of the kept range that each of n consecutive pieces owns, by the rule above — piece
 * i brings n_in[i] samples, the first at `position`; it keeps kept_of[i] of them beginning at its first_of[i]-th (0 where it keeps
 * none).  With the frames of a batch as the pieces this is the per-frame slicing of the batch's kept PCM: the kept ranges lie one behind
 * the other in the output.  AACG_ERR_INVALID_ARG: a null pointer, skip or a finite keep at or above 2^40, a position that would wrap. */
int  aacg_trim_counts(uint64_t position, uint64_t skip, uint64_t keep, const uint32_t* n_in, uint32_t n, uint32_t* first_of, uint32_t* kept_of);
/* Host code only, exact integers: the window at the stage's input for a window (skip_in, keep_in) given in samples of the STREAM'S OWN
 * rate and time, with the route's latencies compensated — the limiter's AACG_LIMIT_BLOCK samples (limiter != 0) and a linear-phase
 * table's (L taps - 1) / (2 L) input samples.  With A(t) = 2 L t + 128 L limiter + L taps - 1:
 *     skip = ceil(A(skip_in) / 2M),   keep = ceil(A(skip_in + keep_in) / 2M) - skip   (AACG_TRIM_ALL stays AACG_TRIM_ALL),
 *     residual = skip - A(skip_in) / 2M = residual_num / residual_den, in [0, 1) output samples: how far behind the exact place of
 *     sample skip_in the first kept output sample lies (residual_num and residual_den may be null).
 * Without a resampler pass L = M = 1 and taps = 0; the filter term is then left out: skip = skip_in + 64 limiter, keep = keep_in.  A
 * caller-supplied table that is NOT linear-phase has whatever delay its designer gave it: compensate that by hand.
 * AACG_ERR_INVALID_ARG: a null skip or keep, L or M outside 1..1024, taps above 64, skip_in or a finite keep_in at or above 2^40, or a
 * result there. */
int  aacg_trim_design(uint64_t skip_in, uint64_t keep_in, int limiter, uint32_t L, uint32_t M, uint32_t taps, uint64_t* skip, uint64_t* keep,
                      uint64_t* residual_num, uint64_t* residual_den);
/* ... with the limiter's delay in samples (aacg_pipeline_limiter_delay: 64, or 64 + T / 2 with the true-peak detector; 0: no limiter) in
 * the place of 64 x limiter: A(t) = 2 L t + 2 L delay + L taps - 1, the rest unchanged.  delay = 64 gives exactly
 * aacg_trim_design(..., 1, ...), delay = 0 exactly (..., 0, ...).  The same refusals. */
int  aacg_trim_design_delay(uint64_t skip_in, uint64_t keep_in, uint32_t delay, uint32_t L, uint32_t M, uint32_t taps, uint64_t* skip, uint64_t* keep,
                            uint64_t* residual_num, uint64_t* residual_den);

#ifdef __cplusplus
}
#endif
#endif /* AACGPU_H */
