/*
 * aacg_pipeline.hip — bytes in, PCM out: the device front end and the transform behind ONE call per batch, several batches in
 * flight (aacg_pipeline_*, include/aacgpu.h).
 *
 * What a host of the reference does per frame and per stream in `readChunk()` (src/decoder.js:125-216: parse the
 * raw_data_block, process(elements), interleave), for a batch of streams at once and without the host in between: the frames'
 * bytes go up through page-locked staging, aacg_parse_device writes the unit records / spectra / band words in HBM,
 * aacg_plan_refresh_from_parse_ex turns them into a KEPT plan's unit records (the plan's run tables depend on which streams
 * bring how many frames of which elements, not on what the frames hold), aacg_decode_pipelined runs the transform, and the PCM
 * comes down into page-locked memory.  The host only finds the frame boundaries (ADTS frame_length) and says which stream slot
 * each run of frames belongs to.
 *
 * LANES.  A batch takes one of `lanes` sets of device buffers and a HIP stream of its own; aacg_pipeline_submit returns when the batch
 * is enqueued, aacg_pipeline_collect waits for it (bounded).  Batch k's PCM goes down while batch k + 1's bytes go up and are parsed;
 * the transform launches of consecutive batches go through aacg_decode_pipelined — the SAME plan continued launch after launch, its
 * unit records kept in one set per lane (aacg_plan_set_unit_sets) so that refreshing the next batch's records does not wait for the
 * launch that reads the previous ones — and so meet in the cross-launch rendezvous cells.  Why the bytes go up through a kernel, the
 * lanes' streams have the priorities they have and every lane has a parser of its own is measured and written where each is made:
 * at aacg_pipe_copy, in aacg_pipeline_create and at lane_t.
 *
 * BATCHES are ragged (aacg_pipeline_submit_ragged): each stream brings its own frame count, packed stream after stream; the rectangular
 * call is the case of equal counts.  Streams of up to eight channels: a stream's element layout (which SCE / CPE / LFE elements a frame
 * has, in order — decoder.js:233-247 deals channels out in element order and drops what exceeds chanConfig) is learnt from its first
 * frame (one small synchronous parse when a stream is new), the plan lists exactly those elements, and a later frame with other
 * elements is refused as a whole (AACG_PARSE_LAYOUT).
 *
 * Two PLAN MODES (aacg_pipeline_config.plan_mode).  0, kept plans: a plan per batch shape (plan_for), its refresh map expanded on the
 * lane's stream (aacg_pipe_map) from a per-stream table staged with the bytes, so a new shape costs the submit path no allocation and
 * no synchronous copy.  1, device plans: ONE plan with the pipeline's capacity made at create (aacg_plan_create_shaped), whose set of
 * the lane every batch shapes on the device — aacg_plan_shape_table completes the per-stream table in the staging,
 * aacg_plan_shape_launch runs the shaping kernel in the place of aacg_pipe_map — so a new shape costs no plan build, no upload of
 * O(units) bytes and no eviction either.  The modes part in choose_plan and in enqueue_front, nowhere else.
 *
 * STAGES (aacg_pipeline_config.stages), each independent of the others and of the plan mode.  AACG_PIPELINE_STAGE_TNS / _PNS: the
 * engine has AACG_TNS_SPEC / AACG_PNS_SPEC, the parser writes TNS side info into a buffer of the lane's, aacg_tns_records_from_parse
 * makes the batch's TNS records behind the parse, and the plans are plans for aacg_decode_pipelined_stages, which takes those records
 * as a launch input.  AACG_PIPELINE_STAGE_WINDOW_SHAPE: one launch of aacg_plan_carry_window_shape behind every refresh sets
 * window_shape_prev of the batch's unit records from the frame before and, across batches, from the engine's per-channel state.
 * aacg_pipeline_set_concealment (plan mode 1): one launch of aacg_plan_conceal_refused between the two replaces a refused frame's records by
 * its stream's last good frame, faded; the slots' state — that frame's records, two sides per slot — passes from batch to batch
 * like the resampler's history (SLOT STATE below).
 *
 * THE WAY OUT is a chain: transform -> mix (aacg_pipeline_set_mix: O = 1 or 2 channels leave in the place of C) -> limit
 * (aacg_pipeline_set_limiter: a gain per stream and a look-ahead limiter, sample for sample, state per slot like the resampler's) -> resample
 * (aacg_pipeline_set_resample: each stream's PCM leaves at L / M times the rate, a ragged count of samples per stream) -> features
 * (aacg_pipeline_set_features: one channel of PCM framed and transformed, float32 (log-)mel feature frames leave in its place) -> tail (the
 * planar launch for aacg_pipeline_submit_device with AACG_PCM_PLANAR, the copy down for a host batch, nothing for PCM left packed on
 * the device).  Which links a batch has, which buffer each reads and writes — a lane's, or the caller's in the place of the last — and
 * how many bytes is decided ONCE, in check_batch, by aacg_pipe::exit_plan (aacg_pipe_exit.h has the table, tests/test_pipe_exit_plan.py
 * pins it); enqueue_transform and enqueue_out walk that plan.  The two submissions share one body (submit_batch); the results' copy and
 * the lane's `done` event are the same whatever the way out, and aacg_pipeline_wait_device puts a consumer's stream behind that event.
 *
 * SLOT STATE, RECORDS, ORDER.  The resampler has state per slot — a clock, kept here modulo M, and on the device the last T - 1 samples
 * per channel, double-buffered — and so, each in its kind, have the feature stage, the meter with the true peak, the limiter and the
 * concealment; the trim has a position.  What the host keeps of it (aacg_pipe_slots.h, host-only, pinned by tests/test_pipe_slots.py;
 * a stage struct here derives from its slots and adds the device pointers), the batch's per-stream records made from it (check_batch:
 * build_*), their sections in the lane's one staging block behind the per-stream table (record_block) and the advance when the batch
 * has been enqueued, not before (enqueue_out: commit_*), are that header's.  Consecutive batches hand device state on ACROSS lanes:
 * ONE helper, ordered_launch, makes a launch wait for its stage's latest event unless it is this lane's — on the lane's stream behind
 * its parse and transform — records this lane's event behind it and makes that the latest (lane_t::ordered, aacg_pipeline::last, ORD_*).
 *
 * On a lane's stream, in this order: clear (unlearnt streams) -> copy up -> stale count -> parse -> TNS records -> map / shape ->
 * refresh -> conceal -> carry -> fork -> transform -> join -> mix -> wait / limit / record -> wait / resample / record -> wait / features / record -> planar or copy down -> results copy -> `done`.
 *
 * Host code apart from two small kernels (aacg_pipe_copy, aacg_pipe_map); it uses nothing but the public ABI of parser and engine
 * (and aacg_pipe_map.h / aacg_plan_shape.h / aacg_pcm_planar.h / aacg_pcm_mix.h / aacg_pcm_resample.h / aacg_pcm_features.h / aacg_pcm_limit.h for the tables it fills and the
 * side launches it makes).  DESIGN.md 7a has how it came to be this way, round by round.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/aacgpu.h"
#include "../../include/aacgpu_tools.h"
#include "aacg_pcm_mix.h"
#include "aacg_pcm_planar.h"
#include "aacg_pipe_slots.h"                              /* ... and with it aacg_pipe_exit.h and the PCM stages' limits and records, host only: the bodies are the engine's */
#define AACG_TRUEPEAK_HOST_ONLY
#include "aacg_pcm_truepeak.h"
#include "aacg_pcm_limit_tp.h"                            /* (host only too: both switches above are set) */
#include "aacg_plan_shape.h"
#include "aacg_wait.h"

#define AACG_PIPELINE_MAX_LANES 8
/* the bits of aacg_pipeline_config.stages that select the SPEC engine modes and the plans and launches that go with them
 * (AACG_PIPELINE_STAGE_WINDOW_SHAPE selects neither: one carry launch behind the refresh, whatever the plan) */
#define AACG_PIPELINE_SPEC_STAGES (AACG_PIPELINE_STAGE_TNS | AACG_PIPELINE_STAGE_PNS)

/* The side launches on a batch's PCM, each in aacg_engine_<stage>.hip with its kernels and described in aacg_pcm_<stage>.h: into a caller's
 * planar tensor, mixed to one or two channels, resampled by L / M, to (log-)mel feature frames, metered, gained and limited, its true
 * peak, cut to each stream's window.  false: not a launch the kernel serves (not_served) */
bool aacg_planar_launch(const aacg_planar_args& A, hipStream_t s);
bool aacg_mix_launch(const aacg_mix_args& A, hipStream_t s);
bool aacg_resample_launch(const aacg_resample_args& A, hipStream_t s);
bool aacg_features_launch(const aacg_features_args& A, hipStream_t s);
bool aacg_loudness_launch(const aacg_loudness_args& A, hipStream_t s);
bool aacg_limit_launch(const aacg_limit_args& A, hipStream_t s);
bool aacg_limit_tp_launch(const aacg_limit_tp_args& A, hipStream_t s);
bool aacg_truepeak_launch(const aacg_truepeak_args& A, hipStream_t s);
bool aacg_trim_launch(const aacg_trim_args& A, hipStream_t s);

/* The batch's bytes up (and its few kilobytes of results down) are moved by THIS kernel, not by hipMemcpyAsync: page-locked host
 * memory is mapped into the device's address space, and a few workgroups of 16-byte loads and stores move 1.4 MB in 30 us.  The
 * runtime's copies go through the two SDMA engines whatever their direction: in round 6's first build a lane's bytes waited up
 * to 0.6 ms behind another lane's PCM on its way down (kernel + copy trace, profiles/r06_resident_budget.txt), and the lanes ran
 * in lockstep pairs with the link idle a third of the time — 0.89-0.93 ms per batch.  A kernel on the lane's own stream waits
 * for nothing but its predecessor on that stream.  The PCM itself stays with the SDMA engines, ONE copy per batch: 0.64 ms per
 * batch (52 GB/s).  Measured against it: the PCM through this kernel too — 0.89, its PCIe-bound stores hold up the other
 * kernels' stores (the parse kernel then takes 1.0-1.4 ms instead of 0.55) — and the PCM as two SDMA halves on two streams —
 * 0.84-0.88, the halves of one batch take both engines and the next lane's copy waits behind them. */
extern "C" __global__ __launch_bounds__(256)
void aacg_pipe_copy(const uint4* src, uint4* dst, size_t n16, int clear_last)
{
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u* s = (const v4u*)src;
    v4u* d = (v4u*)dst;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        __builtin_nontemporal_store(__builtin_nontemporal_load(&s[i]), &d[i]);
        /* the results' copy: its last 16 bytes are the batch's refusal count, cleared for the lane's next batch by the lane that has
         * just read them (one launch less on the lane's stream than a memset in front of every batch) */
        if (clear_last && i == n16 - 1) { const v4u zero = {0u, 0u, 0u, 0u}; ((v4u*)src)[i] = zero; }
    }
}

/* A batch's refresh map from its per-stream table (aacg_pipe_map.h), on the lane's stream in front of the refresh that reads it:
 * a new batch shape costs the lane no device allocation and no synchronous copy. */
extern "C" __global__ __launch_bounds__(AACG_PIPE_MAP_THREADS)
void aacg_pipe_map(const aacg_pipe_stream* tab, uint32_t n_streams, uint32_t U, aacg_refresh_map* map)
{
    aacg_pipe::map_body(tab, n_streams, U, map, gridDim.x);
}

/* the stages whose slots' device state passes from batch to batch across lanes: their launches are ordered by events (ordered_launch);
 * the true peak stands inside the meter's */
enum { ORD_LIMIT, ORD_RESAMPLE, ORD_FEATURES, ORD_METER, ORD_STAGES };

struct aacg_pipeline {
    aacg_pipeline_config cfg;
    aacg_engine* engine = nullptr;
    aacg_parser* parser = nullptr;      /* layouts of new streams (synchronous, host pointers) */
    int n_lanes = 5;
    uint32_t C = 2;                     /* channels of a frame's PCM (chanConfig) */
    uint32_t O = 0;                     /* aacg_pipeline_set_mix: channels that leave (1 or 2); 0: no mix, C leave */
    float mix[AACG_MIX_MAX_OUT * AACG_MIX_MAX_IN] = {};      /* M[o][c] at mix[o * C + c] */
    /* The stages with state per slot: what the host keeps per slot — a clock or a position, and the two sides — and the settings the
     * batch's records follow from are the base (aacg_pipe_slots.h); here is what the launches need besides.
     * aacg_pipeline_set_resample: L / M and the table's taps (L = 0: no resampler), the table and the slots' histories on the device
     * ([slot][2][T - 1][channels out] floats) */
    struct resample_t : aacg_pipe::resample_slots {
        uint32_t T = 0;
        void *d_table = nullptr, *d_hist = nullptr;
        size_t lane_elems = 0;          /* the largest batch's output: elements of a lane's d_rs and h_pcm */
    } rs;
    /* aacg_pipeline_set_features: the stage's parameters (K = 0: none), its tables and the slots' histories on the device ([slot][2][K - 1] floats) */
    struct features_t : aacg_pipe::features_slots {
        uint32_t R = 0, n_mels = 0, log = 0;
        float floor = 0.0f;
        void *d_basis = nullptr, *d_fb = nullptr, *d_hist = nullptr;
        size_t lane_elems = 0;          /* the largest batch's output: floats of a lane's d_ft and h_pcm */
    } ft;
    /* aacg_pipeline_set_loudness: the meter's hop (0: none) and sections and the slots' state on the device ([slot][2][C][6] floats).
     * front16: the bytes IN FRONT of a lane's results (d_res, h_res) that take a batch's records, right-aligned, so that the results'
     * copy brings them down too (results_blocks).  out, out_cap, out_counts: the destination named for the next submission
     * (aacg_pipeline_loudness_out) while `armed` */
    struct loudness_t : aacg_pipe::loudness_slots {
        float coeffs[10] = {};
        void* d_state = nullptr; size_t front16 = 0;
        float* out = nullptr; size_t out_cap = 0; uint32_t* out_counts = nullptr; bool armed = false;
    } ld;
    /* aacg_pipeline_set_true_peak: the table's shape (L 0: none), the table and the slots' state on the device ([slot][2][T x C] words:
     * the history and the partial maximum).  The clock, the parities, the fresh flags, the records and the event are the meter's: the
     * launch stands between the meter's and the meter's event.  A batch's floats lie in front of the meter's records in the lane's
     * block (ld.front16 covers both).  out, out_cap: the destination named for the next submission (aacg_pipeline_true_peak_out) while
     * `armed` */
    struct truepeak_t {
        uint32_t L = 0, T = 0;
        void *d_table = nullptr, *d_state = nullptr;
        float* out = nullptr; size_t out_cap = 0; bool armed = false;
    } tp;
    /* aacg_pipeline_set_limiter: the two settings (on: a limiter is set) and the slots' state on the device ([slot][2][AACG_LIMIT_STATE(Oc)] floats).
     * aacg_pipeline_set_limiter_true_peak: the detector's table (tp_L 0: none) and the slots' histories beside that state
     * ([slot][2][(tp_T - 1) x Oc] floats), which follow the same parities and fresh flags */
    struct limiter_t : aacg_pipe::limiter_slots {
        float ceiling = 0.0f, release = 0.0f;
        void* d_state = nullptr;
        uint32_t tp_L = 0, tp_T = 0;
        void *d_tp_table = nullptr, *d_tp_hist = nullptr;
    } lim;
    /* aacg_pipeline_set_concealment: the two settings (on: the stage is set) and the slots' state on the device ([slot][2] sides,
     * aacg_conceal_state_bytes).  total: the concealed frames of collected batches */
    struct conceal_t : aacg_pipe::conceal_slots {
        uint32_t fade_steps = 0, hold_frames = 0;
        void* d_state = nullptr; uint64_t total = 0;
    } cn;
    /* aacg_pipeline_set_trim: all of it is the host's — the stage has no device state, a batch's kept ranges go up in its records */
    aacg_pipe::trim_slots tr;
    hipEvent_t last[ORD_STAGES] = {};   /* the event behind the latest launch of each ordered stage, whichever lane made it (ordered_launch) */
    uint32_t Cp = 2, U = 1;             /* what the parser is allowed per frame: channels (block stride), elements */
    bool learn = false;                 /* C > 2: layouts are learnt; C <= 2: every frame one SCE / one CPE */
    bool spec_stages = false;           /* cfg.stages has AACG_PIPELINE_STAGE_TNS or _PNS: SPEC engine modes, stages plans, aacg_decode_pipelined_stages */
    bool carry_shape = false;           /* cfg.stages has AACG_PIPELINE_STAGE_WINDOW_SHAPE: aacg_plan_carry_window_shape behind every refresh */
    /* a stream's element layout (aacg_pipe_map.h): channels of every SCE / LFE / CPE of a frame in order; kept = how many of them fit into C channels */
    typedef aacg_pipe_layout layout_t;
    std::vector<layout_t> layout;       /* per slot; n = 0: not learnt yet */
    /* kept plans, by batch shape: (the stream slots in order, each one's frame count); the layouts are the slots' */
    struct kept { std::vector<uint32_t> frames; std::vector<uint32_t> slots; aacg_plan* plan; uint64_t used; };
    std::vector<kept> plans;
    uint64_t tick = 0, plan_builds = 0;
    /* plan_mode 1 (aacg_pipeline_config): ONE plan with the pipeline's capacity, a set per lane, shaped on the device batch by batch
     * (aacg_plan_create_shaped) — `plans`, plan_for and the stale-plan retry are not on that path */
    aacg_plan* shaped = nullptr;
    uint64_t shaped_batches = 0, launches = 0;
    std::vector<layout_t> batch_layout; /* the submitting batch's streams' layouts, as its plan lists them */
    std::vector<uint32_t> rect_counts;  /* aacg_pipeline_submit's counts: every stream frames_per_stream */
    /* what a lane and a walk slot share: a parser and a stream of its own, and what says whether something is in flight on them */
    struct slot_t { aacg_parser* parser = nullptr; hipStream_t st = nullptr; hipEvent_t done = nullptr; bool busy = false; uint64_t ticket = 0; };
    struct lane_t : slot_t {
        /* A parser of its own per lane: a parser's launches are ordered one behind the other (they share its lane-order scratch),
         * and a batch's parse is the longest single step of the route — one GPU lane walks one frame's bits, so 4096 frames keep a
         * quarter of the chip busy for as long as the longest frame takes (0.5-0.8 ms; profiles/r06_resident_budget.txt).  With a
         * parser per lane the parses of consecutive batches run side by side. */
        void *d_bytes = nullptr, *d_frames = nullptr, *d_units = nullptr, *d_q = nullptr, *d_meta = nullptr, *d_res = nullptr, *d_pcm = nullptr, *d_refused = nullptr;
        void* d_mix = nullptr;            /* aacg_pipeline_set_mix: the mixed PCM of a host or planar batch, max_streams x max_frames x 1024 x O elements */
        void* d_rs = nullptr;             /* aacg_pipeline_set_resample: the resampled PCM of a host batch, rs.lane_elems elements */
        void* d_ft = nullptr;             /* aacg_pipeline_set_features: the feature frames of a host batch, ft.lane_elems floats */
        void* d_lim = nullptr;            /* aacg_pipeline_set_limiter: the limited PCM wherever it is not a packed device batch's last stage, max_streams x max_frames x 1024 x Oc elements */
        void* d_lim_peak = nullptr;       /* aacg_pipeline_set_limiter_true_peak: the detector's float per block of 64, max_streams x max_frames x 16 floats */
        void* d_trim = nullptr;           /* aacg_pipeline_set_trim: the trimmed PCM of a host batch, the largest batch's untrimmed elements */
        hipEvent_t ordered[ORD_STAGES] = {};      /* the events behind this lane's latest launch of each ordered stage, made at create (ordered_launch) */
        float* ld_user = nullptr; size_t ld_bytes = 0;      /* ... and the batch in flight's records: where they go at collect, and how many bytes */
        float* tp_user = nullptr; size_t tp_bytes = 0;      /* aacg_pipeline_set_true_peak: the same for the batch in flight's true-peak floats */
        void* d_map = nullptr;            /* the batch's refresh map (aacg_pipe_map): max_streams x max_frames x U entries, made at create */
        /* aacg_pipeline_config.stages with AACG_PIPELINE_STAGE_TNS: the parser's TNS side info (max_streams x max_frames x Cp records)
         * and what aacg_tns_records_from_parse makes of it, the batch's records and their matrices — a launch input like d_q */
        void *d_tns_info = nullptr, *d_tns = nullptr;
        void *h_in = nullptr, *h_pcm = nullptr, *h_res = nullptr;
        size_t bytes_cap = 0;             /* of h_in and of d_bytes: they grow together (grow_pair) */
        /* the batch in flight */
        bool count_stale = false;
        void* collect_pcm = nullptr; size_t collect_bytes = 0;      /* the exit plan's collect part: h_pcm's bytes for the caller's pageable memory; 0: nothing to copy */
        aacg_parse_result* user_results = nullptr; uint32_t* user_refused = nullptr; uint32_t n = 0;
        struct span_t { uint32_t first, frames; };
        std::vector<span_t> unlearnt;     /* the packed frames of the batch's streams whose layout was not known: nothing of them was decoded */
    } lane[AACG_PIPELINE_MAX_LANES];
    uint64_t submitted = 0;
    /* span walks (aacg_pipeline_walk_submit): two slots, made at the first walk — a stream more at set-up would shift the
     * runtime's stream -> hardware queue assignment under the lanes' streams.  Bytes up and results down by aacg_pipe_copy through
     * page-locked staging, as a batch's; buffers grow, never shrink. */
    struct walk_t : slot_t {
        void *d_in = nullptr, *d_out = nullptr, *h_in = nullptr, *h_out = nullptr;
        size_t in_cap = 0, out_cap = 0;
        aacg_parse_frame* user_frames = nullptr; aacg_walk_result* user_results = nullptr;
        size_t frames_bytes = 0, results_bytes = 0, results_at = 0;
    } walk[2];
    uint64_t walks_submitted = 0;
    std::vector<aacg_code_entry> entries; uint32_t counts[12] = {};
    size_t res_cap16 = 0;               /* a lane's h_res: results of up to max_streams x max_frames frames, then (16-byte aligned) the refusal count */
    aacg_wait_policy wait;
    std::string err;
};

namespace {

bool ok(aacg_pipeline* p, hipError_t rc, const char* what)
{
    if (rc == hipSuccess) return true;
    p->err = std::string(what) + ": " + hipGetErrorString(rc);
    return false;
}
int engine_fail(aacg_pipeline* p, const char* what, int rc) { p->err = std::string(what) + aacg_last_error(p->engine); return rc; }
#define P_TRY(p, call, code) do { if (!ok((p), (call), #call)) return (code); } while (0)

size_t pcm_elem(const aacg_pipeline* p) { return p->cfg.output_kind == AACG_OUTPUT_I16 ? 2 : 4; }
/* the channels of the PCM that leaves: the mix's rows, or the transform's channels */
uint32_t out_channels(const aacg_pipeline* p) { return p->O ? p->O : p->C; }
/* what the pipeline is, for aacg_pipe::exit_plan and what goes with it (aacg_pipe_exit.h) */
aacg_exit_pipe exit_pipe(const aacg_pipeline* p)
{
    return {p->C, p->O, p->rs.L != 0, (uint32_t)pcm_elem(p), (uint32_t)p->cfg.max_streams, (uint32_t)p->cfg.max_frames, p->rs.lane_elems,
            p->ft.K ? p->ft.n_mels : 0u, p->ft.lane_elems, p->lim.on ? 1u : 0u, p->tr.on ? 1u : 0u};
}
/* the most samples per channel a batch brings to a stage behind the resampler: what the kernels and their records count in 32 bits */
uint64_t most_samples(const aacg_pipeline* p)
{
    return p->rs.L ? aacg_pipe::exit_resample_most((uint32_t)p->cfg.max_streams, (uint32_t)p->cfg.max_frames, p->rs.L, p->rs.M)
                   : (uint64_t)p->cfg.max_streams * (uint64_t)p->cfg.max_frames * 1024u;
}
/* the most records per channel a batch brings the meter: every stream may complete a hop that earlier batches began */
uint64_t most_hops(const aacg_pipeline* p, uint32_t hop) { return (uint64_t)p->cfg.max_streams * ((uint64_t)p->cfg.max_frames * 1024u / hop + 1u); }

/* The refusals every aacg_pipeline_set_* begins with, in their order: no configuration, the stage is set already (`has`: "has a mix"), a
 * batch has been submitted, a stage is set that `what` ("the mix") must be set before.  Every refusal leaves the pipeline exactly as it was */
struct set_before { bool set; const char* has; };
int refuse_set(aacg_pipeline* p, const char* fn, bool already, const char* has, const char* what, std::initializer_list<set_before> before = {}, bool no_cfg = false)
{
    std::string no = no_cfg ? "no configuration" : already ? std::string("the pipeline ") + has + " already" : p->submitted ? std::string("a batch has been submitted (") + what + " is set before the first)" : "";
    for (const auto& b : before) if (b.set && no.empty()) no = std::string("the pipeline has ") + b.has + " already (" + what + " is set before it)";
    if (!no.empty()) p->err = std::string(fn) + ": " + no;
    return no.empty() ? AACG_OK : AACG_ERR_INVALID_ARG;
}
/* the first entry of a caller's table that is not finite, as a refusal: "<what> <i><of> is not finite"; false: every entry is */
bool not_finite(aacg_pipeline* p, const float* v, size_t n, const char* what, const char* of)
{
    for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) { p->err = what + std::to_string(i) + of + " is not finite"; return true; }
    return false;
}

/* a slot's layout as plans and callers see it: the learnt one (n = 0: none yet), or, C <= 2, one element of C channels */
aacg_pipeline::layout_t layout_of(const aacg_pipeline* p, uint32_t slot)
{
    aacg_pipeline::layout_t lay = p->layout[slot];
    if (!p->learn) { lay.n = lay.kept = 1; lay.nch[0] = (uint8_t)p->C; }
    return lay;
}

/* true if the runtime knows this host pointer as page-locked (aacg_host_alloc / hipHostMalloc / hipHostRegister) */
bool is_pinned(const void* ptr)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

/* bytes (a multiple of 16, both ends 16-byte aligned) between device memory and mapped page-locked host memory, on stream s */
void pipe_copy(const void* src, void* dst, size_t bytes, hipStream_t s, bool clear_last = false)
{
    const size_t n16 = bytes / 16;
    if (!n16) return;
    const unsigned blocks = (unsigned)((n16 + 255) / 256 < 64 ? (n16 + 255) / 256 : 64);      /* 64 x 256 lanes x 16 bytes in flight: the link, not the chip */
    hipLaunchKernelGGL(aacg_pipe_copy, dim3(blocks), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, n16, clear_last ? 1 : 0);
}

/* page-locked and device buffers of at least `need` bytes (grown by half again: a steady state allocates nothing) */
int grow_pair(aacg_pipeline* p, void** h, void** d, size_t* cap, size_t need)
{
    if (need <= *cap) return AACG_OK;
    if (*h) (void)hipHostFree(*h);
    if (*d) (void)hipFree(*d);
    *h = *d = nullptr; *cap = 0;
    const size_t want = need * 3 / 2 + 4096;
    P_TRY(p, hipHostMalloc(h, want, hipHostMallocDefault), AACG_ERR_OUT_OF_MEMORY);
    P_TRY(p, hipMalloc(d, want), AACG_ERR_OUT_OF_MEMORY);
    *cap = want;
    return AACG_OK;
}

/* The buffers a lane gets after create (aacg_pipeline_set_mix, aacg_pipeline_set_resample): `bytes` of device memory at lane_t::*buf
 * for EVERY lane — or for none: false leaves the lanes as they were */
typedef aacg_pipeline::lane_t lane_t;
void lanes_release(aacg_pipeline* p, void* lane_t::*buf)
{
    for (auto& L : p->lane) if (L.*buf) { (void)hipFree(L.*buf); L.*buf = nullptr; }
}
bool lanes_alloc(aacg_pipeline* p, void* lane_t::*buf, size_t bytes)
{
    for (int k = 0; k < p->n_lanes; k++)
        if (hipMalloc(&(p->lane[k].*buf), bytes) != hipSuccess) { (void)hipGetLastError(); lanes_release(p, buf); return false; }
    return true;
}
/* A set-up's allocations did not all succeed: what it made goes — device memory of its own, the lanes' buffers (buf; null: none) —
 * and the refusal is `what` */
int no_memory(aacg_pipeline* p, std::initializer_list<void*> made, void* lane_t::*buf, const char* what)
{
    (void)hipGetLastError();
    for (void* d : made) if (d) (void)hipFree(d);
    if (buf) lanes_release(p, buf);
    p->err = what;
    return AACG_ERR_OUT_OF_MEMORY;
}
/* Every lane's results block again with front16 bytes IN FRONT of the results for a meter's and a true peak's records, device and
 * page-locked, cleared — for every lane or for none: false leaves the lanes as they were.  Nothing is in flight yet */
bool results_blocks(aacg_pipeline* p, size_t front16)
{
    const size_t block = front16 + p->res_cap16 + 16;
    void *d_new[AACG_PIPELINE_MAX_LANES] = {}, *h_new[AACG_PIPELINE_MAX_LANES] = {};
    bool good = true;
    for (int k = 0; k < p->n_lanes && good; k++)
        good = hipMalloc(&d_new[k], block) == hipSuccess && hipMemset(d_new[k], 0, block) == hipSuccess && hipHostMalloc(&h_new[k], block, hipHostMallocDefault) == hipSuccess;
    for (int k = 0; k < p->n_lanes; k++) {
        auto& L = p->lane[k];
        if (!good) { if (d_new[k]) (void)hipFree(d_new[k]); if (h_new[k]) (void)hipHostFree(h_new[k]); continue; }
        (void)hipFree((char*)L.d_res - p->ld.front16); (void)hipHostFree((char*)L.h_res - p->ld.front16);      /* the old block, at its true base */
        L.d_res = (char*)d_new[k] + front16; L.h_res = (char*)h_new[k] + front16; L.d_refused = (char*)L.d_res + p->res_cap16;
        L.count_stale = false;                          /* (the new block's count is zero) */
    }
    if (good) p->ld.front16 = front16; else (void)hipGetLastError();
    return good;
}
/* A launch whose slots' device state passes from batch to batch while consecutive batches run on different streams: it waits for the
 * stage's latest, here — behind this lane's parse, transform and whatever of the way out lies in front, which need not wait — and this
 * lane's event behind it is the latest from now on.  launch(): AACG_OK, or the refusal with p->err set */
template <typename F>
int ordered_launch(aacg_pipeline* p, lane_t& L, int ord, F launch)
{
    if (p->last[ord] && p->last[ord] != L.ordered[ord]) P_TRY(p, hipStreamWaitEvent(L.st, p->last[ord], 0), AACG_ERR_NO_DEVICE);
    if (const int rc = launch()) return rc;
    P_TRY(p, hipEventRecord(L.ordered[ord], L.st), AACG_ERR_NO_DEVICE);
    p->last[ord] = L.ordered[ord];
    return AACG_OK;
}
int not_served(aacg_pipeline* p, const char* kernel) { p->err = std::string(kernel) + ": not a launch the kernel serves"; return AACG_ERR_INVALID_ARG; }
/* A lane's page-locked PCM staging is made lazily, at the size of the largest batch's output (aacg_pipe::exit_host_capacity).  What a
 * submission that failed half-way left behind has the size of before a mix or a resampler was set: it goes, and is made again */
void drop_host_staging(aacg_pipeline* p)
{
    for (int k = 0; k < p->n_lanes; k++) if (p->lane[k].h_pcm) { (void)hipHostFree(p->lane[k].h_pcm); p->lane[k].h_pcm = nullptr; }
}

/* A staging block, made and filled: the bytes (16-byte aligned, AACG_PARSE_PAD readable bytes behind them), the table of frames or
 * spans, and at extra_at (16-byte aligned again) room for what else goes up with them: a batch's per-stream table.  Page-locked
 * and device copy have one layout and one size, `up`. */
struct staging_t { size_t padded, extra_at, up; };
int stage(aacg_pipeline* p, void** h, void** d, size_t* cap, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* rows, uint32_t n_rows, size_t extra, staging_t& G)
{
    const size_t table = (size_t)n_rows * sizeof(aacg_parse_frame);
    G.padded = ((n_bytes + 15) & ~(size_t)15) + 64; G.extra_at = G.padded + ((table + 15) & ~(size_t)15); G.up = G.extra_at + extra;
    int rc = grow_pair(p, h, d, cap, G.up);
    if (rc) return rc;
    std::memcpy(*h, bytes, n_bytes);
    std::memset((char*)*h + n_bytes, 0, G.padded - n_bytes);
    std::memcpy((char*)*h + G.padded, rows, table);
    return AACG_OK;
}

/* One batch on its way through submit_batch: what the caller gave, then what each step leaves for the steps behind it */
typedef aacg_pipe::record_block RB;
struct batch_t {
    const uint8_t* bytes; size_t n_bytes; const aacg_parse_frame* frames; const uint32_t* slots; uint32_t n_streams; const uint32_t* frames_of;
    void* pcm_out; const aacg_pcm_device_out* dev; aacg_parse_result* results; uint32_t* n_refused;
    uint32_t n, longest;                         /* check_batch: the batch's frames, the largest count of a stream */
    uint32_t set;                                /* the lane's index: the set of a plan's unit records that is this lane's */
    aacg_exit_plan X;                            /* check_batch: the way out (aacg_pipe_exit.h) — which stage writes which buffer, and how many bytes */
    staging_t G;                                 /* stage_batch (the per-stream table lies at G.extra_at) */
    /* check_batch: the records of the stages that are set, from the slots' clocks, windows, gains and sides as they stand (aacg_pipe_slots.h:
     * build_*; the concealment's are sized there and made in choose_plan, from the plan's table) */
    std::vector<aacg_resample_stream> rs; std::vector<aacg_features_stream> ft; std::vector<aacg_loudness_stream> ld;
    std::vector<aacg_limit_stream> lim; std::vector<aacg_conceal_stream> cn; std::vector<aacg_trim_stream> tr;
    std::vector<uint32_t> tr_in;                 /* ... what each stream brings the trim: its slot's position advances by it in enqueue_out */
    uint32_t tr_items, ft_items;                 /* ... the trim's and the feature stage's launch items */
    size_t ld_floats, tp_floats;                 /* ... the floats the batch's loudness and true-peak records take, 0 without the stage */
    RB R;                                        /* stage_batch: where each stage's records lie in the staging block, behind the per-stream table */
    aacg_plan* plan;                             /* choose_plan: null when no stream of the batch has a layout yet */
};

/* a buffer of the exit plan, for this lane and this batch */
void* exit_buf(const aacg_pipeline::lane_t& L, const batch_t& B, uint8_t id)
{
    void* const of[] = {nullptr, L.d_pcm, L.d_mix, L.d_rs, L.h_pcm, B.dev ? B.dev->d_pcm : B.pcm_out, L.d_ft, L.d_lim, L.d_trim};      /* AACG_EXIT_BUF_NONE .. AACG_EXIT_LANE_TRIM */
    return of[id];
}

std::string lanes_text(aacg_pipeline* p)
{
    std::string o;
    char b[160];
    for (int k = 0; k < p->n_lanes; k++) {
        const auto& L = p->lane[k];
        hipError_t st = L.st ? hipStreamQuery(L.st) : hipSuccess;
        (void)hipGetLastError();
        std::snprintf(b, sizeof b, "%slane %d %s (ticket %llu, %s)", k ? ", " : "", k, st == hipSuccess ? "idle" : st == hipErrorNotReady ? "BUSY" : "error",
                      (unsigned long long)L.ticket, L.busy ? "not collected" : "collected");
        o += b;
    }
    return o;
}

int timed_out(aacg_pipeline* p, const char* what)
{
    char b[200], dump[3000] = "";
    std::snprintf(b, sizeof b, "%s: the GPU did not answer within %.1f s (aacg_pipeline_set_wait_limit_ms); %llu batches submitted; ", what, p->wait.limit_s, (unsigned long long)p->submitted);
    (void)aacg_debug_in_flight(p->engine, dump, sizeof dump);
    p->err = std::string(b) + lanes_text(p) + "; engine: " + dump;
    return AACG_ERR_TIMEOUT;
}

/* the bounded wait for what is in flight in a lane or a walk slot */
int wait_done(aacg_pipeline* p, aacg_pipeline::slot_t& S, const char* what)
{
    const hipError_t st = aacg_wait_event(S.done, p->wait);
    if (st == hipErrorNotReady) return timed_out(p, what);
    P_TRY(p, st, AACG_ERR_NO_DEVICE);
    return AACG_OK;
}

/* the lane's batch is complete: what it staged goes to the caller */
int finish_lane(aacg_pipeline* p, aacg_pipeline::lane_t& L)
{
    if (!L.busy) return AACG_OK;
    int rc = wait_done(p, L, "aacg_pipeline_collect");
    if (rc) return rc;
    if (L.collect_bytes) std::memcpy(L.collect_pcm, L.h_pcm, L.collect_bytes);
    if (L.ld_bytes) std::memcpy(L.ld_user, (const char*)L.h_res - ((L.ld_bytes + 15) & ~(size_t)15), L.ld_bytes);      /* the meter's records lie in front of the results */
    if (L.tp_bytes) std::memcpy(L.tp_user, (const char*)L.h_res - ((L.ld_bytes + 15) & ~(size_t)15) - ((L.tp_bytes + 15) & ~(size_t)15), L.tp_bytes);      /* ... and the true-peak floats in front of those */
    /* a stream whose first frame did not parse has no layout yet: every frame of it in this batch came out silent and says so */
    aacg_parse_result* res = (aacg_parse_result*)L.h_res;
    uint32_t* refused = (uint32_t*)((char*)L.h_res + p->res_cap16);
    for (const auto& u : L.unlearnt)
        for (uint32_t f = 0; f < u.frames; f++) { aacg_parse_result& r = res[(size_t)u.first + f]; if (r.status == AACG_PARSE_OK) r.status = AACG_PARSE_LAYOUT; (*refused)++; }
    if (p->cn.on) for (uint32_t i = 0; i < L.n; i++) p->cn.total += (res[i].flags & AACG_PARSE_CONCEALED) ? 1u : 0u;
    if (L.user_results) std::memcpy(L.user_results, res, (size_t)L.n * sizeof(aacg_parse_result));
    if (L.user_refused) std::memcpy(L.user_refused, refused, 4);
    L.busy = false;
    return AACG_OK;
}

/* the walk in a slot is complete: its results go to the caller */
int finish_walk(aacg_pipeline* p, aacg_pipeline::walk_t& W)
{
    if (!W.busy) return AACG_OK;
    int rc = wait_done(p, W, "aacg_pipeline_walk_collect");
    if (rc) return rc;
    std::memcpy(W.user_frames, W.h_out, W.frames_bytes);
    std::memcpy(W.user_results, (char*)W.h_out + W.results_at, W.results_bytes);
    W.busy = false;
    return AACG_OK;
}

/* ---- Plan mode 0, all of it: the kept plans by batch shape and their LRU, the plans a relearnt slot invalidates, the new plan for
 * a launch that found its own stale.  With plan mode 1 `plans` stays empty and choose_plan / enqueue_transform call none of this. ---- */
void drop_plan(aacg_pipeline* p, size_t i)
{
    aacg_plan_destroy(p->plans[i].plan);                 /* waits (bounded) for the launches that read it */
    p->plans.erase(p->plans.begin() + (long)i);
}
void drop_plans(aacg_pipeline* p) { while (!p->plans.empty()) drop_plan(p, p->plans.size() - 1); }
/* the plans that list this slot: made for a layout the slot no longer has, or while it had none (they list nothing of it) */
void drop_plans_with(aacg_pipeline* p, uint32_t slot)
{
    for (size_t i = p->plans.size(); i-- > 0;) {
        bool has = false;
        for (uint32_t s : p->plans[i].slots) has = has || s == slot;
        if (has) drop_plan(p, i);
    }
}

/* The plan for a batch of this shape: stream s brings frames_of[s] frames, parsed frames first_s .. first_s + frames_of[s] - 1
 * (aacg_pipe::plan_list: the units the plan lists; the map they are refreshed through is the lane's, aacg_pipe_map).  The
 * batch's layouts are in p->batch_layout. */
int plan_for(aacg_pipeline* p, const uint32_t* slots, const uint32_t* frames_of, uint32_t S, aacg_plan** out)
{
    for (auto& k : p->plans)
        if (k.slots.size() == S && std::memcmp(k.slots.data(), slots, S * sizeof(uint32_t)) == 0 &&
            std::memcmp(k.frames.data(), frames_of, S * sizeof(uint32_t)) == 0) { k.used = ++p->tick; *out = k.plan; return AACG_OK; }
    std::vector<aacg_unit_desc> u;
    uint32_t total = 0;
    for (uint32_t s = 0; s < S; s++) total += frames_of[s];
    u.reserve((size_t)total * (p->learn ? 4 : 1));
    aacg_pipe::plan_list(p->batch_layout.data(), slots, frames_of, S, p->C, p->Cp, p->U, &u, nullptr, nullptr);
    if (u.empty()) { *out = nullptr; return AACG_OK; }     /* no stream of the batch has a layout yet: nothing to transform, every frame is refused */
    aacg_plan* plan = nullptr;
    int rc = p->spec_stages ? aacg_plan_create_stages(p->engine, u.data(), (uint32_t)u.size(), &plan) : aacg_plan_create(p->engine, u.data(), (uint32_t)u.size(), &plan);
    if (rc == AACG_OK && (rc = aacg_plan_set_unit_sets(p->engine, plan, (uint32_t)p->n_lanes))) { aacg_plan_destroy(plan); plan = nullptr; }
    if (rc) return engine_fail(p, "aacg_plan_create: ", rc);
    p->plan_builds++;
    if (p->plans.size() >= 8) {                          /* the least recently used shape makes room */
        size_t lru = 0;
        for (size_t i = 1; i < p->plans.size(); i++) if (p->plans[i].used < p->plans[lru].used) lru = i;
        drop_plan(p, lru);
    }
    p->plans.push_back({std::vector<uint32_t>(frames_of, frames_of + S), std::vector<uint32_t>(slots, slots + S), plan, ++p->tick});
    *out = plan;
    return AACG_OK;
}

/* another shape's plan has advanced these streams since this one was used: plans are made from the engine's current state */
int replan_stale(aacg_pipeline* p, aacg_pipeline::lane_t& L, batch_t& B)
{
    drop_plans(p);
    int rc = plan_for(p, B.slots, B.frames_of, B.n_streams, &B.plan);
    if (rc == AACG_OK && B.plan) P_TRY(p, hipMemsetAsync(L.d_refused, 0, 16, L.st), AACG_ERR_NO_DEVICE);      /* the stale plan's refresh has counted this batch's refusals already */
    return rc;
}
/* ---- end of plan mode 0 ---- */

/* the element layouts of streams that are new: their first frames through one small synchronous parse (host pointers) */
int learn_layouts(aacg_pipeline* p, const uint8_t* bytes, const aacg_parse_frame* frames, const uint32_t* slots, uint32_t S, const uint32_t* frames_of)
{
    std::vector<uint32_t> who, first;
    for (uint32_t s = 0, i = 0; s < S; i += frames_of[s], s++) if (!p->layout[slots[s]].n) { who.push_back(s); first.push_back(i); }
    if (who.empty()) return AACG_OK;
    /* gather those frames' bytes (they lie anywhere in the caller's buffer) */
    std::vector<aacg_parse_frame> fr(who.size());
    std::vector<uint8_t> buf;
    for (size_t k = 0; k < who.size(); k++) {
        const aacg_parse_frame& f = frames[first[k]];
        fr[k].byte_offset = (uint32_t)buf.size(); fr[k].byte_length = f.byte_length;
        buf.insert(buf.end(), bytes + f.byte_offset, bytes + f.byte_offset + f.byte_length);
        buf.resize((buf.size() + 15) & ~(size_t)15);
    }
    const uint32_t n = (uint32_t)who.size(), U = p->U, Cp = p->Cp;
    std::vector<aacg_unit_desc> units((size_t)n * U);
    std::vector<int16_t> q((size_t)n * Cp * 1024);
    std::vector<aacg_band_meta> meta((size_t)n * Cp);
    std::vector<aacg_parse_result> res(n);
    int rc = aacg_parse_batch(p->parser, buf.data(), buf.size(), fr.data(), n, U, Cp, (uint32_t)p->cfg.parse_options, units.data(), q.data(), meta.data(), nullptr, res.data());
    if (rc) { p->err = std::string("learning the streams' element layouts: ") + aacg_parser_last_error(p->parser); return rc; }
    for (uint32_t k = 0; k < n; k++) {
        if (res[k].status != AACG_PARSE_OK || !res[k].n_units) continue;      /* not learnt: the stream's frames of this batch are refused, the next batch tries again */
        aacg_pipeline::layout_t lay;
        uint32_t chan = 0;
        lay.n = res[k].n_units > 8 ? 8 : res[k].n_units;
        for (uint32_t e = 0; e < lay.n; e++) {
            lay.nch[e] = units[(size_t)k * U + e].n_ch;
            if (chan + lay.nch[e] <= p->C && lay.kept == e) lay.kept = (uint8_t)(e + 1);   /* decoder.js:233: elements while channel < channels; one that would cross the end is not taken either */
            chan += lay.nch[e];
        }
        p->layout[slots[who[k]]] = lay;
        drop_plans_with(p, slots[who[k]]);                  /* plans made while this slot's layout was unknown list nothing of it */
    }
    return AACG_OK;
}

/* aacg_pipeline_submit_device's own refusals, all on the host, before anything is enqueued: what only the runtime can say about the
 * pointer, here, in its place among the rules that need no runtime (aacg_pipe::exit_check; b is what B.X was made from) */
int check_device_out(aacg_pipeline* p, const batch_t& B, const aacg_exit_batch& b)
{
    const aacg_pcm_device_out* out = B.dev;
    if (!out || !out->d_pcm) { p->err = "aacg_pipeline_submit_device: no device memory for the PCM (out or out->d_pcm is null)"; return AACG_ERR_INVALID_ARG; }
    const aacg_exit_refusal no = aacg_pipe::exit_check(exit_pipe(p), b, B.X, *out, aacg_planar_items(B.n_streams, out->stride_frames, (uint32_t)pcm_elem(p)));
    if (no.code && !no.late) { p->err = no.text; return no.code; }
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, out->d_pcm) != hipSuccess) { (void)hipGetLastError(); p->err = "aacg_pipeline_submit_device: d_pcm is not memory the HIP runtime knows (pageable host memory?)"; return AACG_ERR_INVALID_ARG; }
    if (a.type != hipMemoryTypeDevice || a.device != p->cfg.device_ordinal) {
        p->err = a.type == hipMemoryTypeDevice ? "aacg_pipeline_submit_device: d_pcm is another device's memory" : "aacg_pipeline_submit_device: d_pcm is not device memory (host memory, page-locked or not)";
        return AACG_ERR_INVALID_ARG;
    }
    if (no.code) p->err = no.text;
    return no.code;
}

}  // namespace

extern "C" {

const char* aacg_pipeline_last_error(const aacg_pipeline* p) { return p ? p->err.c_str() : "null pipeline"; }

void aacg_pipeline_destroy(aacg_pipeline* p)
{
    if (!p) return;
    (void)hipSetDevice(p->cfg.device_ordinal);
    bool answered = true;
    for (int k = 0; k < p->n_lanes && answered; k++) if (p->lane[k].st) answered = aacg_wait_stream(p->lane[k].st, p->wait) != hipErrorNotReady;
    (void)hipGetLastError();
    if (!answered) {
        /* a device that does not answer is not waited for again and nothing of it is freed (hipFree waits for the device) */
        std::fprintf(stderr, "aacgpu: aacg_pipeline_destroy: the GPU did not answer within the wait limit — the pipeline's device memory is left allocated\n");
        delete p;
        return;
    }
    drop_plans(p);
    if (p->shaped) aacg_plan_destroy(p->shaped);
    for (auto& W : p->walk) {
        if (W.st) (void)aacg_wait_stream(W.st, p->wait);
        for (void* d : {W.d_in, W.d_out}) if (d) (void)hipFree(d);
        for (void* h : {W.h_in, W.h_out}) if (h) (void)hipHostFree(h);
        if (W.done) (void)hipEventDestroy(W.done);
        if (W.parser) aacg_parser_destroy(W.parser);
        if (W.st) (void)hipStreamDestroy(W.st);
    }
    for (auto& L : p->lane) {
        /* (d_frames lies in d_bytes, d_refused in d_res; a meter's records lie in front of d_res and h_res, in their blocks) */
        for (void* d : {L.d_bytes, L.d_units, L.d_q, L.d_meta, L.d_res ? (void*)((char*)L.d_res - p->ld.front16) : nullptr, L.d_pcm, L.d_mix, L.d_rs, L.d_ft, L.d_lim, L.d_lim_peak, L.d_trim, L.d_map, L.d_tns_info, L.d_tns}) if (d) (void)hipFree(d);
        for (void* h : {L.h_in, L.h_pcm, L.h_res ? (void*)((char*)L.h_res - p->ld.front16) : nullptr}) if (h) (void)hipHostFree(h);
        if (L.done) (void)hipEventDestroy(L.done);
        for (hipEvent_t ev : L.ordered) if (ev) (void)hipEventDestroy(ev);
        if (L.parser) aacg_parser_destroy(L.parser);
    }
    for (void* d : {p->rs.d_table, p->rs.d_hist, p->ft.d_basis, p->ft.d_fb, p->ft.d_hist, p->ld.d_state, p->lim.d_state, p->lim.d_tp_table, p->lim.d_tp_hist, p->tp.d_table, p->tp.d_state, p->cn.d_state}) if (d) (void)hipFree(d);
    if (p->parser) aacg_parser_destroy(p->parser);
    if (p->engine) aacg_destroy(p->engine);
    for (auto& L : p->lane) if (L.st) (void)hipStreamDestroy(L.st);
    delete p;
}

int aacg_pipeline_create(const aacg_pipeline_config* cfg, const aacg_code_entry* entries, const uint32_t counts[12], aacg_pipeline** out)
{
    if (!cfg || !out || !entries || !counts) return AACG_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg->abi_version != AACG_ABI_VERSION || cfg->max_streams < 1 || cfg->max_frames < 1 || cfg->channels < 1 || cfg->channels > AACG_MAX_CHANNELS ||
        (cfg->output_kind != AACG_OUTPUT_F32 && cfg->output_kind != AACG_OUTPUT_I16) || (uint64_t)cfg->max_streams * (uint64_t)cfg->max_frames > (1u << 22) ||
        cfg->lanes < 0 || cfg->lanes > AACG_PIPELINE_MAX_LANES || cfg->plan_mode < 0 || cfg->plan_mode > 1 ||
        (cfg->stages & ~(AACG_PIPELINE_STAGE_TNS | AACG_PIPELINE_STAGE_PNS | AACG_PIPELINE_STAGE_WINDOW_SHAPE)) || cfg->reserved[0])
        return AACG_ERR_INVALID_ARG;
    if ((cfg->stages & AACG_PIPELINE_SPEC_STAGES) && cfg->output_kind == AACG_OUTPUT_I16) {
        std::fprintf(stderr, "aacgpu: aacg_pipeline_create: stages (AACG_TNS_SPEC / AACG_PNS_SPEC) need AACG_OUTPUT_F32 — with int16 PCM the stages are a spectral launch of "
                             "their own, which needs a spectrum buffer per plan and does not overlap\n");
        return AACG_ERR_UNSUPPORTED;
    }
    aacg_pipeline* p = new (std::nothrow) aacg_pipeline();
    if (!p) return AACG_ERR_OUT_OF_MEMORY;
    p->cfg = *cfg;
    p->spec_stages = (cfg->stages & AACG_PIPELINE_SPEC_STAGES) != 0;
    p->carry_shape = (cfg->stages & AACG_PIPELINE_STAGE_WINDOW_SHAPE) != 0;
    p->n_lanes = cfg->lanes ? cfg->lanes : 5;      /* four of the lowest priority and one of the level above: int16 PCM 0.37 -> 0.33 ms per batch, the link's rate; six and more share queues again */
    p->C = (uint32_t)cfg->channels;
    p->learn = p->C > 2;
    p->Cp = p->learn ? AACG_MAX_CHANNELS : p->C;
    p->U = p->learn ? 8u : 1u;
    p->layout.resize((size_t)cfg->max_streams);
    {   /* the codebooks again for the walk's parsers, made at the first walk */
        size_t n_entries = 0;
        for (int b = 0; b < 12; b++) { p->counts[b] = counts[b]; n_entries += counts[b]; }
        p->entries.assign(entries, entries + n_entries);
    }
    aacg_config ec;
    std::memset(&ec, 0, sizeof ec);
    ec.abi_version = AACG_ABI_VERSION; ec.device_ordinal = cfg->device_ordinal; ec.sample_index = cfg->sample_index;
    ec.max_streams = cfg->max_streams; ec.max_channels = cfg->channels; ec.input_kind = AACG_INPUT_QUANT_I16;
    ec.tns_mode = (cfg->stages & AACG_PIPELINE_STAGE_TNS) ? AACG_TNS_SPEC : AACG_TNS_REFERENCE;
    ec.pns_mode = (cfg->stages & AACG_PIPELINE_STAGE_PNS) ? AACG_PNS_SPEC : AACG_PNS_REFERENCE;
    ec.output_kind = cfg->output_kind; ec.cce_mode = AACG_CCE_REFERENCE;
    int rc = aacg_create(&ec, &p->engine);
    if (rc == AACG_OK) rc = aacg_parser_create(cfg->device_ordinal, cfg->sample_index, entries, counts, &p->parser);
    /* device plans: the one plan, made here — a failure (the in-launch cells of long chains are the large part) is the caller's to
     * see, there is no falling back to kept plans */
    if (rc == AACG_OK && cfg->plan_mode == 1 &&
        (rc = (p->spec_stages ? aacg_plan_create_shaped_stages : aacg_plan_create_shaped)(p->engine, (uint32_t)cfg->max_streams, (uint32_t)cfg->max_frames, p->U, (uint32_t)p->n_lanes, &p->shaped)))
        std::fprintf(stderr, "aacgpu: %s\n", aacg_last_error(p->engine));
    if (rc) { aacg_pipeline_destroy(p); return rc; }
    const size_t n = (size_t)cfg->max_streams * (size_t)cfg->max_frames, C = p->C, Cp = p->Cp, U = p->U;
    p->res_cap16 = (n * sizeof(aacg_parse_result) + 15) & ~(size_t)15;
    bool good = ok(p, hipSetDevice(cfg->device_ordinal), "hipSetDevice");
    /* The lanes' streams take the LOWEST priority: the runtime deals streams of one priority onto a handful of hardware queues
     * of their own, and two streams on one queue run one behind the other — a lane's parse behind another lane's copy down.
     * At the ordinary priority the lanes shared two queues with whatever else the process had made (kernel trace of round 6's first
     * build); at the lowest they are by themselves, and what competes with them for compute units — the transform launches on
     * the engine's highest-priority streams — is what should win. */
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    for (int k = 0; k < p->n_lanes && good; k++) {
        auto& L = p->lane[k];
        if (aacg_parser_create(cfg->device_ordinal, cfg->sample_index, entries, counts, &L.parser) != AACG_OK) { p->err = "aacg_parser_create (lane)"; good = false; break; }
        /* lanes 0..3 at the lowest priority, a level nobody else uses (four hardware queues); further lanes at the level between
         * that and the engine's pipeline streams: other queues again, so that a fifth lane does not wait behind the first */
        const int prio = k < 4 ? least : (least + greatest) / 2;
        good = ok(p, hipStreamCreateWithPriority(&L.st, hipStreamNonBlocking, prio), "hipStreamCreate") &&
               ok(p, hipEventCreateWithFlags(&L.done, hipEventDisableTiming), "hipEventCreate") &&               ok(p, hipMalloc(&L.d_units, n * U * sizeof(aacg_unit_desc)), "hipMalloc") &&
               ok(p, hipMalloc(&L.d_map, n * U * sizeof(aacg_refresh_map)), "hipMalloc") &&
               ok(p, hipMalloc(&L.d_q, n * Cp * 2048), "hipMalloc") && ok(p, hipMemsetAsync(L.d_q, 0, n * Cp * 2048, L.st), "hipMemset") &&
               ok(p, hipMalloc(&L.d_meta, n * Cp * sizeof(aacg_band_meta)), "hipMalloc") &&
               ok(p, hipMalloc(&L.d_res, p->res_cap16 + 16), "hipMalloc") &&      /* the refusal count lies behind the results: one copy brings both down */
               ok(p, hipMemsetAsync(L.d_res, 0, p->res_cap16 + 16, L.st), "hipMemset") &&
               ok(p, hipMalloc(&L.d_pcm, n * C * 1024 * pcm_elem(p)), "hipMalloc") &&
               (!(cfg->stages & AACG_PIPELINE_STAGE_TNS) ||
                (ok(p, hipMalloc(&L.d_tns_info, n * Cp * sizeof(aacg_tns_info)), "hipMalloc") &&
                 ok(p, hipMalloc(&L.d_tns, aacg_tns_records_bytes((uint32_t)(n * Cp))), "hipMalloc"))) &&
               ok(p, hipHostMalloc(&L.h_res, p->res_cap16 + 16, hipHostMallocDefault), "hipHostMalloc") &&
               aacg_wait_stream(L.st, p->wait) == hipSuccess;
        for (hipEvent_t& ev : L.ordered) good = good && ok(p, hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");      /* (a few per lane, whichever stages are set later) */
        if (good) L.d_refused = (char*)L.d_res + p->res_cap16;
    }
    if (!good) { if (p->err.empty()) p->err = "the pipeline's set-up did not complete"; std::fprintf(stderr, "aacgpu: %s\n", p->err.c_str()); aacg_pipeline_destroy(p); return AACG_ERR_OUT_OF_MEMORY; }
    *out = p;
    return AACG_OK;
}

int aacg_pipeline_set_wait_limit_ms(aacg_pipeline* p, uint32_t ms)
{
    if (!p || !ms) return AACG_ERR_INVALID_ARG;
    p->wait.limit_s = ms * 1e-3;
    (void)aacg_set_wait_limit_ms(p->engine, ms);
    (void)aacg_parser_set_wait_limit_ms(p->parser, ms);
    for (int k = 0; k < p->n_lanes; k++) (void)aacg_parser_set_wait_limit_ms(p->lane[k].parser, ms);
    for (auto& W : p->walk) if (W.parser) (void)aacg_parser_set_wait_limit_ms(W.parser, ms);
    return AACG_OK;
}

int aacg_pipeline_set_mix(aacg_pipeline* p, uint32_t out_channels, const float* matrix)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_mix", p->O != 0, "has a mix", "the mix",
                                  {{p->rs.L != 0, "a resampler"}, {p->ft.K != 0, "a feature stage"}, {p->lim.on, "a limiter"}, {p->tr.on, "a trim"}})) return no;
    if (out_channels < 1 || out_channels > AACG_MIX_MAX_OUT) { p->err = "aacg_pipeline_set_mix: out_channels is not 1 or 2"; return AACG_ERR_INVALID_ARG; }
    if (!matrix) { p->err = "aacg_pipeline_set_mix: no matrix"; return AACG_ERR_INVALID_ARG; }
    if (not_finite(p, matrix, (size_t)out_channels * p->C, "aacg_pipeline_set_mix: coefficient ", " of the matrix")) return AACG_ERR_INVALID_ARG;
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const size_t bytes = (size_t)p->cfg.max_streams * (size_t)p->cfg.max_frames * out_channels * 1024u * pcm_elem(p);
    if (!lanes_alloc(p, &lane_t::d_mix, bytes)) return no_memory(p, {}, nullptr, "aacg_pipeline_set_mix: no device memory for the lanes' mixed PCM");
    drop_host_staging(p);
    std::memset(p->mix, 0, sizeof p->mix);
    std::memcpy(p->mix, matrix, (size_t)out_channels * p->C * sizeof(float));
    p->O = out_channels;
    return AACG_OK;
}

int aacg_pipeline_out_channels(const aacg_pipeline* p) { return p ? (int)out_channels(p) : AACG_ERR_INVALID_ARG; }

int aacg_pipeline_set_resample(aacg_pipeline* p, uint32_t L, uint32_t M, uint32_t taps, const float* table)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_resample", p->rs.L != 0, "has a resampler", "the resampler", {{p->ft.K != 0, "a feature stage"}, {p->tr.on, "a trim"}})) return no;
    if (const int why = aacg_resample_check(L, M, taps)) { p->err = std::string("aacg_pipeline_set_resample: ") + aacg_resample_why(why); return AACG_ERR_INVALID_ARG; }
    if (!table) { p->err = "aacg_pipeline_set_resample: no table"; return AACG_ERR_INVALID_ARG; }
    const size_t n_table = (size_t)L * taps;
    if (not_finite(p, table, n_table, "aacg_pipeline_set_resample: coefficient ", " of the table")) return AACG_ERR_INVALID_ARG;
    /* the largest batch's output, samples per channel: the kernel and its records count them in 32 bits */
    const uint64_t most = aacg_pipe::exit_resample_most((uint32_t)p->cfg.max_streams, (uint32_t)p->cfg.max_frames, L, M);
    if (most >= (1ull << 31)) { p->err = "aacg_pipeline_set_resample: max_streams x max_frames x 1024 x L / M is 2^31 samples or more"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const uint32_t O = out_channels(p);
    const size_t lane_elems = (size_t)most * O, hist_bytes = (size_t)p->cfg.max_streams * 2u * (taps - 1u) * O * sizeof(float);
    void *d_table = nullptr, *d_hist = nullptr;
    /* (the table, synchronously: nothing is in flight yet.  The history needs no clearing: a fresh slot's is not read) */
    if (hipMalloc(&d_table, n_table * sizeof(float)) != hipSuccess || hipMalloc(&d_hist, hist_bytes) != hipSuccess ||
        !lanes_alloc(p, &lane_t::d_rs, lane_elems * pcm_elem(p)) || hipMemcpy(d_table, table, n_table * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return no_memory(p, {d_table, d_hist}, &lane_t::d_rs, "aacg_pipeline_set_resample: no device memory for the table, the slots' histories and the lanes' resampled PCM");
    drop_host_staging(p);
    p->rs.make((size_t)p->cfg.max_streams); p->rs.d_table = d_table; p->rs.d_hist = d_hist; p->rs.lane_elems = lane_elems;
    p->rs.M = M; p->rs.T = taps; p->rs.L = L;
    return AACG_OK;
}

int aacg_pipeline_set_features(aacg_pipeline* p, const aacg_features_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_features", p->ft.K != 0, "has a feature stage", "the stage", {}, !cfg)) return no;
    const uint32_t K = cfg->frame_length, H = cfg->hop, R = cfg->n_rows, NM = cfg->n_mels;
    if (const int why = aacg_features_check(K, H, cfg->pad_left, R, NM)) { p->err = std::string("aacg_pipeline_set_features: ") + aacg_features_why(why); return AACG_ERR_INVALID_ARG; }
    if (!(cfg->floor > 0.0f) || !std::isfinite(cfg->floor)) { p->err = "aacg_pipeline_set_features: floor is not positive and finite"; return AACG_ERR_INVALID_ARG; }
    if (out_channels(p) != 1u) { p->err = "aacg_pipeline_set_features: the stage takes ONE channel (channels == 1, or a mix with out_channels 1)"; return AACG_ERR_INVALID_ARG; }
    if (!cfg->basis || !cfg->fb) { p->err = "aacg_pipeline_set_features: no table"; return AACG_ERR_INVALID_ARG; }
    const size_t n_basis = (size_t)R * K, n_fb = (size_t)NM * (R / 2u);
    if (not_finite(p, cfg->basis, n_basis, "aacg_pipeline_set_features: entry ", " of basis") || not_finite(p, cfg->fb, n_fb, "aacg_pipeline_set_features: entry ", " of fb")) return AACG_ERR_INVALID_ARG;
    /* the largest batch's output, floats: the kernel and its records count them in 32 bits */
    const uint64_t most = aacg_pipe::exit_features_most((uint32_t)p->cfg.max_streams, most_samples(p), H) * NM;
    if (most >= (1ull << 31)) { p->err = "aacg_pipeline_set_features: max_streams x max_frames x 1024 x (L / M) / hop x n_mels is 2^31 or more"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const size_t hist_bytes = (size_t)p->cfg.max_streams * 2u * (K - 1u) * sizeof(float);
    void *d_basis = nullptr, *d_fb = nullptr, *d_hist = nullptr;
    /* (the tables, synchronously: nothing is in flight yet.  The history needs no clearing: a fresh slot's is not read) */
    if (hipMalloc(&d_basis, n_basis * sizeof(float)) != hipSuccess || hipMalloc(&d_fb, n_fb * sizeof(float)) != hipSuccess || hipMalloc(&d_hist, hist_bytes) != hipSuccess ||
        !lanes_alloc(p, &lane_t::d_ft, (size_t)most * sizeof(float)) ||
        hipMemcpy(d_basis, cfg->basis, n_basis * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_fb, cfg->fb, n_fb * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return no_memory(p, {d_basis, d_fb, d_hist}, &lane_t::d_ft, "aacg_pipeline_set_features: no device memory for the tables, the slots' histories and the lanes' feature frames");
    drop_host_staging(p);
    p->ft.make((size_t)p->cfg.max_streams); p->ft.d_basis = d_basis; p->ft.d_fb = d_fb; p->ft.d_hist = d_hist; p->ft.lane_elems = (size_t)most;
    p->ft.H = H; p->ft.P = cfg->pad_left; p->ft.R = R; p->ft.n_mels = NM; p->ft.log = cfg->log ? 1u : 0u; p->ft.floor = cfg->floor; p->ft.K = K;
    return AACG_OK;
}

int aacg_pipeline_set_loudness(aacg_pipeline* p, const aacg_loudness_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_loudness", p->ld.hop != 0, "has a meter", "the meter", {}, !cfg)) return no;
    if (cfg->hop < 1u || cfg->hop > AACG_LOUDNESS_MAX_HOP) { p->err = "aacg_pipeline_set_loudness: hop is not in 1..2^20"; return AACG_ERR_INVALID_ARG; }
    if (not_finite(p, &cfg->coeffs[0][0], 10, "aacg_pipeline_set_loudness: coefficient ", "")) return AACG_ERR_INVALID_ARG;
    const uint64_t most = most_hops(p, cfg->hop);          /* the largest batch's records per channel */
    if (most * p->C >= (1ull << 27)) { p->err = "aacg_pipeline_set_loudness: max_streams x (max_frames x 1024 / hop + 1) x channels is 2^27 records or more"; return AACG_ERR_INVALID_ARG; }
    /* (... and the kernel's lanes count a batch's PCM in 16-byte vectors, in 32 bits) */
    if ((uint64_t)p->cfg.max_streams * (uint64_t)p->cfg.max_frames * (1024u * p->C * pcm_elem(p) / 16u) > AACG_LOUDNESS_MAX_VECTORS) { p->err = "aacg_pipeline_set_loudness: max_streams x max_frames frames of PCM are 64 GiB or more"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const size_t state_bytes = (size_t)p->cfg.max_streams * 2u * p->C * AACG_LOUDNESS_STATE * sizeof(float);
    /* a lane's results get a block with room for the records in front of them (the state needs no clearing: a fresh slot's is not read) */
    void* d_state = nullptr;
    if (hipMalloc(&d_state, state_bytes) != hipSuccess || !results_blocks(p, ((size_t)most * p->C * 2u * sizeof(float) + 15) & ~(size_t)15))
        return no_memory(p, {d_state}, nullptr, "aacg_pipeline_set_loudness: no device memory for the slots' state and the lanes' records");
    p->ld.make((size_t)p->cfg.max_streams); p->ld.d_state = d_state;
    std::memcpy(p->ld.coeffs, cfg->coeffs, sizeof p->ld.coeffs);
    p->ld.hop = cfg->hop;
    return AACG_OK;
}

int aacg_pipeline_set_limiter(aacg_pipeline* p, const aacg_limiter_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_limiter", p->lim.on, "has a limiter", "the limiter", {{p->tr.on, "a trim"}}, !cfg)) return no;
    if (!(cfg->ceiling > 0.0f) || !std::isfinite(cfg->ceiling)) { p->err = "aacg_pipeline_set_limiter: ceiling is not positive and finite"; return AACG_ERR_INVALID_ARG; }
    if (!(cfg->release > 0.0f) || !(cfg->release <= 1.0f)) { p->err = "aacg_pipeline_set_limiter: release is not in (0, 1]"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const uint32_t Oc = out_channels(p);
    const size_t bytes = (size_t)p->cfg.max_streams * (size_t)p->cfg.max_frames * Oc * 1024u * pcm_elem(p);
    const size_t state_bytes = (size_t)p->cfg.max_streams * 2u * AACG_LIMIT_STATE(Oc) * sizeof(float);
    void* d_state = nullptr;
    /* (the state needs no clearing: a fresh slot's is not read) */
    if (hipMalloc(&d_state, state_bytes) != hipSuccess || !lanes_alloc(p, &lane_t::d_lim, bytes))
        return no_memory(p, {d_state}, nullptr, "aacg_pipeline_set_limiter: no device memory for the slots' state and the lanes' limited PCM");
    p->lim.make((size_t)p->cfg.max_streams); p->lim.d_state = d_state; p->lim.ceiling = cfg->ceiling; p->lim.release = cfg->release;
    p->lim.on = true;
    return AACG_OK;
}

int aacg_pipeline_set_limiter_true_peak(aacg_pipeline* p, const aacg_true_peak_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!cfg) { p->err = "aacg_pipeline_set_limiter_true_peak: no configuration"; return AACG_ERR_INVALID_ARG; }
    if (!p->lim.on) { p->err = "aacg_pipeline_set_limiter_true_peak: the pipeline has no limiter (aacg_pipeline_set_limiter comes first)"; return AACG_ERR_INVALID_ARG; }
    if (const int no = refuse_set(p, "aacg_pipeline_set_limiter_true_peak", p->lim.tp_L != 0, "has a true-peak detector", "the detector", {{p->tr.on, "a trim"}})) return no;
    if (const int why = aacg_truepeak_check(cfg->phases, cfg->taps)) { p->err = std::string("aacg_pipeline_set_limiter_true_peak: ") + aacg_truepeak_why(why); return AACG_ERR_INVALID_ARG; }
    if (!cfg->table) { p->err = "aacg_pipeline_set_limiter_true_peak: no table"; return AACG_ERR_INVALID_ARG; }
    const size_t n_table = (size_t)cfg->phases * cfg->taps;
    if (not_finite(p, cfg->table, n_table, "aacg_pipeline_set_limiter_true_peak: coefficient ", "")) return AACG_ERR_INVALID_ARG;
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    /* (the histories need no clearing: a fresh slot's is not read; the lanes' scratch is written whole by every batch's detector) */
    const size_t hist_bytes = (size_t)p->cfg.max_streams * 2u * AACG_LIMIT_TP_HIST(cfg->taps, out_channels(p)) * sizeof(float);
    const size_t peak_bytes = (size_t)p->cfg.max_streams * (size_t)p->cfg.max_frames * AACG_LIMIT_TP_FRAME_BLOCKS * sizeof(float);
    void *d_table = nullptr, *d_hist = nullptr;
    if (hipMalloc(&d_table, n_table * sizeof(float)) != hipSuccess || hipMemcpy(d_table, cfg->table, n_table * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&d_hist, hist_bytes) != hipSuccess || !lanes_alloc(p, &lane_t::d_lim_peak, peak_bytes))
        return no_memory(p, {d_table, d_hist}, nullptr, "aacg_pipeline_set_limiter_true_peak: no device memory for the table, the slots' state and the lanes' scratch");
    p->lim.d_tp_table = d_table; p->lim.d_tp_hist = d_hist; p->lim.tp_T = cfg->taps; p->lim.tp_L = cfg->phases;
    return AACG_OK;
}

int aacg_pipeline_limiter_delay(const aacg_pipeline* p, uint32_t* samples)
{
    if (!p || !samples || !p->lim.on) return AACG_ERR_INVALID_ARG;
    *samples = AACG_LIMIT_BLOCK + p->lim.tp_T / 2u;
    return AACG_OK;
}

int aacg_pipeline_set_concealment(aacg_pipeline* p, const aacg_conceal_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_concealment", p->cn.on, "conceals", "concealment", {}, !cfg)) return no;
    if (cfg->fade_steps > 64u) { p->err = "aacg_pipeline_set_concealment: fade_steps is not in 0..64"; return AACG_ERR_INVALID_ARG; }
    if (cfg->hold_frames < 1u || cfg->hold_frames > 255u) { p->err = "aacg_pipeline_set_concealment: hold_frames is not in 1..255"; return AACG_ERR_INVALID_ARG; }
    if (!p->shaped) {
        p->err = "aacg_pipeline_set_concealment: plan_mode 0 — its retry of a stale plan would run the stage twice for one batch; plan_mode 1's shaped set is never stale";
        return AACG_ERR_UNSUPPORTED;
    }
    if (p->spec_stages) {
        p->err = "aacg_pipeline_set_concealment: not with AACG_PIPELINE_STAGE_TNS or AACG_PIPELINE_STAGE_PNS (the TNS records of a repeated frame and repeated noise bands are not served)";
        return AACG_ERR_UNSUPPORTED;
    }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const size_t state_bytes = aacg_conceal_state_bytes((uint32_t)p->cfg.max_streams, p->Cp);
    void* d_state = nullptr;
    /* (cleared: a slot that has been through no batch is fresh and its side is not read, but the block is small and this is once) */
    if (hipMalloc(&d_state, state_bytes) != hipSuccess || hipMemset(d_state, 0, state_bytes) != hipSuccess)
        return no_memory(p, {d_state}, nullptr, "aacg_pipeline_set_concealment: no device memory for the slots' state");
    p->cn.side.make((size_t)p->cfg.max_streams); p->cn.d_state = d_state; p->cn.fade_steps = cfg->fade_steps; p->cn.hold_frames = cfg->hold_frames;
    p->cn.on = true;
    return AACG_OK;
}

int aacg_pipeline_concealed(const aacg_pipeline* p, uint64_t* count)
{
    if (!p || !count) return AACG_ERR_INVALID_ARG;
    *count = p->cn.total;
    return AACG_OK;
}

int aacg_pipeline_set_gain(aacg_pipeline* p, uint32_t slot, float gain)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!p->lim.on) { p->err = "aacg_pipeline_set_gain: the pipeline has no limiter (aacg_pipeline_set_limiter)"; return AACG_ERR_INVALID_ARG; }
    if ((int)slot >= p->cfg.max_streams) { p->err = "aacg_pipeline_set_gain: stream slot out of range"; return AACG_ERR_INVALID_ARG; }
    if (!aacg_limit_gain_ok(gain)) { p->err = "aacg_pipeline_set_gain: gain is not in 0..1024"; return AACG_ERR_INVALID_ARG; }
    p->lim.gain[slot] = gain;                            /* nothing in flight reads it: a batch's gains went up in its records */
    return AACG_OK;
}

int aacg_pipeline_gain(const aacg_pipeline* p, uint32_t slot, float* gain)
{
    if (!p || !gain || !p->lim.on || (int)slot >= p->cfg.max_streams) return AACG_ERR_INVALID_ARG;
    *gain = p->lim.gain[slot];
    return AACG_OK;
}

int aacg_pipeline_set_trim(aacg_pipeline* p, const aacg_trim_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (const int no = refuse_set(p, "aacg_pipeline_set_trim", p->tr.on, "has a trim", "the trim", {}, !cfg)) return no;
    if (aacg_trim_check(cfg->skip, cfg->keep)) { p->err = "aacg_pipeline_set_trim: skip or a finite keep is 2^40 or more"; return AACG_ERR_INVALID_ARG; }
    const uint64_t most = most_samples(p);               /* the largest batch's input, samples per channel */
    if (most >= (1ull << 31)) { p->err = "aacg_pipeline_set_trim: max_streams x max_frames x 1024 (x L / M) is 2^31 samples or more"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    /* (a host batch's trimmed PCM: at most what the stage receives.  With a feature stage the trim writes nothing) */
    if (!p->ft.K && !lanes_alloc(p, &lane_t::d_trim, (size_t)most * out_channels(p) * pcm_elem(p))) return no_memory(p, {}, nullptr, "aacg_pipeline_set_trim: no device memory for the lanes' trimmed PCM");
    p->tr.make((size_t)p->cfg.max_streams, cfg->skip, cfg->keep);
    p->tr.on = true;
    return AACG_OK;
}

int aacg_pipeline_set_stream_trim(aacg_pipeline* p, uint32_t slot, uint64_t skip, uint64_t keep)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!p->tr.on) { p->err = "aacg_pipeline_set_stream_trim: the pipeline has no trim (aacg_pipeline_set_trim)"; return AACG_ERR_INVALID_ARG; }
    if ((int)slot >= p->cfg.max_streams) { p->err = "aacg_pipeline_set_stream_trim: stream slot out of range"; return AACG_ERR_INVALID_ARG; }
    if (aacg_trim_check(skip, keep)) { p->err = "aacg_pipeline_set_stream_trim: skip or a finite keep is 2^40 or more"; return AACG_ERR_INVALID_ARG; }
    p->tr.S[slot] = skip; p->tr.K[slot] = keep; p->tr.Q[slot] = 0;      /* nothing in flight reads them: a batch's ranges went up in its records */
    return AACG_OK;
}

int aacg_pipeline_stream_trim(const aacg_pipeline* p, uint32_t slot, uint64_t* skip, uint64_t* keep, uint64_t* position)
{
    if (!p || !p->tr.on || (int)slot >= p->cfg.max_streams) return AACG_ERR_INVALID_ARG;
    if (skip) *skip = p->tr.S[slot];
    if (keep) *keep = p->tr.K[slot];
    if (position) *position = p->tr.Q[slot];
    return AACG_OK;
}

int aacg_pipeline_loudness_out(aacg_pipeline* p, float* records, size_t capacity_floats, uint32_t* n_out_of)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!p->ld.hop) { p->err = "aacg_pipeline_loudness_out: the pipeline has no meter (aacg_pipeline_set_loudness)"; return AACG_ERR_INVALID_ARG; }
    if (!records && capacity_floats) { p->err = "aacg_pipeline_loudness_out: no memory for the records"; return AACG_ERR_INVALID_ARG; }
    p->ld.out = records; p->ld.out_cap = capacity_floats; p->ld.out_counts = n_out_of; p->ld.armed = true;
    return AACG_OK;
}

int aacg_pipeline_set_true_peak(aacg_pipeline* p, const aacg_true_peak_config* cfg)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!cfg) { p->err = "aacg_pipeline_set_true_peak: no configuration"; return AACG_ERR_INVALID_ARG; }
    if (!p->ld.hop) { p->err = "aacg_pipeline_set_true_peak: the pipeline has no meter (aacg_pipeline_set_loudness comes first)"; return AACG_ERR_INVALID_ARG; }
    if (const int no = refuse_set(p, "aacg_pipeline_set_true_peak", p->tp.L != 0, "has a true-peak stage", "the stage")) return no;
    if (const int why = aacg_truepeak_check(cfg->phases, cfg->taps)) { p->err = std::string("aacg_pipeline_set_true_peak: ") + aacg_truepeak_why(why); return AACG_ERR_INVALID_ARG; }
    if (!cfg->table) { p->err = "aacg_pipeline_set_true_peak: no table"; return AACG_ERR_INVALID_ARG; }
    const size_t n_table = (size_t)cfg->phases * cfg->taps;
    if (not_finite(p, cfg->table, n_table, "aacg_pipeline_set_true_peak: coefficient ", "")) return AACG_ERR_INVALID_ARG;
    if ((uint64_t)p->cfg.max_streams * (uint64_t)p->cfg.max_frames > AACG_TRUEPEAK_MAX_FRAMES) { p->err = "aacg_pipeline_set_true_peak: max_streams x max_frames is more than 2^21 frames"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    /* the largest batch's floats, one per meter's record and channel (the meter's limit holds: below 2^27), in front of the meter's in
     * a lane's block, made again as aacg_pipeline_set_loudness made it.  The state IS cleared: a batch finds the partial maximum it
     * writes to empty (aacg_pcm_truepeak.h) */
    const size_t tp16 = ((size_t)most_hops(p, p->ld.hop) * p->C * sizeof(float) + 15) & ~(size_t)15;
    const size_t state_bytes = (size_t)p->cfg.max_streams * 2u * AACG_TRUEPEAK_STATE(cfg->taps, p->C) * sizeof(float);
    void *d_table = nullptr, *d_state = nullptr;
    if (hipMalloc(&d_table, n_table * sizeof(float)) != hipSuccess || hipMemcpy(d_table, cfg->table, n_table * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&d_state, state_bytes) != hipSuccess || hipMemset(d_state, 0, state_bytes) != hipSuccess || !results_blocks(p, p->ld.front16 + tp16))
        return no_memory(p, {d_table, d_state}, nullptr, "aacg_pipeline_set_true_peak: no device memory for the table, the slots' state and the lanes' records");
    p->tp.d_table = d_table; p->tp.d_state = d_state; p->tp.T = cfg->taps; p->tp.L = cfg->phases;
    return AACG_OK;
}

int aacg_pipeline_true_peak_out(aacg_pipeline* p, float* peaks, size_t capacity_floats)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (!p->tp.L) { p->err = "aacg_pipeline_true_peak_out: the pipeline has no true-peak stage (aacg_pipeline_set_true_peak)"; return AACG_ERR_INVALID_ARG; }
    if (!peaks && capacity_floats) { p->err = "aacg_pipeline_true_peak_out: no memory for the records"; return AACG_ERR_INVALID_ARG; }
    p->tp.out = peaks; p->tp.out_cap = capacity_floats; p->tp.armed = true;
    return AACG_OK;
}

int aacg_pipeline_loudness_counts(aacg_pipeline* p, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, uint32_t* n_out)
{
    if (!p || !slots || !frames_of || !n_out) return AACG_ERR_INVALID_ARG;
    if (!p->ld.hop) { p->err = "aacg_pipeline_loudness_counts: the pipeline has no meter (aacg_pipeline_set_loudness)"; return AACG_ERR_INVALID_ARG; }
    for (uint32_t s = 0; s < n_streams; s++) {
        if ((int)slots[s] >= p->cfg.max_streams) { p->err = "aacg_pipeline_loudness_counts: stream slot out of range"; return AACG_ERR_INVALID_ARG; }
        if ((int64_t)frames_of[s] > p->cfg.max_frames) { p->err = "aacg_pipeline_loudness_counts: a stream brings more frames than max_frames"; return AACG_ERR_INVALID_ARG; }
    }
    for (uint32_t s = 0; s < n_streams; s++) n_out[s] = (uint32_t)aacg_loudness_emits(p->ld.hop, p->ld.N[slots[s]], 1024ull * frames_of[s]);
    return AACG_OK;
}

int aacg_pipeline_out_samples(aacg_pipeline* p, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, uint32_t* n_out)
{
    if (!p || !slots || !frames_of || !n_out) return AACG_ERR_INVALID_ARG;
    for (uint32_t s = 0; s < n_streams; s++) {
        if ((int)slots[s] >= p->cfg.max_streams) { p->err = "aacg_pipeline_out_samples: stream slot out of range"; return AACG_ERR_INVALID_ARG; }
        if ((int64_t)frames_of[s] > p->cfg.max_frames) { p->err = "aacg_pipeline_out_samples: a stream brings more frames than max_frames"; return AACG_ERR_INVALID_ARG; }
    }
    for (uint32_t s = 0; s < n_streams; s++) n_out[s] = p->rs.L ? aacg_pipe::resample_count(p->rs.L, p->rs.M, p->rs.N[slots[s]], frames_of[s]) : frames_of[s] * 1024u;
    if (p->tr.on)                                        /* a trim: what the slots' windows keep of them at the slots' positions */
        for (uint32_t s = 0; s < n_streams; s++) { uint32_t first; aacg_trim_span(p->tr.Q[slots[s]], p->tr.S[slots[s]], p->tr.K[slots[s]], n_out[s], &first, &n_out[s]); }
    if (p->ft.K)                                         /* feature frames: what the samples above complete at the slots' clocks */
        for (uint32_t s = 0; s < n_streams; s++) { aacg_features_stream r; aacg_features_span(p->ft.K, p->ft.H, p->ft.P, p->ft.N[slots[s]], n_out[s], &r); n_out[s] = r.n_out; }
    return AACG_OK;
}

int aacg_mix_standard(uint32_t channels, uint32_t out_channels, float surround_gain, int normalise, float* matrix)
{
    /* what each position of the resident route's channel order gives the left and the right row (include/aacgpu.h has the table):
     * F: all of it to its side, C: 1/sqrt 2 to both, S: the surround gain to its side, B: the surround gain / sqrt 2 to both, 0: nothing */
    enum { Z, FL, FR, CC, SL, SR, BC };
    static const uint8_t pos[9][8] = {{}, {CC}, {FL, FR}, {CC, FL, FR}, {CC, FL, FR, BC}, {CC, FL, FR, SL, SR}, {CC, FL, FR, SL, SR, Z}, {},
                                      {CC, FL, FR, FL, FR, SL, SR, Z}};
    if (channels < 1 || channels > 8 || channels == 7 || out_channels < 1 || out_channels > 2 || !matrix || !std::isfinite(surround_gain)) return AACG_ERR_INVALID_ARG;
    const double a = (double)surround_gain, h = 1.0 / std::sqrt(2.0);
    double row[2][8], sum[2] = {0.0, 0.0};
    for (uint32_t c = 0; c < channels; c++) {
        const int k = pos[channels][c];
        row[0][c] = k == FL ? 1.0 : k == CC ? h : k == SL ? a : k == BC ? a * h : 0.0;
        row[1][c] = k == FR ? 1.0 : k == CC ? h : k == SR ? a : k == BC ? a * h : 0.0;
        sum[0] += row[0][c]; sum[1] += row[1][c];
    }
    if (normalise) {
        if (!(sum[0] > 0.0) || !(sum[1] > 0.0)) return AACG_ERR_INVALID_ARG;      /* (a negative surround gain that cancels a row) */
        for (uint32_t c = 0; c < channels; c++) { row[0][c] /= sum[0]; row[1][c] /= sum[1]; }
    }
    for (uint32_t c = 0; c < channels; c++) {
        if (out_channels == 2) { matrix[c] = (float)row[0][c]; matrix[channels + c] = (float)row[1][c]; }
        else matrix[c] = (float)((row[0][c] + row[1][c]) * 0.5);
    }
    return AACG_OK;
}

int aacg_pipeline_reset_stream(aacg_pipeline* p, uint32_t slot)
{
    if (!p || (int)slot >= p->cfg.max_streams) return AACG_ERR_INVALID_ARG;
    /* the slot's batches in flight belong to the stream that had it: they are finished first (aacg_reset_stream waits for the
     * engine's launches; the PCM on its way down and the caller's buffers are the lanes') */
    for (int k = 0; k < p->n_lanes; k++) { int rc = finish_lane(p, p->lane[k]); if (rc) return rc; }
    int rc = aacg_reset_stream(p->engine, slot);
    if (rc) return engine_fail(p, "", rc);
    if (p->rs.L) p->rs.reset(slot);                         /* the resampler's clock starts again; the history is zeros by the rule and is not read */
    if (p->ft.K) p->ft.reset(slot);                         /* ... and the feature stage's */
    if (p->ld.hop) p->ld.reset(slot);                       /* ... and the meter's: its filters, energy and peak are zeros by the rule and are not read */
    if (p->tr.on) p->tr.reset(slot);                        /* ... and the trim's position; the slot's window is the caller's and stays */
    if (p->cn.on) p->cn.side.reset(slot);                   /* ... and the last good frame: the slot's next batch starts with none */
    if (p->lim.on) p->lim.side.reset(slot);                     /* ... and the limiter's held block and nodes, and its detector's history; the slot's gain is the caller's and stays */
    if (p->learn && p->layout[slot].n) {                    /* a new stream: its layout is learnt anew; the plans made for the old one go */
        p->layout[slot] = aacg_pipeline::layout_t();
        drop_plans_with(p, slot);
    }
    return AACG_OK;
}

namespace {

/* Step 1, the host refusals: nothing is enqueued and no lane touched before they pass */
int check_batch(aacg_pipeline* p, batch_t& B)
{
    if ((int)B.n_streams > p->cfg.max_streams) { p->err = "batch larger than the pipeline was created for"; return AACG_ERR_CAPACITY; }
    uint64_t total = 0;
    B.longest = 0;
    for (uint32_t s = 0; s < B.n_streams; s++) {
        if (!B.frames_of[s]) { p->err = "a stream of the batch brings no frame (frames_of[s] == 0)"; return AACG_ERR_INVALID_ARG; }
        if ((int64_t)B.frames_of[s] > p->cfg.max_frames) { p->err = "a stream brings more frames than max_frames"; return AACG_ERR_CAPACITY; }
        total += B.frames_of[s];
        if (B.frames_of[s] > B.longest) B.longest = B.frames_of[s];
    }
    if (total > (uint64_t)p->cfg.max_streams * (uint64_t)p->cfg.max_frames) { p->err = "the batch's frames exceed max_streams x max_frames"; return AACG_ERR_CAPACITY; }
    B.n = (uint32_t)total;
    for (uint32_t s = 0; s < B.n_streams; s++) if ((int)B.slots[s] >= p->cfg.max_streams) { p->err = "stream slot out of range"; return AACG_ERR_CAPACITY; }
    {   /* a slot is one stream's overlap state: a batch brings each at most once (its frames are consecutive ones of that stream) */
        std::vector<bool> seen((size_t)p->cfg.max_streams, false);
        for (uint32_t s = 0; s < B.n_streams; s++) { if (seen[B.slots[s]]) { p->err = "a stream slot is listed twice in one batch"; return AACG_ERR_INVALID_ARG; } seen[B.slots[s]] = true; }
    }
    for (uint32_t i = 0; i < B.n; i++)
        if ((size_t)B.frames[i].byte_offset + B.frames[i].byte_length > B.n_bytes) { p->err = "a frame points outside the byte buffer"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    /* the way out, decided here and nowhere else.  Page-locked caller memory (aacg_host_alloc) takes the PCM straight from the device;
     * anything else goes through the lane's own page-locked staging and one host copy at collect */
    aacg_exit_batch b = {B.n, B.n_streams, B.longest, 0u, B.dev ? B.dev->stride_frames : 0u, 0u, 0u};
    b.dest = B.pcm_out ? (is_pinned(B.pcm_out) ? AACG_EXIT_HOST_PINNED : AACG_EXIT_HOST_PAGEABLE) : aacg_pipe::exit_dest_device(B.dev ? B.dev->layout : AACG_PCM_PACKED);
    /* the records of the stages that are set, from the slots' state as it stands (aacg_pipe_slots.h): it advances in enqueue_out.  The
     * trim in front of the feature stage: that one takes each stream's kept range */
    if (p->rs.L) aacg_pipe::build_resample(p->rs, B.slots, B.frames_of, B.n_streams, B.rs, b);
    if (p->tr.on) aacg_pipe::build_trim(p->tr, B.rs, b.dest == AACG_EXIT_DEV_PLANAR && !p->ft.K, B.slots, B.frames_of, B.n_streams, B.tr, B.tr_in, B.tr_items, b);
    if (p->ft.K) aacg_pipe::build_features(p->ft, B.rs, B.tr, B.slots, B.frames_of, B.n_streams, B.ft, B.ft_items, b);
    if (p->ld.hop) {                                     /* a meter, and the true-peak stage beside it: whether the named destinations hold the batch's records */
        if (!p->ld.armed) { p->err = "the pipeline has a meter and no destination is named for this submission's records (aacg_pipeline_loudness_out)"; return AACG_ERR_INVALID_ARG; }
        aacg_pipe::build_loudness(p->ld, p->C, p->tp.L != 0, B.slots, B.frames_of, B.n_streams, B.ld, B.ld_floats, B.tp_floats);
        if (B.ld_floats > p->ld.out_cap) { p->err = "the destination named for the loudness records is too small for this submission"; return AACG_ERR_CAPACITY; }
        if (p->tp.L && !p->tp.armed) { p->err = "the pipeline has a true-peak stage and no destination is named for this submission's records (aacg_pipeline_true_peak_out)"; return AACG_ERR_INVALID_ARG; }
        if (p->tp.L && B.tp_floats > p->tp.out_cap) { p->err = "the destination named for the true-peak records is too small for this submission"; return AACG_ERR_CAPACITY; }
    }
    if (p->lim.on) aacg_pipe::build_limiter(p->lim, B.slots, B.frames_of, B.n_streams, B.lim);
    if (p->cn.on) B.cn.assign(B.n_streams, aacg_conceal_stream());      /* concealment: a record per stream, made from the plan's table (choose_plan) */
    B.X = aacg_pipe::exit_plan(exit_pipe(p), b);
    return B.pcm_out ? AACG_OK : check_device_out(p, B, b);
}

/* Step 3, staging: the bytes, the frame table and room for the per-stream table that aacg_pipe_map expands into the refresh map
 * (plan mode 1: that the shaping kernel reads) in one block, the tables behind the bytes on the device too; and the lane's page-locked
 * PCM staging, if the way out goes through it */
int stage_batch(aacg_pipeline* p, aacg_pipeline::lane_t& L, batch_t& B)
{
    /* (the stages' per-stream records lie behind the per-stream table, 16-byte aligned, section behind section: one block, one copy up) */
    const size_t tab_bytes = (size_t)B.n_streams * (p->shaped ? sizeof(aacg_shape_stream) : sizeof(aacg_pipe_stream)), tab16 = (tab_bytes + 15) & ~(size_t)15;
    B.R = RB(B.rs, B.ft, B.ld, B.lim, B.cn, B.tr);
    const size_t more = B.R.lay(0);
    int rc = stage(p, &L.h_in, &L.d_bytes, &L.bytes_cap, B.bytes, B.n_bytes, B.frames, B.n, more ? tab16 + more : tab_bytes, B.G);
    if (rc) return rc;
    B.R.lay(B.G.extra_at + tab16);
    B.R.copy(L.h_in);                                    /* (the concealment's once more when they are made: choose_plan) */
    L.d_frames = (char*)L.d_bytes + B.G.padded;
    if (B.X.collect_copy && !L.h_pcm) P_TRY(p, hipHostMalloc(&L.h_pcm, aacg_pipe::exit_host_capacity(exit_pipe(p)), hipHostMallocDefault), AACG_ERR_OUT_OF_MEMORY);
    return AACG_OK;
}

/* Step 4, the plan is chosen and the per-stream table filled in: the first of the two places where the plan modes part */
int choose_plan(aacg_pipeline* p, const aacg_pipeline::lane_t& L, batch_t& B)
{
    void* const tab = (char*)L.h_in + B.G.extra_at;
    if (!p->shaped) {
        aacg_pipe::plan_list(p->batch_layout.data(), B.slots, B.frames_of, B.n_streams, p->C, p->Cp, p->U, nullptr, nullptr, (aacg_pipe_stream*)tab);
        return plan_for(p, B.slots, B.frames_of, B.n_streams, &B.plan);
    }
    /* the plan is chosen: the one there is, its set of this lane shaped from the batch's table — which the engine checks against
     * the plan's capacity and completes (each stream's first run and link, the overlap rotation) before anything is enqueued */
    uint32_t n_units = 0;
    aacg_pipe::shape_table(p->batch_layout.data(), B.slots, B.frames_of, B.n_streams, (aacg_shape_stream*)tab);
    int rc = aacg_plan_shape_table(p->engine, p->shaped, B.set, (aacg_shape_stream*)tab, B.n_streams, p->Cp, &n_units);
    B.plan = n_units ? p->shaped : nullptr;              /* (no stream of the batch has a layout yet: nothing to transform, as with kept plans) */
    if (p->cn.on) {                                      /* concealment: its records from the completed table, into their section */
        aacg_pipe::build_conceal(p->cn, (const aacg_shape_stream*)tab, B.n_streams, B.cn);
        B.R.copy(L.h_in, RB::CN);
    }
    return rc ? engine_fail(p, "aacg_plan_shape_table: ", rc) : AACG_OK;
}

/* Step 5, the front of the lane's stream: the clear for unlearnt streams, the staging's copy up, the stale count, the parse, the TNS
 * records, and the map or — the second place where the plan modes part — the shaping launch */
int enqueue_front(aacg_pipeline* p, aacg_pipeline::lane_t& L, const batch_t& B)
{
    hipStream_t st = L.st;
    const uint32_t Cp = p->Cp, U = p->U;
    L.unlearnt.clear();
    if (p->learn) for (uint32_t s = 0, i = 0; s < B.n_streams; i += B.frames_of[s], s++) if (!p->layout[B.slots[s]].kept) L.unlearnt.push_back({i, B.frames_of[s]});
    if (!L.unlearnt.empty()) P_TRY(p, hipMemsetAsync(exit_buf(L, B, B.X.stage[0].dst), 0, B.X.xform_bytes, st), AACG_ERR_NO_DEVICE);      /* no unit writes their frames: the transform's destination, cleared */
    pipe_copy(L.h_in, L.d_bytes, B.G.up, st);             /* aacg_pipe_copy: not the SDMA engines, where it would queue behind other lanes' PCM */
    if (L.count_stale) P_TRY(p, hipMemsetAsync(L.d_refused, 0, 16, st), AACG_ERR_NO_DEVICE);      /* a submission that failed half-way left its count behind */
    L.count_stale = true;
    /* the spectra of a refused frame and the positions outside the coded bands are never read by the transform (a refused frame
     * becomes a silent unit), so the parser need not clear 8 KB per frame first */
    int rc = aacg_parse_device(L.parser, L.d_bytes, (const aacg_parse_frame*)L.d_frames, B.n, U, Cp, (uint32_t)p->cfg.parse_options | AACG_PARSE_SKIP_ZERO_FILL,
                               (aacg_unit_desc*)L.d_units, (int16_t*)L.d_q, (aacg_band_meta*)L.d_meta, (aacg_tns_info*)L.d_tns_info, (aacg_parse_result*)L.d_res, st);
    if (rc) { p->err = std::string("aacg_parse_device: ") + aacg_parser_last_error(L.parser); return rc; }
    if (!B.plan) return AACG_OK;
    /* AACG_PIPELINE_STAGE_TNS: the batch's TNS records and their matrices, made where the side info lies, behind the parse on the
     * lane's stream; the launch that read this lane's buffer last was its previous batch's, whose PCM has come down since */
    if (L.d_tns && (rc = aacg_tns_records_from_parse(p->engine, (const aacg_unit_desc*)L.d_units, (const aacg_parse_result*)L.d_res, (const aacg_tns_info*)L.d_tns_info,
                                                     B.n, U, Cp, L.d_tns, st))) return engine_fail(p, "aacg_tns_records_from_parse: ", rc);
    const void* const d_tab = (const char*)L.d_bytes + B.G.extra_at;
    if (p->shaped) {                                     /* the shaping kernel INSTEAD of aacg_pipe_map: the map, and the set's unit, run and link records */
        if ((rc = aacg_plan_shape_launch(p->engine, p->shaped, (const aacg_shape_stream*)d_tab, U, (aacg_refresh_map*)L.d_map, st))) return engine_fail(p, "aacg_plan_shape_launch: ", rc);
        p->shaped_batches++;
    } else {                                             /* the map the refresh reads: behind the staging's copy, on the lane's stream */
        const uint32_t blocks = B.n_streams < 256 ? B.n_streams : 256;
        hipLaunchKernelGGL(aacg_pipe_map, dim3(blocks), dim3(AACG_PIPE_MAP_THREADS), 0, st, (const aacg_pipe_stream*)d_tab, B.n_streams, U, (aacg_refresh_map*)L.d_map);
    }
    return AACG_OK;
}

/* Step 6, the transform and the join behind it; a batch without a plan has neither */
int enqueue_transform(aacg_pipeline* p, aacg_pipeline::lane_t& L, batch_t& B)
{
    int rc = AACG_OK;
    void* const d_pcm = exit_buf(L, B, B.X.stage[0].dst);      /* the exit plan's first stage is the transform */
    for (int attempt = 0; B.plan; attempt++) {
        /* this lane's set of the plan's unit records: the launch that read it last was this lane's previous batch, whose PCM has
         * come down on this stream since */
        rc = aacg_plan_refresh_from_parse_ex(p->engine, B.plan, (const aacg_unit_desc*)L.d_units, (aacg_parse_result*)L.d_res, p->U,
                                             (const aacg_refresh_map*)L.d_map, B.set, (uint32_t*)L.d_refused, L.st);
        /* AACG_PIPELINE_STAGE_WINDOW_SHAPE: the refreshed shapes are final — each frame's first half takes the shape of the frame
         * before, a stream's first frame the one its previous batch left (a second attempt starts from where the first started) */
        /* aacg_pipeline_set_concealment: a refused frame takes its stream's last good frame, faded — in front of the carry, so that the
         * shape carried behind a concealed frame is that frame's */
        if (rc == AACG_OK && p->cn.on)
            rc = aacg_plan_conceal_refused(p->engine, B.plan, B.set, (aacg_parse_result*)L.d_res, (int16_t*)L.d_q, (aacg_band_meta*)L.d_meta, p->Cp,
                                           (const aacg_conceal_stream*)((const char*)L.d_bytes + B.R.at(RB::CN)), B.n_streams, B.longest, p->cn.d_state,
                                           (uint32_t)p->cfg.max_streams, p->cn.fade_steps, p->cn.hold_frames, L.st);
        if (rc == AACG_OK && p->carry_shape) rc = aacg_plan_carry_window_shape(p->engine, B.plan, (const aacg_refresh_map*)L.d_map, B.set, L.st);
        /* the transform: behind this lane's parse and refresh (fork), in front of its copy down (join); consecutive batches of
         * one shape are consecutive launches of one plan and overlap through the rendezvous cells */
        if (rc == AACG_OK) rc = aacg_pipeline_fork(p->engine, L.st);
        if (rc == AACG_OK) rc = p->spec_stages ? aacg_decode_pipelined_stages(p->engine, B.plan, L.d_q, (const aacg_band_meta*)L.d_meta, L.d_tns, L.d_tns ? B.n * p->Cp : 0u, d_pcm)
                                              : aacg_decode_pipelined(p->engine, B.plan, L.d_q, (const aacg_band_meta*)L.d_meta, d_pcm);
        if (rc == AACG_OK) p->launches++;
        if (rc != AACG_ERR_STALE_PLAN || attempt || p->shaped) break;      /* (a shaped set is made from the engine's current state inside this call: never stale) */
        if ((rc = replan_stale(p, L, B))) return rc;        /* plan mode 0: once more, with a plan made now */
    }
    if (rc == AACG_OK && B.plan) rc = aacg_pipeline_join(p->engine, L.st);
    return rc ? engine_fail(p, "transform: ", rc) : AACG_OK;
}

/* Step 7, the way out: the exit plan's stages behind the transform, each from the buffer the one before wrote; then the results' copy,
 * the lane's event, what finish_lane needs */
int enqueue_out(aacg_pipeline* p, aacg_pipeline::lane_t& L, const batch_t& B, uint64_t* ticket)
{
    const uint32_t Oc = out_channels(p), E = (uint32_t)pcm_elem(p);
    for (uint32_t i = 1; i < B.X.n_stages; i++) {
        const aacg_exit_stage& S = B.X.stage[i];
        const void* const src = exit_buf(L, B, S.src);
        void* const dst = exit_buf(L, B, S.dst);
        if (S.what == AACG_EXIT_MIX) {                   /* the packed PCM of C channels into O */
            aacg_mix_args M = {src, dst, B.n, p->C, p->O, E, {}};
            std::memcpy(M.m, p->mix, sizeof M.m);
            if (!aacg_mix_launch(M, L.st)) return not_served(p, "aacg_pcm_mix");
        } else if (S.what == AACG_EXIT_LIMIT) {
            /* the packed PCM of Oc channels, gained and limited, sample for sample; the slots' held blocks and nodes pass from batch to batch */
            const aacg_limit_args A = {src, dst, (const aacg_limit_stream*)((const char*)L.d_bytes + B.R.at(RB::LIM)), (float*)p->lim.d_state, B.n_streams, B.n,
                                       p->lim.ceiling, p->lim.release, Oc, E};
            /* ... and with the true-peak detector the histories too: its two launches stand where the plain one stands */
            const aacg_limit_tp_args Q = {A, (const float*)p->lim.d_tp_table, (float*)p->lim.d_tp_hist, (float*)L.d_lim_peak, p->lim.tp_L, p->lim.tp_T};
            if (const int rc = ordered_launch(p, L, ORD_LIMIT, [&] {
                    if (p->lim.tp_L) return aacg_limit_tp_launch(Q, L.st) ? AACG_OK : not_served(p, "aacg_pcm_limit_tp");
                    return aacg_limit_launch(A, L.st) ? AACG_OK : not_served(p, "aacg_pcm_limit"); })) return rc;
        } else if (S.what == AACG_EXIT_RESAMPLE) {
            /* the packed PCM at the new rate, either layout; the slots' histories pass from batch to batch */
            const aacg_resample_args A = {src, dst, (const aacg_resample_stream*)((const char*)L.d_bytes + B.R.at(RB::RS)), (const float*)p->rs.d_table, (float*)p->rs.d_hist,
                                          B.n_streams, B.n, p->rs.L, p->rs.M, p->rs.T, S.dst == AACG_EXIT_CALLER ? B.X.row : 0u, Oc, E};      /* (the row is the stage's that writes the caller's tensor) */
            if (const int rc = ordered_launch(p, L, ORD_RESAMPLE, [&] { return aacg_resample_launch(A, L.st) ? AACG_OK : not_served(p, "aacg_pcm_resample"); })) return rc;
        } else if (S.what == AACG_EXIT_FEATURES) {
            /* the one channel of PCM, as the stage before left it, into feature frames, either layout; the slots' histories pass from batch to batch */
            const aacg_features_args A = {src, (float*)dst, (const aacg_features_stream*)((const char*)L.d_bytes + B.R.at(RB::FT)), (const float*)p->ft.d_basis, (const float*)p->ft.d_fb,
                                          (float*)p->ft.d_hist, B.n_streams, B.ft_items, p->ft.K, p->ft.H, p->ft.R, p->ft.n_mels, p->ft.floor, p->ft.log, B.X.ft_row, E};
            if (const int rc = ordered_launch(p, L, ORD_FEATURES, [&] { return aacg_features_launch(A, L.st) ? AACG_OK : not_served(p, "aacg_pcm_features"); })) return rc;
        } else if (S.what == AACG_EXIT_TRIM) {
            /* each stream's kept range of the packed PCM, as the stage before left it, either layout.  No state: nothing to wait for and
             * no event.  A batch that keeps nothing launches nothing for a packed destination; a planar one still gets its zeros */
            const uint64_t src_elems = (uint64_t)(p->rs.L ? B.rs.back().out_first + B.rs.back().n_out : B.n * 1024u) * Oc;
            const aacg_trim_args A = {src, dst, (const aacg_trim_stream*)((const char*)L.d_bytes + B.R.at(RB::TR)), src_elems, B.n_streams, B.tr_items, B.X.row, Oc, E};
            if (B.tr_items && !aacg_trim_launch(A, L.st)) return not_served(p, "aacg_pcm_trim");
        } else if (S.tail == AACG_EXIT_TAIL_COPY_DOWN && p->tr.on && !S.bytes) {
            /* (a trim kept nothing of the batch: no copy of nothing) */
        } else if (S.tail == AACG_EXIT_TAIL_PLANAR_LAUNCH) {
            /* the caller's tensor from the packed PCM and the per-stream table that came up with the bytes (either plan mode's record
             * begins with frame_first and frames), padding included: where the copy down sits for a host batch */
            const aacg_planar_args A = {src, dst, (const char*)L.d_bytes + B.G.extra_at, (uint32_t)(p->shaped ? sizeof(aacg_shape_stream) : sizeof(aacg_pipe_stream)),
                                        B.n_streams, B.dev->stride_frames, Oc, E};
            if (!aacg_planar_launch(A, L.st)) return not_served(p, "aacg_pcm_planar");
        } else                                           /* AACG_EXIT_TAIL_COPY_DOWN: one SDMA copy per batch (see aacg_pipe_copy) */
            P_TRY(p, hipMemcpyAsync(dst, src, S.bytes, hipMemcpyDeviceToHost, L.st), AACG_ERR_NO_DEVICE);
    }
    /* the results and, behind where the largest batch's would end, the refusal count: one small launch (a launch that writes to
     * host memory costs 50 us of the lane's time whatever it carries) */
    L.count_stale = false;
    size_t ld16 = 0, tp16 = 0;
    if (p->ld.hop) {
        /* the meter: the transform's PCM, wherever the exit plan's first stage put it, into records that lie right in front of the lane's
         * results, so that the one copy below brings both down.  The slots' state passes from batch to batch */
        ld16 = (B.ld_floats * sizeof(float) + 15) & ~(size_t)15;
        tp16 = (B.tp_floats * sizeof(float) + 15) & ~(size_t)15;
        aacg_loudness_args A = {exit_buf(L, B, B.X.stage[0].dst), (float*)((char*)L.d_res - ld16), (const aacg_loudness_stream*)((const char*)L.d_bytes + B.R.at(RB::LD)),
                                (float*)p->ld.d_state, B.n_streams, B.n, p->ld.hop, {}, p->C, E};
        std::memcpy(A.coeffs, p->ld.coeffs, sizeof A.coeffs);
        const int rc = ordered_launch(p, L, ORD_METER, [&]() -> int {
            if (!aacg_loudness_launch(A, L.st)) return not_served(p, "aacg_pcm_loudness");
            if (!p->tp.L) return AACG_OK;
            /* the true peak, beside the meter: the same PCM and the same records, into floats that lie in front of the meter's and are
             * cleared first (hops that straddle frames arrive as atomic maxima).  Its slots' state is ordered by the meter's event, which
             * is recorded behind both launches */
            uint32_t* const d_tp = (uint32_t*)((char*)L.d_res - ld16 - tp16);
            if (tp16) P_TRY(p, hipMemsetAsync(d_tp, 0, tp16, L.st), AACG_ERR_NO_DEVICE);
            const aacg_truepeak_args Q = {A.src, d_tp, A.rec, (const float*)p->tp.d_table, (float*)p->tp.d_state, B.n_streams, B.n, p->ld.hop, p->tp.L, p->tp.T, p->C, E};
            return aacg_truepeak_launch(Q, L.st) ? AACG_OK : not_served(p, "aacg_pcm_truepeak");
        });
        if (rc) return rc;
    }
    pipe_copy((const char*)L.d_res - ld16 - tp16, (char*)L.h_res - ld16 - tp16, tp16 + ld16 + p->res_cap16 + 16, L.st, true);      /* ... and the count is cleared for the lane's next batch (set to zero at create) */
    P_TRY(p, hipGetLastError(), AACG_ERR_NO_DEVICE);
    P_TRY(p, hipEventRecord(L.done, L.st), AACG_ERR_NO_DEVICE);
    L.busy = true; L.ticket = ++p->submitted; L.collect_pcm = B.pcm_out; L.collect_bytes = B.X.collect_copy ? (size_t)B.X.out_bytes : 0;
    L.user_results = B.results; L.user_refused = B.n_refused; L.n = B.n;
    /* the batch is enqueued: its streams' clocks and positions advance and their device state changes sides (a submission refused or
     * failed before this point has left them alone, and what its launch wrote lies in the buffers the slots do not read) */
    aacg_pipe::commit_resample(p->rs, B.rs); aacg_pipe::commit_features(p->ft, B.ft); aacg_pipe::commit_loudness(p->ld, B.ld);
    aacg_pipe::commit_limiter(p->lim, B.lim); aacg_pipe::commit_trim(p->tr, B.slots, B.tr_in); aacg_pipe::commit_conceal(p->cn, B.cn, B.plan != nullptr);
    /* the meter's destination is this batch's now, and the next submission names its own */
    L.ld_user = p->ld.out; L.ld_bytes = B.ld_floats * sizeof(float);
    L.tp_user = p->tp.out; L.tp_bytes = B.tp_floats * sizeof(float);
    if (p->ld.hop && p->ld.out_counts) for (uint32_t s = 0; s < B.n_streams; s++) p->ld.out_counts[s] = B.ld[s].n_out;
    p->ld.armed = p->tp.armed = false;
    *ticket = L.ticket;
    return AACG_OK;
}

/* One batch onto the next lane: aacg_pipeline_submit_ragged (pcm_out: host memory, dev null) and aacg_pipeline_submit_device (dev:
 * the caller's device memory, pcm_out null) are this, and differ where the PCM goes and nowhere else. */
int submit_batch(aacg_pipeline* p, batch_t B, uint64_t* ticket)
{
    int rc = check_batch(p, B);
    if (rc) return rc;
    B.set = (uint32_t)(p->submitted % (uint64_t)p->n_lanes);
    aacg_pipeline::lane_t& L = p->lane[B.set];
    if ((rc = finish_lane(p, L))) return rc;             /* step 2: the batch `lanes` submissions ago, if nobody has collected it */
    if (p->learn && (rc = learn_layouts(p, B.bytes, B.frames, B.slots, B.n_streams, B.frames_of))) return rc;
    /* the batch's layouts as its plan lists them (a stream without one has no unit in the plan) */
    p->batch_layout.resize(B.n_streams);
    for (uint32_t s = 0; s < B.n_streams; s++) p->batch_layout[s] = layout_of(p, B.slots[s]);
    if ((rc = stage_batch(p, L, B)) || (rc = choose_plan(p, L, B)) || (rc = enqueue_front(p, L, B)) || (rc = enqueue_transform(p, L, B))) return rc;
    return enqueue_out(p, L, B, ticket);
}

}  // namespace

int aacg_pipeline_submit_ragged(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                void* pcm_out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket)
{
    if (!p || !bytes || !frames || !slots || !frames_of || !pcm_out || !n_streams || !ticket) return AACG_ERR_INVALID_ARG;
    return submit_batch(p, {bytes, n_bytes, frames, slots, n_streams, frames_of, pcm_out, nullptr, results, n_refused}, ticket);
}

int aacg_pipeline_submit_device(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                const aacg_pcm_device_out* out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket)
{
    if (!p || !bytes || !frames || !slots || !frames_of || !n_streams || !ticket) return AACG_ERR_INVALID_ARG;
    return submit_batch(p, {bytes, n_bytes, frames, slots, n_streams, frames_of, nullptr, out, results, n_refused}, ticket);      /* (check_device_out refuses a null `out`) */
}

int aacg_pipeline_wait_device(aacg_pipeline* p, uint64_t ticket, void* hip_stream)
{
    if (!p || !ticket || ticket > p->submitted) { if (p) p->err = "aacg_pipeline_wait_device: no such ticket"; return AACG_ERR_INVALID_ARG; }
    aacg_pipeline::lane_t& L = p->lane[(ticket - 1) % (uint64_t)p->n_lanes];
    if (L.ticket != ticket || !L.busy) return AACG_OK;       /* collected, or a later batch has taken the lane and finished this one first */
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    const hipError_t st = hipEventQuery(L.done);
    if (st == hipSuccess) return AACG_OK;                   /* complete: nothing to wait for */
    if (st != hipErrorNotReady) P_TRY(p, st, AACG_ERR_NO_DEVICE);
    (void)hipGetLastError();
    P_TRY(p, hipStreamWaitEvent((hipStream_t)hip_stream, L.done, 0), AACG_ERR_NO_DEVICE);
    return AACG_OK;
}

int aacg_pipeline_submit(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                         const uint32_t* slots, uint32_t n_streams, uint32_t frames_per_stream,
                         void* pcm_out, aacg_parse_result* results, uint32_t* n_refused, uint64_t* ticket)
{
    if (!p || !bytes || !frames || !slots || !pcm_out || !n_streams || !frames_per_stream || !ticket) return AACG_ERR_INVALID_ARG;
    if ((int)n_streams > p->cfg.max_streams || (int)frames_per_stream > p->cfg.max_frames) { p->err = "batch larger than the pipeline was created for"; return AACG_ERR_CAPACITY; }
    p->rect_counts.assign(n_streams, frames_per_stream);      /* the rectangle: every stream the same count */
    return aacg_pipeline_submit_ragged(p, bytes, n_bytes, frames, slots, n_streams, p->rect_counts.data(), pcm_out, results, n_refused, ticket);
}

int aacg_pipeline_collect(aacg_pipeline* p, uint64_t ticket)
{
    if (!p || !ticket || ticket > p->submitted) return AACG_ERR_INVALID_ARG;
    aacg_pipeline::lane_t& L = p->lane[(ticket - 1) % (uint64_t)p->n_lanes];
    if (L.ticket != ticket) return AACG_OK;              /* a later batch has taken the lane: this one was finished then */
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    return finish_lane(p, L);
}

int aacg_pipeline_walk_submit(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* spans, uint32_t n_spans,
                              uint32_t max_frames, aacg_parse_frame* frames, aacg_walk_result* results, uint64_t* ticket)
{
    if (!p || !bytes || !spans || !n_spans || !max_frames || !frames || !results || !ticket) return AACG_ERR_INVALID_ARG;
    if (n_bytes >= (1u << 29)) { p->err = "aacg_pipeline_walk_submit: 2^29 bytes or more"; return AACG_ERR_INVALID_ARG; }
    for (uint32_t i = 0; i < n_spans; i++)
        if ((size_t)spans[i].byte_offset + spans[i].byte_length > n_bytes) { p->err = "a span points outside the byte buffer"; return AACG_ERR_INVALID_ARG; }
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    aacg_pipeline::walk_t& W = p->walk[p->walks_submitted % 2];
    int rc = finish_walk(p, W);                          /* the walk two submissions ago, if nobody has collected it */
    if (rc) return rc;
    if (!W.parser) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        rc = aacg_parser_create(p->cfg.device_ordinal, p->cfg.sample_index, p->entries.data(), p->counts, &W.parser);
        if (rc) { p->err = std::string("aacg_parser_create (walk): ") + (W.parser ? aacg_parser_last_error(W.parser) : ""); if (W.parser) aacg_parser_destroy(W.parser); W.parser = nullptr; return rc; }
        (void)aacg_parser_set_wait_limit_ms(W.parser, (uint32_t)(p->wait.limit_s * 1e3));
        P_TRY(p, hipStreamCreateWithPriority(&W.st, hipStreamNonBlocking, least), AACG_ERR_NO_DEVICE);
        P_TRY(p, hipEventCreateWithFlags(&W.done, hipEventDisableTiming), AACG_ERR_NO_DEVICE);
    }
    /* up: the bytes (16-byte aligned, zeros behind them) and the spans; down: the block table, then the per-span results */
    staging_t G;
    const size_t fr = (size_t)n_spans * max_frames * sizeof(aacg_parse_frame), fr16 = (fr + 15) & ~(size_t)15, rs = (size_t)n_spans * sizeof(aacg_walk_result);
    if ((rc = stage(p, &W.h_in, &W.d_in, &W.in_cap, bytes, n_bytes, spans, n_spans, 0, G))) return rc;
    if ((rc = grow_pair(p, &W.h_out, &W.d_out, &W.out_cap, fr16 + rs))) return rc;
    pipe_copy(W.h_in, W.d_in, G.up, W.st);
    rc = aacg_parse_walk_device(W.parser, W.d_in, (const aacg_parse_frame*)((char*)W.d_in + G.padded), n_spans, max_frames, (uint32_t)p->cfg.parse_options,
                                (aacg_parse_frame*)W.d_out, (aacg_walk_result*)((char*)W.d_out + fr16), W.st);
    if (rc) { p->err = std::string("aacg_parse_walk_device: ") + aacg_parser_last_error(W.parser); return rc; }
    pipe_copy(W.d_out, W.h_out, fr16 + ((rs + 15) & ~(size_t)15), W.st);
    P_TRY(p, hipGetLastError(), AACG_ERR_NO_DEVICE);
    P_TRY(p, hipEventRecord(W.done, W.st), AACG_ERR_NO_DEVICE);
    W.busy = true; W.ticket = ++p->walks_submitted; W.user_frames = frames; W.user_results = results;
    W.frames_bytes = fr; W.results_bytes = rs; W.results_at = fr16;
    *ticket = W.ticket;
    return AACG_OK;
}

int aacg_pipeline_walk_collect(aacg_pipeline* p, uint64_t ticket)
{
    if (!p || !ticket || ticket > p->walks_submitted) return AACG_ERR_INVALID_ARG;
    aacg_pipeline::walk_t& W = p->walk[(ticket - 1) % 2];
    if (W.ticket != ticket) return AACG_OK;              /* a later walk has taken the slot: this one was finished then */
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    return finish_walk(p, W);
}

int aacg_pipeline_decode(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                         const uint32_t* slots, uint32_t n_streams, uint32_t frames_per_stream,
                         void* pcm_out, aacg_parse_result* results, uint32_t* n_refused)
{
    uint64_t t = 0;
    int rc = aacg_pipeline_submit(p, bytes, n_bytes, frames, slots, n_streams, frames_per_stream, pcm_out, results, n_refused, &t);
    return rc ? rc : aacg_pipeline_collect(p, t);
}

int aacg_pipeline_decode_ragged(aacg_pipeline* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames,
                                const uint32_t* slots, uint32_t n_streams, const uint32_t* frames_of,
                                void* pcm_out, aacg_parse_result* results, uint32_t* n_refused)
{
    uint64_t t = 0;
    int rc = aacg_pipeline_submit_ragged(p, bytes, n_bytes, frames, slots, n_streams, frames_of, pcm_out, results, n_refused, &t);
    return rc ? rc : aacg_pipeline_collect(p, t);
}

int aacg_pipeline_stream_window_shape(aacg_pipeline* p, uint32_t slot, uint8_t shapes[8])
{
    if (!p || !shapes || (int)slot >= p->cfg.max_streams) return AACG_ERR_INVALID_ARG;
    P_TRY(p, hipSetDevice(p->cfg.device_ordinal), AACG_ERR_NO_DEVICE);
    /* what is in flight for the slot is finished first (aacg_get_window_shape waits for the engine's launches and the lanes' streams) */
    for (int k = 0; k < p->n_lanes; k++) { int rc = finish_lane(p, p->lane[k]); if (rc) return rc; }
    std::memset(shapes, 0, 8);
    for (uint32_t c = 0; c < p->C; c++) {
        int rc = aacg_get_window_shape(p->engine, slot, c, &shapes[c]);
        if (rc) return engine_fail(p, "", rc);
    }
    return AACG_OK;
}

uint64_t aacg_pipeline_plan_builds(const aacg_pipeline* p) { return p ? p->plan_builds : 0; }

int aacg_pipeline_launch_counts(const aacg_pipeline* p, uint64_t* shaped, uint64_t* chained, uint64_t* launches)
{
    if (!p) return AACG_ERR_INVALID_ARG;
    if (shaped) *shaped = p->shaped_batches;
    if (chained) *chained = aacg_pipeline_chained(p->engine);
    if (launches) *launches = p->launches;
    return AACG_OK;
}

int aacg_pipeline_stream_layout(aacg_pipeline* p, uint32_t slot, uint8_t element_channels[8], uint32_t* kept)
{
    if (!p || (int)slot >= p->cfg.max_streams) return AACG_ERR_INVALID_ARG;
    const aacg_pipeline::layout_t lay = layout_of(p, slot);
    if (element_channels) std::memcpy(element_channels, lay.nch, 8);
    if (kept) *kept = lay.kept;
    return (int)lay.n;
}

}  // extern "C"
