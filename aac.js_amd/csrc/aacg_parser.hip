/*
 * aacg_parser.hip — the device front end behind include/aacgpu.h's aacg_parser_* / aacg_parse_* entry points:
 * the kernel (one lane per frame, aacg_parse.h) and its host plumbing.  Independent of aacg_engine: it shares
 * record formats with it, no state.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "aacg_parse.h"
#include "aacg_host.h"
#include "aacg_wait.h"

extern "C" DP_KERNEL(AACG_PARSE_WG_LARGE, 1)
void aacg_parse_frames(const aacg_parse_params P) { aacg_parse::parse_body(P); }

/* one wave per workgroup: a span is a few thousand serial code words, and a walk of a few hundred spans should spread over as
 * many CUs as it has waves */
#define AACG_WALK_WG 64
extern "C" DP_KERNEL(AACG_WALK_WG, 1)
void aacg_parse_walk_spans(const aacg_walk_params W) { aacg_parse::walk_body(W); }

/* Lane order: a counting sort of the frames by length, longest first (8-byte buckets).  Three small launches. */
__device__ __forceinline__ uint32_t length_bucket(uint32_t bytes)
{
    const uint32_t k = bytes >> 3;
    return AACG_PARSE_BUCKETS - 1u - (k < AACG_PARSE_BUCKETS ? k : AACG_PARSE_BUCKETS - 1u);
}
/* one frame per thread; the buckets are counted in LDS first: frames cluster in a few hundred buckets, and 64 k global
 * atomics on those took 70 us per pass */
extern "C" __global__ __launch_bounds__(256)
void aacg_parse_order_count(const aacg_parse_frame* frames, uint32_t n, uint32_t* hist)
{
    __shared__ uint32_t cnt[AACG_PARSE_BUCKETS];
    for (uint32_t b = threadIdx.x; b < AACG_PARSE_BUCKETS; b += 256u) cnt[b] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) atomicAdd(&cnt[length_bucket(frames[i].byte_length)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < AACG_PARSE_BUCKETS; b += 256u) if (cnt[b]) atomicAdd(&hist[b], cnt[b]);
}
extern "C" __global__ __launch_bounds__(AACG_PARSE_BUCKETS)
void aacg_parse_order_scan(uint32_t* hist)
{
    __shared__ uint32_t sum[AACG_PARSE_BUCKETS];
    const uint32_t t = threadIdx.x, mine = hist[t];
    sum[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < AACG_PARSE_BUCKETS; d <<= 1) {
        const uint32_t add = t >= d ? sum[t - d] : 0u;
        __syncthreads();
        sum[t] += add;
        __syncthreads();
    }
    hist[t] = sum[t] - mine;                               /* exclusive: where the bucket starts */
}
extern "C" __global__ __launch_bounds__(256)
void aacg_parse_order_fill(const aacg_parse_frame* frames, uint32_t n, uint32_t* next, uint32_t* order, uint32_t n_wg, uint32_t waves_per_wg)
{
    __shared__ uint32_t cnt[AACG_PARSE_BUCKETS];          /* the block's frames per bucket, then where its share starts */
    for (uint32_t b = threadIdx.x; b < AACG_PARSE_BUCKETS; b += 256u) cnt[b] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t bucket = 0, rank = 0;
    if (i < n) { bucket = length_bucket(frames[i].byte_length); rank = atomicAdd(&cnt[bucket], 1u); }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < AACG_PARSE_BUCKETS; b += 256u) if (cnt[b]) cnt[b] = atomicAdd(&next[b], cnt[b]);
    __syncthreads();
    if (i < n) {
        /* sorted position -> lane: piece c of 64 neighbours becomes wave c / n_wg of workgroup c % n_wg */
        const uint32_t pos = cnt[bucket] + rank, piece = pos >> 6;
        order[((piece % n_wg) * waves_per_wg + piece / n_wg) * 64u + (pos & 63u)] = i;
    }
}

/* Small batches (a resident pipeline's 4096 frames): everything in front of the parse kernel in ONE launch.  On a stream that
 * carries a batch through a dozen small steps every step costs its launch gap (5-10 us, and up to 60 when a transform launch of
 * the highest priority holds the dispatcher: profiles/r06_resident_budget.txt), and five of them were memsets, three the
 * counting sort.  Block 0 sorts (count, scan, place: the three kernels above in one workgroup's LDS); the other blocks clear
 * the regions the parser promises zeroed.  Regions are multiples of 16 bytes. */
#define AACG_PARSE_PREPARE_MAX 16384u
struct aacg_clear_regions { void* at[4]; unsigned long long n16[4]; };
extern "C" __global__ __launch_bounds__(1024)
void aacg_parse_prepare(const aacg_clear_regions C, const aacg_parse_frame* frames, uint32_t n, uint32_t* order, uint32_t lanes, uint32_t n_wg, uint32_t waves_per_wg)
{
    const uint32_t t = threadIdx.x;
    if (order && blockIdx.x == 0) {
        __shared__ uint32_t cnt[AACG_PARSE_BUCKETS], sum[AACG_PARSE_BUCKETS];
        for (uint32_t i = t; i < lanes; i += 1024u) order[i] = 0xffffffffu;        /* idle lanes */
        cnt[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += 1024u) atomicAdd(&cnt[length_bucket(frames[i].byte_length)], 1u);
        __syncthreads();
        const uint32_t mine = cnt[t];
        sum[t] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < AACG_PARSE_BUCKETS; d <<= 1) {
            const uint32_t add = t >= d ? sum[t - d] : 0u;
            __syncthreads();
            sum[t] += add;
            __syncthreads();
        }
        cnt[t] = sum[t] - mine;                                                      /* where the bucket starts */
        __syncthreads();
        for (uint32_t i = t; i < n; i += 1024u) {
            const uint32_t pos = atomicAdd(&cnt[length_bucket(frames[i].byte_length)], 1u), piece = pos >> 6;
            order[((piece % n_wg) * waves_per_wg + piece / n_wg) * 64u + (pos & 63u)] = i;
        }
        return;
    }
    const uint32_t first = order ? 1u : 0u, blocks = gridDim.x - first;
    if (!blocks) return;
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const v4u zero = {0u, 0u, 0u, 0u};
    for (int r = 0; r < 4; r++) {
        v4u* d = (v4u*)C.at[r];
        const size_t n16 = (size_t)C.n16[r];
        for (size_t i = (size_t)(blockIdx.x - first) * 1024u + t; i < n16; i += (size_t)blocks * 1024u) d[i] = zero;
    }
}

/* the device buffers, grown on demand: the host round trips' (aacg_parse_batch's seven, aacg_parse_walk's four) and the lane order */
enum { B_BYTES, B_FRAMES, B_UNITS, B_Q, B_META, B_TNS, B_RESULTS, W_BYTES, W_SPANS, W_BLOCKS, W_RESULTS, ORDER, N_BUF };

struct aacg_parser {
    int device = 0;
    hipStream_t stream = nullptr;
    aacg_parse_tables* d_tab = nullptr;
    size_t lds_bytes = 0;
    uint32_t lut_words = 0;
    int n_cus = 256;
    void* d_buf[N_BUF] = {};          /* (ORDER: the lane order + the bucket counters behind it) */
    size_t cap[N_BUF] = {};
    hipEvent_t order_free = nullptr;  /* recorded behind every launch: the lane-order scratch may be rewritten after it */
    hipStream_t last_stream = nullptr;
    aacg_wait_policy wait;            /* aacg_parse_batch's host waits are bounded (aacg_wait.h): AACG_ERR_TIMEOUT */
    std::string err;
};

namespace {

int fail(aacg_parser* p, int rc, const std::string& m) { if (p) p->err = m; return rc; }
int hip_fail(aacg_parser* p, hipError_t e, const char* what) { return fail(p, AACG_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }
#define HIPCHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(p, e_, #call); } while (0)

int grow(aacg_parser* p, int i, size_t bytes)
{
    if (bytes <= p->cap[i]) return AACG_OK;
    if (p->d_buf[i]) (void)hipFree(p->d_buf[i]);
    p->d_buf[i] = nullptr; p->cap[i] = 0;
    if (hipMalloc(&p->d_buf[i], bytes) != hipSuccess) return fail(p, AACG_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    p->cap[i] = bytes;
    return AACG_OK;
}

/* The lane order and the clearing in front of a parse or walk kernel on stream s: P.order is set (sorted: the parser's scratch,
 * grown here; otherwise null: table order), the regions that have an address are zeroed.  One launch (aacg_parse_prepare) when
 * every region is a multiple of 16 bytes at a multiple of 16 and there are at most AACG_PARSE_PREPARE_MAX frames, else memsets and
 * the three sorting kernels.  grid x P.wg_threads are the lanes of the kernel that follows. */
struct region { void* at; size_t bytes; };
int order_and_clear(aacg_parser* p, aacg_parse_params& P, bool sorted, unsigned grid, const region* regions, int n_regions, hipStream_t s)
{
    const size_t lanes = (size_t)grid * P.wg_threads;
    int rc = sorted ? grow(p, ORDER, (lanes + AACG_PARSE_BUCKETS) * sizeof(uint32_t)) : AACG_OK;
    if (rc) return rc;
    /* The lane-order scratch belongs to the parser, not to the launch: a launch on another stream first waits for the
     * previous launch's kernels (same stream: ordered anyway).  Two streams may therefore alternate on one parser. */
    if (p->last_stream && p->last_stream != s) HIPCHECK(hipStreamWaitEvent(s, p->order_free, 0));
    uint32_t* const order = sorted ? (uint32_t*)p->d_buf[ORDER] : nullptr;
    P.order = order;
    bool fused = P.n_frames <= AACG_PARSE_PREPARE_MAX;
    aacg_clear_regions C = {};
    size_t total16 = 0;
    for (int i = 0; i < n_regions; i++) {
        const region& r = regions[i];
        if (!r.at) continue;
        if (((uintptr_t)r.at | r.bytes) & 15u) fused = false;
        C.at[i] = r.at; C.n16[i] = r.bytes / 16u; total16 += r.bytes / 16u;
    }
    if (fused) {                                         /* one launch in front of the kernel (aacg_parse_prepare) */
        /* clearing blocks: four 16-byte stores per thread, 512 at the most, and 0 when there is nothing to clear (the walk): its
         * prepare launch is the sorting block alone, and with nothing to sort either there is no launch */
        const size_t clearing = (total16 + 4095u) / 4096u;
        const unsigned blocks = (unsigned)(clearing > 512u ? 512u : clearing) + (sorted ? 1u : 0u);
        if (blocks) hipLaunchKernelGGL(aacg_parse_prepare, dim3(blocks), dim3(1024), 0, s, C, P.frames, P.n_frames, order, (uint32_t)lanes, grid, P.wg_threads / 64u);
        return AACG_OK;
    }
    for (int i = 0; i < n_regions; i++) if (regions[i].at) HIPCHECK(hipMemsetAsync(regions[i].at, 0, regions[i].bytes, s));
    if (sorted) {
        uint32_t* hist = order + lanes;
        const unsigned blocks = (P.n_frames + 255u) / 256u;
        HIPCHECK(hipMemsetAsync(order, 0xff, lanes * sizeof(uint32_t), s));
        HIPCHECK(hipMemsetAsync(hist, 0, AACG_PARSE_BUCKETS * sizeof(uint32_t), s));
        hipLaunchKernelGGL(aacg_parse_order_count, dim3(blocks), dim3(256), 0, s, P.frames, P.n_frames, hist);
        hipLaunchKernelGGL(aacg_parse_order_scan, dim3(1), dim3(AACG_PARSE_BUCKETS), 0, s, hist);
        hipLaunchKernelGGL(aacg_parse_order_fill, dim3(blocks), dim3(256), 0, s, P.frames, P.n_frames, hist, order, grid, P.wg_threads / 64u);
    }
    return AACG_OK;
}

/* behind the kernel that reads the lane order: the scratch may be rewritten after order_free */
int launched(aacg_parser* p, hipStream_t s)
{
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(p->order_free, s));
    p->last_stream = s;
    return AACG_OK;
}

int launch(aacg_parser* p, aacg_parse_params& P, hipStream_t s)
{
    /* up to one small workgroup per CU: stage the frames in LDS; beyond that the rate matters more than the time per
     * frame, and 16 waves per CU reading in place overlap what one wave per SIMD cannot (AACG_PARSE_WG overrides) */
    const char* env = std::getenv("AACG_PARSE_WG");
    P.wg_threads = env ? (uint32_t)std::atoi(env) : (P.n_frames <= (uint32_t)p->n_cus * AACG_PARSE_WG_SMALL ? AACG_PARSE_WG_SMALL : P.n_frames <= (uint32_t)p->n_cus * 512u ? 512u : AACG_PARSE_WG_LARGE);
    if (P.wg_threads != AACG_PARSE_WG_SMALL && P.wg_threads != 512 && P.wg_threads != AACG_PARSE_WG_LARGE) return fail(p, AACG_ERR_INVALID_ARG, "AACG_PARSE_WG must be 256, 512 or 1024");
    while (AACG_PARSE_LDS_FIXED(p->lut_words, P.wg_threads) > p->lds_bytes) P.wg_threads /= 2;      /* very large tables */
    P.arena_bytes = (uint32_t)(p->lds_bytes - AACG_PARSE_LDS_FIXED(p->lut_words, P.wg_threads));
    const unsigned grid = (P.n_frames + P.wg_threads - 1) / P.wg_threads;
    /* Frames of similar length into the same wave, and long and short waves onto every CU alike (AACG_PARSE_SORT=0: table
     * order).  Measured with frame lengths spread 44..1186 bytes: 16 k frames 1.40 -> 0.89 ms, 64 k 1.36 -> 0.94. */
    static const bool sort_enabled = [] { const char* v = std::getenv("AACG_PARSE_SORT"); return !(v && v[0] == '0'); }();
    /* what the parser promises zeroed: the spectra (positions outside the coded bands), the band words (only the coded ones are
     * written), TNS records, and the unit records of refused frames and of element slots beyond a frame's count (never stale memory) */
    const region regions[4] = {
        { (P.options & AACG_PARSE_SKIP_ZERO_FILL) ? nullptr : (void*)P.q, (size_t)P.n_frames * P.max_channels * 1024u * sizeof(int16_t) },
        { (void*)P.meta, (size_t)P.n_frames * P.max_channels * sizeof(aacg_band_meta) },
        { (void*)P.tns, (size_t)P.n_frames * P.max_channels * sizeof(aacg_tns_info) },
        { (void*)P.units, (size_t)P.n_frames * P.max_units * sizeof(aacg_unit_desc) } };
    int rc = order_and_clear(p, P, sort_enabled && P.n_frames > 64u, grid, regions, 4, s);
    if (rc) return rc;
    hipLaunchKernelGGL(aacg_parse_frames, dim3(grid), dim3(P.wg_threads), p->lds_bytes, s, P);
    return launched(p, s);
}

/* The walk: spans sorted by length, longest first (aacg_parse_prepare with nothing to clear, or the three sorting kernels for
 * very many spans), then one lane per span.  Spans of 8 KiB and more share the longest bucket.  AACG_PARSE_SORT is the frame
 * parse's switch, not the walk's. */
int walk_launch(aacg_parser* p, aacg_walk_params& W, hipStream_t s)
{
    aacg_parse_params& P = W.P;
    P.wg_threads = AACG_WALK_WG;
    P.arena_bytes = 0;
    const unsigned grid = (P.n_frames + AACG_WALK_WG - 1) / AACG_WALK_WG;
    int rc = order_and_clear(p, P, P.n_frames > 64u, grid, nullptr, 0, s);
    if (rc) return rc;
    hipLaunchKernelGGL(aacg_parse_walk_spans, dim3(grid), dim3(AACG_WALK_WG), AACG_PARSE_LDS_FIXED(p->lut_words, AACG_WALK_WG), s, W);
    return launched(p, s);
}

void walk_params(aacg_parser* p, aacg_walk_params& W, const void* d_bytes, const aacg_parse_frame* d_spans, uint32_t n_spans,
                 uint32_t max_frames, uint32_t options, aacg_parse_frame* d_frames, aacg_walk_result* d_results)
{
    std::memset(&W, 0, sizeof W);
    W.P.bytes = (const uint32_t*)d_bytes; W.P.frames = d_spans; W.P.tab = p->d_tab; W.P.n_frames = n_spans;
    W.P.options = options & ~AACG_PARSE_SKIP_ZERO_FILL;
    W.blocks = d_frames; W.results = d_results; W.max_frames = max_frames;
}

/* The host round trips (aacg_parse_batch, aacg_parse_walk) on the parser's own stream.  Up: the bytes with AACG_PARSE_PAD_BYTES
 * readable zeros behind them, and the frame or span table. */
size_t padded_bytes(size_t n_bytes) { return (n_bytes + 15u) / 16u * 16u + AACG_PARSE_PAD_BYTES; }
int upload(aacg_parser* p, int b_bytes, const uint8_t* bytes, size_t n_bytes, int b_table, const aacg_parse_frame* table, uint32_t n)
{
    hipStream_t s = p->stream;
    const size_t padded = padded_bytes(n_bytes);
    const size_t tail = padded < AACG_PARSE_PAD_BYTES + 16u ? padded : AACG_PARSE_PAD_BYTES + 16u;      /* zeros behind the last byte */
    HIPCHECK(hipMemsetAsync((char*)p->d_buf[b_bytes] + padded - tail, 0, tail, s));
    HIPCHECK(hipMemcpyAsync(p->d_buf[b_bytes], bytes, n_bytes, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(p->d_buf[b_table], table, n * sizeof(aacg_parse_frame), hipMemcpyHostToDevice, s));
    return AACG_OK;
}
/* the bounded wait for the parser's stream: AACG_ERR_TIMEOUT says what did not complete */
int wait_for(aacg_parser* p, const char* entry, const char* what)
{
    const hipError_t st = aacg_wait_stream(p->stream, p->wait);
    if (st == hipErrorNotReady) return fail(p, AACG_ERR_TIMEOUT, std::string(entry) + ": the " + what + " did not complete within the wait limit");
    HIPCHECK(st);
    return AACG_OK;
}
/* Down, behind the bounded wait for the kernel: the copies into the caller's (pageable) memory wait inside the runtime, and a
 * device that has just answered will carry them out.  Buffer first + i goes to to[i]; null: not an output, or one not asked for. */
int download(aacg_parser* p, const char* entry, int first, void* const* to, const size_t* sizes, int n)
{
    for (int i = 0; i < n; i++) if (to[i]) HIPCHECK(hipMemcpyAsync(to[i], p->d_buf[first + i], sizes[i], hipMemcpyDeviceToHost, p->stream));
    return wait_for(p, entry, "copies back");
}

}  // namespace

extern "C" {

const char* aacg_parse_kernel_name(void) { return "aacg_parse_frames"; }
const char* aacg_parser_last_error(const aacg_parser* p) { return p ? p->err.c_str() : "null parser"; }

const char* aacg_parse_status_string(int status)
{
    static const char* const text[] = {
        "ok", "Insufficient data", "Invalid band type: 12", "Too many bands", "Scalefactor out of range",
        "Pulse tool not allowed in eight short sequence.", "Pulse SWB or offset out of range", "TODO: add pulse data",
        "TNS filter out of range", "Prediction not implemented.", "TODO: decode gain control/SSR", "TODO: PCE_ELEMENT",
        "maxSFB out of range", "Reserved ms mask type: 3", "Huffman: escape sequence too long",
        "more elements or channels in the frame than allowed for",
        "the frame's elements are not the ones its stream began with" };
    return status >= 0 && status < (int)(sizeof text / sizeof *text) ? text[status] : "unknown status";
}

int aacg_parser_create(int device_ordinal, int sample_index, const aacg_code_entry* entries, const uint32_t counts[12], aacg_parser** out)
{
    if (!out) return AACG_ERR_INVALID_ARG;
    *out = nullptr;
    aacg_parser* p = new aacg_parser;
    p->device = device_ordinal;
    std::vector<aacg_parse_tables> tab(1);
    int rc = aacg_parse_build_tables(sample_index, entries, counts, tab.data(), &p->err);
    if (rc == AACG_OK && hipSetDevice(device_ordinal) != hipSuccess) rc = fail(p, AACG_ERR_NO_DEVICE, "hipSetDevice failed");
    if (rc == AACG_OK) {
        p->lds_bytes = 160u * 1024u;                 /* one workgroup per CU: what the tables leave is the frames' staging arena */
        p->lut_words = tab[0].lut_words;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) p->n_cus = prop.multiProcessorCount;
        if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&p->order_free, hipEventDisableTiming) != hipSuccess ||
            hipMalloc((void**)&p->d_tab, sizeof(aacg_parse_tables)) != hipSuccess ||
            hipMemcpy(p->d_tab, tab.data(), sizeof(aacg_parse_tables), hipMemcpyHostToDevice) != hipSuccess ||
            hipFuncSetAttribute((const void*)aacg_parse_frames, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->lds_bytes) != hipSuccess ||
            hipFuncSetAttribute((const void*)aacg_parse_walk_spans, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)AACG_PARSE_LDS_FIXED(p->lut_words, AACG_WALK_WG)) != hipSuccess)
            rc = fail(p, AACG_ERR_NO_DEVICE, "HIP setup of the parser failed");
    }
    /* on failure the object is still returned, so that aacg_parser_last_error() can say why */
    *out = p;
    return rc;
}

void aacg_parser_destroy(aacg_parser* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    /* its own stream and the last caller's stream it launched on, bounded; a device that does not answer keeps the memory */
    if ((p->stream && aacg_wait_stream(p->stream, p->wait) == hipErrorNotReady) ||
        (p->last_stream && p->last_stream != p->stream && aacg_wait_stream(p->last_stream, p->wait) == hipErrorNotReady)) {
        std::fprintf(stderr, "aacgpu: aacg_parser_destroy: the GPU did not answer within the wait limit — device memory of this parser is left allocated\n");
        delete p;
        return;
    }
    (void)hipGetLastError();
    if (p->order_free) (void)hipEventDestroy(p->order_free);
    for (int i = 0; i < N_BUF; i++) if (p->d_buf[i]) (void)hipFree(p->d_buf[i]);
    if (p->d_tab) (void)hipFree(p->d_tab);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

int aacg_parse_device(aacg_parser* p, const void* d_bytes, const aacg_parse_frame* d_frames, uint32_t n_frames,
                      uint32_t max_units, uint32_t max_channels, uint32_t options,
                      aacg_unit_desc* d_units, int16_t* d_q, aacg_band_meta* d_meta, aacg_tns_info* d_tns,
                      aacg_parse_result* d_results, void* hip_stream)
{
    if (!p || !p->d_tab) return AACG_ERR_INVALID_ARG;
    if (!n_frames) return AACG_OK;
    if (!d_bytes || !d_frames || !d_units || !d_q || !d_meta || !d_results || !max_units || !max_channels || ((uintptr_t)d_bytes & 15u))
        return fail(p, AACG_ERR_INVALID_ARG, "aacg_parse_device: null or misaligned argument");
    HIPCHECK(hipSetDevice(p->device));
    aacg_parse_params P;
    P.bytes = (const uint32_t*)d_bytes; P.frames = d_frames; P.tab = p->d_tab; P.units = d_units; P.q = d_q; P.meta = d_meta;
    P.tns = d_tns; P.results = d_results; P.n_frames = n_frames; P.max_units = max_units; P.max_channels = max_channels; P.options = options;
    return launch(p, P, hip_stream ? (hipStream_t)hip_stream : p->stream);
}

int aacg_parse_batch(aacg_parser* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* frames, uint32_t n_frames,
                     uint32_t max_units, uint32_t max_channels, uint32_t options,
                     aacg_unit_desc* units, int16_t* q, aacg_band_meta* meta, aacg_tns_info* tns, aacg_parse_result* results)
{
    if (!p || !p->d_tab) return AACG_ERR_INVALID_ARG;
    if (!n_frames) return AACG_OK;
    if (!bytes || !frames || !units || !q || !meta || !results || !max_units || !max_channels)
        return fail(p, AACG_ERR_INVALID_ARG, "aacg_parse_batch: null argument");
    for (uint32_t f = 0; f < n_frames; f++)
        if ((size_t)frames[f].byte_offset + frames[f].byte_length > n_bytes) return fail(p, AACG_ERR_INVALID_ARG, "frame " + std::to_string(f) + " lies outside the byte buffer");
    HIPCHECK(hipSetDevice(p->device));
    const size_t blocks = (size_t)n_frames * max_channels;
    const size_t sizes[7] = { padded_bytes(n_bytes), n_frames * sizeof(aacg_parse_frame), (size_t)n_frames * max_units * sizeof(aacg_unit_desc),
                              blocks * 1024u * sizeof(int16_t), blocks * sizeof(aacg_band_meta), tns ? blocks * sizeof(aacg_tns_info) : 0,
                              n_frames * sizeof(aacg_parse_result) };
    int rc = AACG_OK;
    for (int i = 0; i < 7; i++) if (sizes[i] && (rc = grow(p, B_BYTES + i, sizes[i]))) return rc;
    if ((rc = upload(p, B_BYTES, bytes, n_bytes, B_FRAMES, frames, n_frames))) return rc;
    aacg_parse_params P;
    P.bytes = (const uint32_t*)p->d_buf[B_BYTES]; P.frames = (const aacg_parse_frame*)p->d_buf[B_FRAMES]; P.tab = p->d_tab;
    P.units = (aacg_unit_desc*)p->d_buf[B_UNITS]; P.q = (int16_t*)p->d_buf[B_Q]; P.meta = (aacg_band_meta*)p->d_buf[B_META];
    P.tns = tns ? (aacg_tns_info*)p->d_buf[B_TNS] : nullptr; P.results = (aacg_parse_result*)p->d_buf[B_RESULTS];
    P.n_frames = n_frames; P.max_units = max_units; P.max_channels = max_channels; P.options = options & ~AACG_PARSE_SKIP_ZERO_FILL;
    if ((rc = launch(p, P, p->stream))) return rc;
    void* const to[7] = { nullptr, nullptr, units, q, meta, tns, results };
    if ((rc = wait_for(p, "aacg_parse_batch", "parse kernel")) == AACG_ERR_TIMEOUT) p->err += " (" + std::to_string(n_frames) + " frames, workgroups of " + std::to_string(P.wg_threads) + ")";
    if (rc) return rc;
    return download(p, "aacg_parse_batch", B_BYTES, to, sizes, 7);
}

int aacg_parse_walk_device(aacg_parser* p, const void* d_bytes, const aacg_parse_frame* d_spans, uint32_t n_spans,
                           uint32_t max_frames, uint32_t options, aacg_parse_frame* d_frames, aacg_walk_result* d_results,
                           void* hip_stream)
{
    if (!p || !p->d_tab) return AACG_ERR_INVALID_ARG;
    if (!n_spans) return AACG_OK;
    if (!d_bytes || !d_spans || !d_frames || !d_results || !max_frames || ((uintptr_t)d_bytes & 15u))
        return fail(p, AACG_ERR_INVALID_ARG, "aacg_parse_walk_device: null, zero or misaligned argument");
    HIPCHECK(hipSetDevice(p->device));
    aacg_walk_params W;
    walk_params(p, W, d_bytes, d_spans, n_spans, max_frames, options, d_frames, d_results);
    return walk_launch(p, W, hip_stream ? (hipStream_t)hip_stream : p->stream);
}

int aacg_parse_walk(aacg_parser* p, const uint8_t* bytes, size_t n_bytes, const aacg_parse_frame* spans, uint32_t n_spans,
                    uint32_t max_frames, uint32_t options, aacg_parse_frame* frames, aacg_walk_result* results)
{
    if (!p || !p->d_tab) return AACG_ERR_INVALID_ARG;
    if (!n_spans) return AACG_OK;
    if (!bytes || !spans || !frames || !results || !max_frames) return fail(p, AACG_ERR_INVALID_ARG, "aacg_parse_walk: null or zero argument");
    if (n_bytes >= (1u << 29)) return fail(p, AACG_ERR_INVALID_ARG, "aacg_parse_walk: 2^29 bytes or more (bit positions are 32-bit)");
    for (uint32_t f = 0; f < n_spans; f++)
        if ((size_t)spans[f].byte_offset + spans[f].byte_length > n_bytes) return fail(p, AACG_ERR_INVALID_ARG, "span " + std::to_string(f) + " lies outside the byte buffer");
    HIPCHECK(hipSetDevice(p->device));
    const size_t sizes[4] = { padded_bytes(n_bytes), n_spans * sizeof(aacg_parse_frame), (size_t)n_spans * max_frames * sizeof(aacg_parse_frame),
                              n_spans * sizeof(aacg_walk_result) };
    int rc = AACG_OK;
    for (int i = 0; i < 4; i++) if ((rc = grow(p, W_BYTES + i, sizes[i]))) return rc;
    if ((rc = upload(p, W_BYTES, bytes, n_bytes, W_SPANS, spans, n_spans))) return rc;
    HIPCHECK(hipMemsetAsync(p->d_buf[W_BLOCKS], 0, sizes[2], p->stream));        /* the slots beyond a span's count read as zero */
    aacg_walk_params W;
    walk_params(p, W, p->d_buf[W_BYTES], (const aacg_parse_frame*)p->d_buf[W_SPANS], n_spans, max_frames, options, (aacg_parse_frame*)p->d_buf[W_BLOCKS], (aacg_walk_result*)p->d_buf[W_RESULTS]);
    if ((rc = walk_launch(p, W, p->stream))) return rc;
    void* const to[4] = { nullptr, nullptr, frames, results };
    if ((rc = wait_for(p, "aacg_parse_walk", "walk kernel")) == AACG_ERR_TIMEOUT) p->err += " (" + std::to_string(n_spans) + " spans)";
    if (rc) return rc;
    return download(p, "aacg_parse_walk", W_BYTES, to, sizes, 4);
}

int aacg_parser_set_wait_limit_ms(aacg_parser* p, uint32_t ms)
{
    if (!p || !ms) return AACG_ERR_INVALID_ARG;
    p->wait.limit_s = ms * 1e-3;
    return AACG_OK;
}

}  // extern "C"
