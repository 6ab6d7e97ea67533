/*
 * aacgpu_napi.c — N-API (node_api.h, N-API <= v8) binding of the C ABI in include/aacgpu.h.
 *
 * This is the FFI layer the JavaScript host (aac.js_amd/js) uses in place of the reference's
 * in-process  this.process(elements) + interleave  (src/decoder.js:201-215).  The addon itself is
 * plain C (gcc); it dlopen()s libaacgpu.so, so it builds on machines without hipcc and fails
 * loudly at load time if the HIP library is absent.  Non-zero status codes become thrown Errors,
 * the convention Aurora's Decoder.decode() already expects from readChunk.
 */
#include <node_api.h>

#include <dlfcn.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/aacgpu.h"

static struct {
    void* dl;
    int  (*create)(const aacg_config*, aacg_engine**);
    void (*destroy)(aacg_engine*);
    const char* (*last_error)(const aacg_engine*);
    int  (*abi_version)(void);
    int  (*reset_stream)(aacg_engine*, uint32_t);
    int  (*get_overlap)(aacg_engine*, uint32_t, uint32_t, float*);
    int  (*set_overlap)(aacg_engine*, uint32_t, uint32_t, const float*);
    int  (*decode_batch)(aacg_engine*, const aacg_unit_desc*, uint32_t, const void*, uint32_t,
                         const aacg_band_meta*, uint32_t, void*, size_t);
    int  (*submit)(aacg_engine*, const aacg_unit_desc*, uint32_t, const void*, uint32_t,
                   const aacg_band_meta*, uint32_t, void*, size_t, uint64_t*);
    int  (*wait)(aacg_engine*, uint64_t);
    int  (*decode_batch_ex)(aacg_engine*, const aacg_batch*);
    int  (*decode_batch_tns)(aacg_engine*, const aacg_unit_desc*, uint32_t, const void*, uint32_t,
                             const aacg_band_meta*, uint32_t, const aacg_tns_info*, uint32_t, void*, size_t);
    int  (*submit_tns)(aacg_engine*, const aacg_unit_desc*, uint32_t, const void*, uint32_t,
                       const aacg_band_meta*, uint32_t, const aacg_tns_info*, uint32_t, void*, size_t, uint64_t*);
    int  (*parser_create)(int, int, const aacg_code_entry*, const uint32_t*, aacg_parser**);
    void (*parser_destroy)(aacg_parser*);
    const char* (*parser_last_error)(const aacg_parser*);
    const char* (*parse_status_string)(int);
    int  (*parse_batch)(aacg_parser*, const uint8_t*, size_t, const aacg_parse_frame*, uint32_t, uint32_t, uint32_t, uint32_t,
                        aacg_unit_desc*, int16_t*, aacg_band_meta*, aacg_tns_info*, aacg_parse_result*);
    int  (*pipeline_create)(const aacg_pipeline_config*, const aacg_code_entry*, const uint32_t*, aacg_pipeline**);
    void (*pipeline_destroy)(aacg_pipeline*);
    const char* (*pipeline_last_error)(const aacg_pipeline*);
    int  (*pipeline_reset_stream)(aacg_pipeline*, uint32_t);
    int  (*pipeline_stream_window_shape)(aacg_pipeline*, uint32_t, uint8_t*);
    int  (*pipeline_decode)(aacg_pipeline*, const uint8_t*, size_t, const aacg_parse_frame*, const uint32_t*, uint32_t, uint32_t,
                            void*, aacg_parse_result*, uint32_t*);
    int  (*pipeline_submit)(aacg_pipeline*, const uint8_t*, size_t, const aacg_parse_frame*, const uint32_t*, uint32_t, uint32_t,
                            void*, aacg_parse_result*, uint32_t*, uint64_t*);
    int  (*pipeline_collect)(aacg_pipeline*, uint64_t);
    int  (*pipeline_decode_ragged)(aacg_pipeline*, const uint8_t*, size_t, const aacg_parse_frame*, const uint32_t*, uint32_t, const uint32_t*,
                                   void*, aacg_parse_result*, uint32_t*);
    int  (*pipeline_submit_ragged)(aacg_pipeline*, const uint8_t*, size_t, const aacg_parse_frame*, const uint32_t*, uint32_t, const uint32_t*,
                                   void*, aacg_parse_result*, uint32_t*, uint64_t*);
    uint64_t (*pipeline_plan_builds)(const aacg_pipeline*);
    int (*pipeline_launch_counts)(const aacg_pipeline*, uint64_t*, uint64_t*, uint64_t*);
    int  (*pipeline_walk_submit)(aacg_pipeline*, const uint8_t*, size_t, const aacg_parse_frame*, uint32_t, uint32_t, aacg_parse_frame*,
                                 aacg_walk_result*, uint64_t*);
    int  (*pipeline_walk_collect)(aacg_pipeline*, uint64_t);
    int  (*pipeline_set_mix)(aacg_pipeline*, uint32_t, const float*);
    int  (*pipeline_out_channels)(const aacg_pipeline*);
    int  (*mix_standard)(uint32_t, uint32_t, float, int, float*);
    int  (*pipeline_set_resample)(aacg_pipeline*, uint32_t, uint32_t, uint32_t, const float*);
    int  (*pipeline_out_samples)(aacg_pipeline*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*);
    int  (*resample_design)(uint32_t, uint32_t, uint32_t, double, double, uint32_t*, uint32_t*, float*, size_t);
    int  (*pipeline_set_concealment)(aacg_pipeline*, const aacg_conceal_config*);
    int  (*pipeline_set_trim)(aacg_pipeline*, const aacg_trim_config*);
    int  (*pipeline_set_stream_trim)(aacg_pipeline*, uint32_t, uint64_t, uint64_t);
    int  (*trim_design)(uint64_t, uint64_t, int, uint32_t, uint32_t, uint32_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*);
    void* (*host_alloc)(size_t);
    void (*host_free)(void*);
} L;

#define CHECK(env, call) do { if ((call) != napi_ok) { napi_throw_error((env), NULL, "aacgpu: N-API call failed: " #call); return NULL; } } while (0)

static napi_value fail(napi_env env, aacg_engine* e, int rc, const char* what)
{
    char msg[1024];
    snprintf(msg, sizeof msg, "aacgpu: %s failed (%d): %s", what, rc, e && L.last_error ? L.last_error(e) : "");
    napi_throw_error(env, NULL, msg);
    return NULL;
}

static int load_lib(napi_env env, const char* path)
{
    if (L.dl) return 1;
    L.dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!L.dl) {
        char msg[1024];
        snprintf(msg, sizeof msg, "aacgpu: cannot load %s: %s (build it with hipcc --offload-arch=gfx950; there is no CPU fallback)", path, dlerror());
        napi_throw_error(env, NULL, msg);
        return 0;
    }
#define SYM(field, name) do { *(void**)&L.field = dlsym(L.dl, name); if (!L.field) { napi_throw_error(env, NULL, "aacgpu: missing symbol " name); return 0; } } while (0)
    SYM(create, "aacg_create"); SYM(destroy, "aacg_destroy"); SYM(last_error, "aacg_last_error");
    SYM(abi_version, "aacg_abi_version"); SYM(reset_stream, "aacg_reset_stream");
    SYM(get_overlap, "aacg_get_overlap"); SYM(set_overlap, "aacg_set_overlap"); SYM(decode_batch, "aacg_decode_batch");
    SYM(submit, "aacg_submit"); SYM(wait, "aacg_wait");
    SYM(decode_batch_ex, "aacg_decode_batch_ex"); SYM(decode_batch_tns, "aacg_decode_batch_tns"); SYM(submit_tns, "aacg_submit_tns");
    SYM(parser_create, "aacg_parser_create"); SYM(parser_destroy, "aacg_parser_destroy"); SYM(parser_last_error, "aacg_parser_last_error");
    SYM(parse_status_string, "aacg_parse_status_string"); SYM(parse_batch, "aacg_parse_batch");
    SYM(pipeline_create, "aacg_pipeline_create"); SYM(pipeline_destroy, "aacg_pipeline_destroy"); SYM(pipeline_last_error, "aacg_pipeline_last_error");
    SYM(pipeline_stream_window_shape, "aacg_pipeline_stream_window_shape");
    SYM(pipeline_reset_stream, "aacg_pipeline_reset_stream"); SYM(pipeline_decode, "aacg_pipeline_decode");
    SYM(pipeline_submit, "aacg_pipeline_submit"); SYM(pipeline_collect, "aacg_pipeline_collect");
    SYM(pipeline_decode_ragged, "aacg_pipeline_decode_ragged"); SYM(pipeline_submit_ragged, "aacg_pipeline_submit_ragged");
    SYM(pipeline_plan_builds, "aacg_pipeline_plan_builds");
    SYM(pipeline_launch_counts, "aacg_pipeline_launch_counts");
    SYM(pipeline_walk_submit, "aacg_pipeline_walk_submit"); SYM(pipeline_walk_collect, "aacg_pipeline_walk_collect");
    SYM(pipeline_set_mix, "aacg_pipeline_set_mix"); SYM(pipeline_out_channels, "aacg_pipeline_out_channels"); SYM(mix_standard, "aacg_mix_standard");
    SYM(pipeline_set_resample, "aacg_pipeline_set_resample"); SYM(pipeline_out_samples, "aacg_pipeline_out_samples"); SYM(resample_design, "aacg_resample_design");
    SYM(pipeline_set_concealment, "aacg_pipeline_set_concealment");
    SYM(pipeline_set_trim, "aacg_pipeline_set_trim"); SYM(pipeline_set_stream_trim, "aacg_pipeline_set_stream_trim"); SYM(trim_design, "aacg_trim_design");
    SYM(host_alloc, "aacg_host_alloc"); SYM(host_free, "aacg_host_free");
#undef SYM
    return 1;
}

static int get_i32(napi_env env, napi_value obj, const char* key, int32_t dflt)
{
    napi_value v; bool has = false; int32_t out = dflt;
    if (napi_has_named_property(env, obj, key, &has) == napi_ok && has &&
        napi_get_named_property(env, obj, key, &v) == napi_ok) napi_get_value_int32(env, v, &out);
    return out;
}

/* What an external points to: the native object behind a tag that says which kind it is (a parser handle passed where an
 * engine is expected is refused instead of being cast), and a lock: an aacg_engine is not re-entrant (include/aacgpu.h:
 * externally serialised), so synchronous calls and the async jobs of one engine — which run on libuv threads — take
 * turns.  Jobs keep a reference on the external, so a collected Engine object cannot be finalised under a running job. */
#define BOX_ENGINE 0x41454e47u   /* 'AENG' */
#define BOX_PARSER 0x41505253u   /* 'APRS' */
#define BOX_PIPELINE 0x4150504cu /* 'APPL' */
#define PCM_RING_MAX 16
typedef struct { uint32_t kind; void* ptr; pthread_mutex_t lock; int out_i16; /* engine / pipeline: AACG_OUTPUT_I16 */
                 int resampled;   /* pipeline: made with { resample } or { trim } — a batch's PCM is ragged, sized by aacg_pipeline_out_samples */
                 /* pipeline, { pcmRing: K }: K page-locked PCM buffers made once and handed out in turn (pipelineDecode) */
                 napi_ref ring_ab[PCM_RING_MAX]; void* ring_ptr[PCM_RING_MAX]; size_t ring_bytes; int ring_n; unsigned ring_next;
                 /* pipeline: the batches submitted and not yet collected, oldest first (pipelineSubmit / pipelineCollect) */
                 void* jobs[4]; int n_jobs;
                 /* pipeline: the span walks submitted and not yet collected, oldest first (pipelineWalkSubmit / pipelineWalkCollect) */
                 void* walks[2]; int n_walks; } handle_box;

static handle_box* box_new(uint32_t kind, void* ptr)
{
    handle_box* b = (handle_box*)calloc(1, sizeof *b);
    if (!b) return NULL;
    b->kind = kind; b->ptr = ptr;
    pthread_mutex_init(&b->lock, NULL);
    return b;
}

static handle_box* box_of(napi_env env, napi_value v, uint32_t kind, const char* what)
{
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || ((handle_box*)p)->kind != kind) { napi_throw_error(env, NULL, what); return NULL; }
    return (handle_box*)p;
}

static void engine_finalize(napi_env env, void* data, void* hint)
{
    (void)env; (void)hint;
    handle_box* b = (handle_box*)data;
    if (!b) return;
    if (b->ptr && L.destroy) L.destroy((aacg_engine*)b->ptr);
    b->kind = 0;
    pthread_mutex_destroy(&b->lock);
    free(b);
}

/* load(path) -> abi version */
static napi_value js_load(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1]; char path[2048]; size_t n = 0; napi_value out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    CHECK(env, napi_get_value_string_utf8(env, argv[0], path, sizeof path, &n));
    if (!load_lib(env, path)) return NULL;
    CHECK(env, napi_create_int32(env, L.abi_version(), &out));
    return out;
}

/* create({deviceOrdinal, sampleIndex, maxStreams, maxChannels, maxBatchUnits, inputKind}) -> external */
static napi_value js_create(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    aacg_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = AACG_ABI_VERSION;
    cfg.device_ordinal = get_i32(env, argv[0], "deviceOrdinal", 0);
    cfg.sample_index = get_i32(env, argv[0], "sampleIndex", 3);
    cfg.max_streams = get_i32(env, argv[0], "maxStreams", 1);
    cfg.max_channels = get_i32(env, argv[0], "maxChannels", 2);
    cfg.max_batch_units = get_i32(env, argv[0], "maxBatchUnits", 0);
    cfg.input_kind = get_i32(env, argv[0], "inputKind", AACG_INPUT_QUANT_I16);
    cfg.tns_mode = get_i32(env, argv[0], "tnsMode", AACG_TNS_REFERENCE);
    cfg.pns_mode = get_i32(env, argv[0], "pnsMode", AACG_PNS_REFERENCE);
    cfg.output_kind = get_i32(env, argv[0], "outputKind", AACG_OUTPUT_F32);
    cfg.cce_mode = get_i32(env, argv[0], "cceMode", AACG_CCE_REFERENCE);
    aacg_engine* e = NULL;
    int rc = L.create(&cfg, &e);
    if (rc) return fail(env, NULL, rc, "aacg_create (is a GPU visible?)");
    handle_box* b = box_new(BOX_ENGINE, e);
    if (!b) { L.destroy(e); napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    b->out_i16 = cfg.output_kind == AACG_OUTPUT_I16;
    CHECK(env, napi_create_external(env, b, engine_finalize, NULL, &out));
    return out;
}

static handle_box* engine_box(napi_env env, napi_value v) { return box_of(env, v, BOX_ENGINE, "aacgpu: bad engine handle"); }
/* The synchronous entry points hold the engine's lock for the whole library call: an async job of the same engine —
 * queued or running on a libuv thread — takes the same lock around aacg_submit / aacg_wait, so the two can never be
 * inside the (non-re-entrant) engine at once.  (The JS wrapper awaits its jobs anyway; this is the backstop.) */
static aacg_engine* engine_lock(napi_env env, napi_value v, handle_box** box)
{
    handle_box* b = engine_box(env, v);
    *box = b;
    if (!b) return NULL;
    pthread_mutex_lock(&b->lock);
    return (aacg_engine*)b->ptr;
}
static void engine_unlock(handle_box* b) { pthread_mutex_unlock(&b->lock); }

static int typed(napi_env env, napi_value v, napi_typedarray_type* type, size_t* len, void** data)
{
    napi_value ab; size_t off;
    return napi_get_typedarray_info(env, v, type, len, data, &ab, &off) == napi_ok;
}

/* optional trailing argument: tns:Uint8Array of aacg_tns_info records (AACG_TNS_SPEC engines); 1 ok, 0 thrown */
static int optional_tns(napi_env env, size_t argc, napi_value* argv, size_t at, void** data, size_t* count)
{
    *data = NULL; *count = 0;
    if (argc <= at) return 1;
    napi_valuetype vt;
    if (napi_typeof(env, argv[at], &vt) != napi_ok) return 0;
    if (vt == napi_null || vt == napi_undefined) return 1;
    napi_typedarray_type tt; size_t nt;
    if (!typed(env, argv[at], &tt, &nt, data) || tt != napi_uint8_array || nt % sizeof(aacg_tns_info)) {
        napi_throw_type_error(env, NULL, "tns must be a Uint8Array of 424-byte aacg_tns_info records");
        return 0;
    }
    *count = nt / sizeof(aacg_tns_info);
    return 1;
}

/* optional trailing argument: cce:Uint8Array of aacg_cce_info records (AACG_CCE_SPEC engines); 1 ok, 0 thrown */
static int optional_cce(napi_env env, size_t argc, napi_value* argv, size_t at, void** data, size_t* count)
{
    *data = NULL; *count = 0;
    if (argc <= at) return 1;
    napi_valuetype vt;
    if (napi_typeof(env, argv[at], &vt) != napi_ok) return 0;
    if (vt == napi_null || vt == napi_undefined) return 1;
    napi_typedarray_type tt; size_t nt;
    if (!typed(env, argv[at], &tt, &nt, data) || tt != napi_uint8_array || nt % sizeof(aacg_cce_info)) {
        napi_throw_type_error(env, NULL, "cce must be a Uint8Array of 7716-byte aacg_cce_info records");
        return 0;
    }
    *count = nt / sizeof(aacg_cce_info);
    return 1;
}

/* decodeBatch(engine, units:Uint8Array(64*n), coeffs:Int16Array|Float32Array, meta:Uint16Array|null, pcm:Float32Array
 *             [, tns:Uint8Array(424*m) [, cce:Uint8Array(7716*k)]]) */
static napi_value js_decode_batch(napi_env env, napi_callback_info info)
{
    size_t argc = 7; napi_value argv[7];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void* dt; size_t nt; void* dcce; size_t ncce;
    if (!optional_tns(env, argc, argv, 5, &dt, &nt) || !optional_cce(env, argc, argv, 6, &dcce, &ncce)) return NULL;
    handle_box* box = engine_box(env, argv[0]);
    if (!box) return NULL;
    napi_typedarray_type tu, tc, tm, tp; size_t nu, nc, nm = 0, np; void *du, *dc, *dm = NULL, *dp;
    if (!typed(env, argv[1], &tu, &nu, &du) || tu != napi_uint8_array || nu % sizeof(aacg_unit_desc)) {
        napi_throw_type_error(env, NULL, "units must be a Uint8Array of 64-byte aacg_unit_desc records"); return NULL; }
    if (!typed(env, argv[2], &tc, &nc, &dc) || (tc != napi_int16_array && tc != napi_float32_array) || nc % 1024) {
        napi_throw_type_error(env, NULL, "coeffs must be an Int16Array or Float32Array, a multiple of 1024 long"); return NULL; }
    napi_valuetype vt;
    CHECK(env, napi_typeof(env, argv[3], &vt));
    if (vt != napi_null && vt != napi_undefined) {
        if (!typed(env, argv[3], &tm, &nm, &dm) || tm != napi_uint16_array || nm % AACG_MAX_SECTIONS) {
            napi_throw_type_error(env, NULL, "meta must be a Uint16Array of 120-word aacg_band_meta records"); return NULL; }
    }
    if (!typed(env, argv[4], &tp, &np, &dp) || tp != (box->out_i16 ? napi_int16_array : napi_float32_array)) {
        napi_throw_type_error(env, NULL, "pcm must be a Float32Array (an Int16Array for an engine created with outputKind: OUTPUT_I16)"); return NULL; }
    aacg_batch b;
    memset(&b, 0, sizeof b);
    b.units = (const aacg_unit_desc*)du; b.n_units = (uint32_t)(nu / sizeof(aacg_unit_desc));
    b.coeffs = dc; b.n_coef_blocks = (uint32_t)(nc / 1024);
    b.meta = (const aacg_band_meta*)dm; b.n_meta = (uint32_t)(nm / AACG_MAX_SECTIONS);
    b.tns = (const aacg_tns_info*)dt; b.n_tns = (uint32_t)nt;
    b.cce = (const aacg_cce_info*)dcce; b.n_cce = (uint32_t)ncce;
    b.pcm_out = dp; b.n_pcm_floats = np;
    aacg_engine* e = engine_lock(env, argv[0], &box);
    if (!e) return NULL;
    int rc = L.decode_batch_ex(e, &b);
    napi_value failed = rc ? fail(env, e, rc, "aacg_decode_batch") : NULL;     /* reads aacg_last_error: still under the lock */
    engine_unlock(box);
    if (rc) return failed;
    return argv[4];
}

static napi_value js_reset_stream(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2]; uint32_t s = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* box;
    napi_get_value_uint32(env, argv[1], &s);
    aacg_engine* e = engine_lock(env, argv[0], &box);
    if (!e) return NULL;
    int rc = L.reset_stream(e, s);
    if (rc) (void)fail(env, e, rc, "aacg_reset_stream");
    engine_unlock(box);
    return NULL;
}

/* getOverlap(engine, stream, channel, Float32Array(1024)) / setOverlap(...) */
static napi_value overlap_io(napi_env env, napi_callback_info info, int set)
{
    size_t argc = 4; napi_value argv[4]; uint32_t s = 0, c = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* box;
    napi_get_value_uint32(env, argv[1], &s);
    napi_get_value_uint32(env, argv[2], &c);
    napi_typedarray_type t; size_t n; void* d;
    if (!typed(env, argv[3], &t, &n, &d) || t != napi_float32_array || n != 1024) {
        napi_throw_type_error(env, NULL, "overlap buffer must be a Float32Array(1024)"); return NULL; }
    aacg_engine* e = engine_lock(env, argv[0], &box);
    if (!e) return NULL;
    int rc = set ? L.set_overlap(e, s, c, (const float*)d) : L.get_overlap(e, s, c, (float*)d);
    if (rc) (void)fail(env, e, rc, set ? "aacg_set_overlap" : "aacg_get_overlap");
    engine_unlock(box);
    return rc ? NULL : argv[3];
}
static napi_value js_get_overlap(napi_env env, napi_callback_info info) { return overlap_io(env, info, 0); }
static napi_value js_set_overlap(napi_env env, napi_callback_info info) { return overlap_io(env, info, 1); }

/* ---- decodeBatchAsync: the same call off the JavaScript thread (napi_async_work), so the event loop keeps
 * parsing the next frames while the GPU works; resolves with the pcm array, rejects with an Error ---------- */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[6];            /* units, coeffs, meta, pcm, tns and the engine handle stay alive until completion */
    handle_box* box;
    const aacg_tns_info* tns; uint32_t n_tns;
    aacg_engine* e;
    const aacg_unit_desc* units; uint32_t n_units;
    const void* coeffs; uint32_t n_blocks;
    const aacg_band_meta* meta; uint32_t n_meta;
    void* pcm; size_t n_pcm;
    int rc;
    char err[512];
} async_job;

static void job_execute(napi_env env, void* data)
{
    (void)env;
    async_job* j = (async_job*)data;
    uint64_t t = 0;
    pthread_mutex_lock(&j->box->lock);             /* jobs of one engine run one at a time, whatever thread they land on */
    j->rc = L.submit_tns(j->e, j->units, j->n_units, j->coeffs, j->n_blocks, j->meta, j->n_meta, j->tns, j->n_tns,
                         j->pcm, j->n_pcm, &t);
    if (!j->rc) j->rc = L.wait(j->e, t);
    if (j->rc) snprintf(j->err, sizeof j->err, "aacgpu: decodeBatchAsync failed (%d): %.400s", j->rc, L.last_error(j->e));
    pthread_mutex_unlock(&j->box->lock);
}

static void job_complete(napi_env env, napi_status status, void* data)
{
    async_job* j = (async_job*)data;
    napi_value v;
    if (status == napi_ok && j->rc == 0) {
        napi_get_reference_value(env, j->refs[3], &v);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg;
        napi_create_string_utf8(env, j->rc ? j->err : "aacgpu: async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &v);
        napi_reject_deferred(env, j->deferred, v);
    }
    for (int i = 0; i < 6; i++) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    free(j);
}

static napi_value js_decode_batch_async(napi_env env, napi_callback_info info)
{
    size_t argc = 6; napi_value argv[6], promise, name;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    void* dt; size_t nt;
    if (!optional_tns(env, argc, argv, 5, &dt, &nt)) return NULL;
    handle_box* box = engine_box(env, argv[0]);
    if (!box) return NULL;
    aacg_engine* e = (aacg_engine*)box->ptr;
    napi_typedarray_type tu, tc, tm, tp; size_t nu, nc, nm = 0, np; void *du, *dc, *dm = NULL, *dp;
    napi_valuetype vt;
    if (!typed(env, argv[1], &tu, &nu, &du) || tu != napi_uint8_array || nu % sizeof(aacg_unit_desc) ||
        !typed(env, argv[2], &tc, &nc, &dc) || (tc != napi_int16_array && tc != napi_float32_array) || nc % 1024 ||
        !typed(env, argv[4], &tp, &np, &dp) || tp != (box->out_i16 ? napi_int16_array : napi_float32_array)) {
        napi_throw_type_error(env, NULL, "decodeBatchAsync(engine, Uint8Array units, Int16Array|Float32Array coeffs, Uint16Array|null meta, Float32Array pcm)");
        return NULL;
    }
    CHECK(env, napi_typeof(env, argv[3], &vt));
    if (vt != napi_null && vt != napi_undefined &&
        (!typed(env, argv[3], &tm, &nm, &dm) || tm != napi_uint16_array || nm % AACG_MAX_SECTIONS)) {
        napi_throw_type_error(env, NULL, "meta must be a Uint16Array of 120-word aacg_band_meta records");
        return NULL;
    }
    async_job* j = (async_job*)calloc(1, sizeof *j);
    if (!j) { napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    j->e = e; j->box = box; j->units = (const aacg_unit_desc*)du;
    napi_create_reference(env, argv[0], 1, &j->refs[5]); j->n_units = (uint32_t)(nu / sizeof(aacg_unit_desc));
    j->coeffs = dc; j->n_blocks = (uint32_t)(nc / 1024); j->meta = (const aacg_band_meta*)dm; j->n_meta = (uint32_t)(nm / AACG_MAX_SECTIONS);
    j->pcm = dp; j->n_pcm = np;
    j->tns = (const aacg_tns_info*)dt; j->n_tns = (uint32_t)nt;
    if (dt) napi_create_reference(env, argv[5], 1, &j->refs[4]);
    const int idx[4] = {1, 2, 3, 4};
    for (int i = 0; i < 4; i++)
        if (!(i == 2 && !dm)) napi_create_reference(env, argv[idx[i]], 1, &j->refs[i]);
    CHECK(env, napi_create_promise(env, &j->deferred, &promise));
    CHECK(env, napi_create_string_utf8(env, "aacgpu.decodeBatchAsync", NAPI_AUTO_LENGTH, &name));
    CHECK(env, napi_create_async_work(env, NULL, name, job_execute, job_complete, j, &j->work));
    CHECK(env, napi_queue_async_work(env, j->work));
    return promise;
}

/* ---- device front end (aacg_parser_*) ------------------------------------------------------------------ */
static void parser_finalize(napi_env env, void* data, void* hint)
{
    (void)env; (void)hint;
    handle_box* b = (handle_box*)data;
    if (!b) return;
    if (b->ptr && L.parser_destroy) L.parser_destroy((aacg_parser*)b->ptr);
    b->kind = 0;
    pthread_mutex_destroy(&b->lock);
    free(b);
}

/* parserCreate({deviceOrdinal, sampleIndex}, entries:Uint8Array(12*n) of aacg_code_entry, counts:Uint32Array(12)) -> external */
static napi_value js_parser_create(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    napi_typedarray_type te, tc; size_t ne, nc; void *de, *dc;
    if (!typed(env, argv[1], &te, &ne, &de) || te != napi_uint8_array || ne % sizeof(aacg_code_entry) ||
        !typed(env, argv[2], &tc, &nc, &dc) || tc != napi_uint32_array || nc != 12) {
        napi_throw_type_error(env, NULL, "parserCreate(opts, entries:Uint8Array of 12-byte aacg_code_entry, counts:Uint32Array(12))"); return NULL; }
    size_t total = 0;
    for (int b = 0; b < 12; b++) total += ((const uint32_t*)dc)[b];
    if (total * sizeof(aacg_code_entry) != ne) { napi_throw_type_error(env, NULL, "counts do not add up to the number of entries"); return NULL; }
    aacg_parser* p = NULL;
    int rc = L.parser_create(get_i32(env, argv[0], "deviceOrdinal", 0), get_i32(env, argv[0], "sampleIndex", 3),
                             (const aacg_code_entry*)de, (const uint32_t*)dc, &p);
    if (rc) {
        char msg[1024];
        snprintf(msg, sizeof msg, "aacgpu: aacg_parser_create failed (%d): %s", rc, p ? L.parser_last_error(p) : "");
        if (p) L.parser_destroy(p);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    handle_box* b = box_new(BOX_PARSER, p);
    if (!b) { L.parser_destroy(p); napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    CHECK(env, napi_create_external(env, b, parser_finalize, NULL, &out));
    return out;
}

/* parseBatch(parser, bytes:Uint8Array, frames:Uint32Array(2*n) [offset, length]..., maxUnits, maxChannels, options,
 *            units:Uint8Array(64*n*maxUnits), q:Int16Array(1024*n*maxChannels), meta:Uint16Array(120*n*maxChannels),
 *            tns:Uint8Array(424*n*maxChannels)|null, results:Uint8Array(8*n)) */
static napi_value js_parse_batch(napi_env env, napi_callback_info info)
{
    size_t argc = 11; napi_value argv[11];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = argc < 11 ? NULL : box_of(env, argv[0], BOX_PARSER, "aacgpu: bad parser handle");
    if (argc < 11) napi_throw_error(env, NULL, "aacgpu: parseBatch takes 11 arguments");
    if (!pb) return NULL;
    aacg_parser* p = (aacg_parser*)pb->ptr;
    napi_typedarray_type t; size_t nb, nf, nu, nq, nm, nr; void *db, *df, *du, *dq, *dm, *dr, *dt; size_t nt;
    uint32_t max_units = 0, max_ch = 0, options = 0;
    napi_get_value_uint32(env, argv[3], &max_units); napi_get_value_uint32(env, argv[4], &max_ch); napi_get_value_uint32(env, argv[5], &options);
    if (!typed(env, argv[1], &t, &nb, &db) || t != napi_uint8_array || !typed(env, argv[2], &t, &nf, &df) || t != napi_uint32_array || (nf & 1)) {
        napi_throw_type_error(env, NULL, "parseBatch: bytes must be a Uint8Array, frames a Uint32Array of (offset, length) pairs"); return NULL; }
    const size_t n = nf / 2;
    if (!typed(env, argv[6], &t, &nu, &du) || t != napi_uint8_array || nu != n * max_units * sizeof(aacg_unit_desc) ||
        !typed(env, argv[7], &t, &nq, &dq) || t != napi_int16_array || nq != n * max_ch * 1024 ||
        !typed(env, argv[8], &t, &nm, &dm) || t != napi_uint16_array || nm != n * max_ch * AACG_MAX_SECTIONS ||
        !typed(env, argv[10], &t, &nr, &dr) || t != napi_uint8_array || nr != n * sizeof(aacg_parse_result)) {
        napi_throw_type_error(env, NULL, "parseBatch: output arrays do not have the sizes n * maxUnits / maxChannels imply"); return NULL; }
    if (!optional_tns(env, argc, argv, 9, &dt, &nt)) return NULL;
    if (dt && nt != n * max_ch) { napi_throw_type_error(env, NULL, "parseBatch: tns must hold n * maxChannels records"); return NULL; }
    int rc = L.parse_batch(p, (const uint8_t*)db, nb, (const aacg_parse_frame*)df, (uint32_t)n, max_units, max_ch, options,
                           (aacg_unit_desc*)du, (int16_t*)dq, (aacg_band_meta*)dm, (aacg_tns_info*)dt, (aacg_parse_result*)dr);
    if (rc) {
        char msg[1024];
        snprintf(msg, sizeof msg, "aacgpu: aacg_parse_batch failed (%d): %s", rc, L.parser_last_error(p));
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    return argv[10];
}

/* ---- bytes in, PCM out (aacg_pipeline_*): the resident route behind SharedEngine({ resident: true }) ------------------- */
static void ring_finalize(napi_env env, void* data, void* hint) { (void)env; (void)hint; if (data && L.host_free) L.host_free(data); }

static void pipe_abandon(napi_env env, void* job);    /* a submitted batch nobody collected: wait for it, drop it */
static void walk_abandon(napi_env env, void* job);    /* a submitted walk nobody collected: dropped behind the pipeline (whose destroy waits for it) */
static void pipeline_finalize(napi_env env, void* data, void* hint)
{
    (void)hint;
    handle_box* b = (handle_box*)data;
    if (!b) return;
    for (int i = 0; i < b->n_jobs; i++) pipe_abandon(env, b->jobs[i]);
    b->n_jobs = 0;
    if (b->ptr && L.pipeline_destroy) L.pipeline_destroy((aacg_pipeline*)b->ptr);
    for (int i = 0; i < b->n_walks; i++) walk_abandon(env, b->walks[i]);
    b->n_walks = 0;
    for (int i = 0; i < b->ring_n; i++) if (b->ring_ab[i]) napi_delete_reference(env, b->ring_ab[i]);   /* (the buffers go with their ArrayBuffers: ring_finalize) */
    b->kind = 0;
    pthread_mutex_destroy(&b->lock);
    free(b);
}

/* pipelineCreate({deviceOrdinal, sampleIndex, maxStreams, channels, maxFrames, outputKind, parseOptions, lanes, planMode, stages, mix, resample, conceal, trim}, entries, counts) -> external
 * (trim: true — aacg_pipeline_set_trim behind the mix and the resampler, before the call returns, every slot's window (0, all) until
 * pipelineSetStreamTrim says otherwise: only the kept samples come back, ragged per stream (pipelineDecode's lengths), possibly none;
 * conceal: { fadeSteps, holdFrames } — aacg_pipeline_set_concealment before the call returns, with planMode 1: a refused frame repeats its
 * stream's last good frame, fading, and its result carries AACG_PARSE_CONCEALED in byte 3; a refused setting destroys the pipeline and throws;
 * resample: { L, M, taps, table: Float32Array(L * taps) } — aacg_pipeline_set_resample behind the mix, before the call returns: the PCM leaves
 * at L / M times the streams' rate, ragged per stream (pipelineDecode's lengths); a refused resampler destroys the pipeline and throws;
 * mix: { outChannels: 1 | 2, matrix: Float32Array(outChannels * channels) } — aacg_pipeline_set_mix before the call returns: the PCM is
 * mixed on the device and outChannels channels leave; a refused mix destroys the pipeline and throws with the reason;
 * planMode 1: device plans, aacg_pipeline_config.plan_mode; stages: AACG_PIPELINE_STAGE_TNS | AACG_PIPELINE_STAGE_PNS | AACG_PIPELINE_STAGE_WINDOW_SHAPE,
 * aacg_pipeline_config.stages — bit 2 carries each channel's window shape from frame to frame on the device) */
static napi_value js_pipeline_create(napi_env env, napi_callback_info info)
{
    size_t argc = 3; napi_value argv[3], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    napi_typedarray_type te, tc; size_t ne, nc; void *de, *dc;
    if (!typed(env, argv[1], &te, &ne, &de) || te != napi_uint8_array || ne % sizeof(aacg_code_entry) ||
        !typed(env, argv[2], &tc, &nc, &dc) || tc != napi_uint32_array || nc != 12) {
        napi_throw_type_error(env, NULL, "pipelineCreate(opts, entries:Uint8Array of 12-byte aacg_code_entry, counts:Uint32Array(12))"); return NULL; }
    size_t total = 0;
    for (int b = 0; b < 12; b++) total += ((const uint32_t*)dc)[b];
    if (total * sizeof(aacg_code_entry) != ne) { napi_throw_type_error(env, NULL, "counts do not add up to the number of entries"); return NULL; }
    aacg_pipeline_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = AACG_ABI_VERSION;
    cfg.device_ordinal = get_i32(env, argv[0], "deviceOrdinal", 0);
    cfg.sample_index = get_i32(env, argv[0], "sampleIndex", 3);
    cfg.max_streams = get_i32(env, argv[0], "maxStreams", 1);
    cfg.channels = get_i32(env, argv[0], "channels", 2);
    cfg.max_frames = get_i32(env, argv[0], "maxFrames", 16);
    cfg.output_kind = get_i32(env, argv[0], "outputKind", AACG_OUTPUT_F32);
    cfg.parse_options = get_i32(env, argv[0], "parseOptions", AACG_PARSE_REFERENCE_QUIRKS);
    cfg.lanes = get_i32(env, argv[0], "lanes", 0);
    cfg.plan_mode = get_i32(env, argv[0], "planMode", 0);
    cfg.stages = get_i32(env, argv[0], "stages", 0);
    aacg_pipeline* p = NULL;
    int rc = L.pipeline_create(&cfg, (const aacg_code_entry*)de, (const uint32_t*)dc, &p);
    if (rc) {
        char msg[256];
        snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_create failed (%d) (is a GPU visible?)", rc);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    {
        napi_value mix; bool has = false; napi_valuetype vt = napi_undefined;
        if (napi_has_named_property(env, argv[0], "mix", &has) == napi_ok && has && napi_get_named_property(env, argv[0], "mix", &mix) == napi_ok &&
            napi_typeof(env, mix, &vt) == napi_ok && vt == napi_object) {
            const int32_t oc = get_i32(env, mix, "outChannels", 0);
            napi_value mv; napi_typedarray_type tm; size_t nm = 0; void* dm = NULL;
            char msg[1024] = "";
            if (napi_get_named_property(env, mix, "matrix", &mv) != napi_ok || !typed(env, mv, &tm, &nm, &dm) || tm != napi_float32_array || oc < 0 || nm != (size_t)oc * (size_t)cfg.channels)
                snprintf(msg, sizeof msg, "pipelineCreate: mix is { outChannels, matrix: Float32Array(outChannels * channels) }");
            else if ((rc = L.pipeline_set_mix(p, (uint32_t)oc, (const float*)dm)))
                snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_set_mix failed (%d): %.800s", rc, L.pipeline_last_error(p));
            if (msg[0]) { L.pipeline_destroy(p); napi_throw_error(env, NULL, msg); return NULL; }
        }
    }
    int resampled = 0;
    {   /* resample: { L, M, taps, table: Float32Array(L * taps) } — aacg_pipeline_set_resample, behind the mix */
        napi_value rs; bool has = false; napi_valuetype vt = napi_undefined;
        if (napi_has_named_property(env, argv[0], "resample", &has) == napi_ok && has && napi_get_named_property(env, argv[0], "resample", &rs) == napi_ok &&
            napi_typeof(env, rs, &vt) == napi_ok && vt == napi_object) {
            const int32_t rl = get_i32(env, rs, "L", 0), rm = get_i32(env, rs, "M", 0), rt = get_i32(env, rs, "taps", 0);
            napi_value tv; napi_typedarray_type tt; size_t nt = 0; void* dt = NULL;
            char msg[1024] = "";
            if (napi_get_named_property(env, rs, "table", &tv) != napi_ok || !typed(env, tv, &tt, &nt, &dt) || tt != napi_float32_array || rl < 1 || rt < 1 || rm < 1 || nt != (size_t)rl * (size_t)rt)
                snprintf(msg, sizeof msg, "pipelineCreate: resample is { L, M, taps, table: Float32Array(L * taps) }");
            else if ((rc = L.pipeline_set_resample(p, (uint32_t)rl, (uint32_t)rm, (uint32_t)rt, (const float*)dt)))
                snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_set_resample failed (%d): %.800s", rc, L.pipeline_last_error(p));
            if (msg[0]) { L.pipeline_destroy(p); napi_throw_error(env, NULL, msg); return NULL; }
            resampled = 1;
        }
    }
    {   /* conceal: { fadeSteps, holdFrames } — aacg_pipeline_set_concealment */
        napi_value cn; bool has = false; napi_valuetype vt = napi_undefined;
        if (napi_has_named_property(env, argv[0], "conceal", &has) == napi_ok && has && napi_get_named_property(env, argv[0], "conceal", &cn) == napi_ok &&
            napi_typeof(env, cn, &vt) == napi_ok && vt == napi_object) {
            const int32_t fs = get_i32(env, cn, "fadeSteps", 2), hf = get_i32(env, cn, "holdFrames", 6);
            char msg[1024] = "";
            aacg_conceal_config cc;
            cc.fade_steps = (uint32_t)fs; cc.hold_frames = (uint32_t)hf;
            if (fs < 0 || hf < 0) snprintf(msg, sizeof msg, "pipelineCreate: conceal is { fadeSteps: 0..64, holdFrames: 1..255 }");
            else if ((rc = L.pipeline_set_concealment(p, &cc)))
                snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_set_concealment failed (%d): %.800s", rc, L.pipeline_last_error(p));
            if (msg[0]) { L.pipeline_destroy(p); napi_throw_error(env, NULL, msg); return NULL; }
        }
    }
    {   /* trim: true — aacg_pipeline_set_trim, behind the mix and the resampler */
        napi_value tv; bool has = false, on = false;
        if (napi_has_named_property(env, argv[0], "trim", &has) == napi_ok && has && napi_get_named_property(env, argv[0], "trim", &tv) == napi_ok &&
            napi_coerce_to_bool(env, tv, &tv) == napi_ok && napi_get_value_bool(env, tv, &on) == napi_ok && on) {
            const aacg_trim_config tc = {0u, AACG_TRIM_ALL};
            if ((rc = L.pipeline_set_trim(p, &tc))) {
                char msg[1024];
                snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_set_trim failed (%d): %.800s", rc, L.pipeline_last_error(p));
                L.pipeline_destroy(p); napi_throw_error(env, NULL, msg); return NULL;
            }
            resampled = 1;                              /* ragged: the kept counts */
        }
    }
    handle_box* b = box_new(BOX_PIPELINE, p);
    if (!b) { L.pipeline_destroy(p); napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    b->out_i16 = cfg.output_kind == AACG_OUTPUT_I16;
    b->resampled = resampled;
    CHECK(env, napi_create_external(env, b, pipeline_finalize, NULL, &out));
    return out;
}

/* Page-locked PCM buffers handed to JavaScript as external ArrayBuffers: the PCM of a batch comes down from the device
 * straight into the memory the Float32Array views — no staging copy, no zero-filled allocation of tens of megabytes per batch.
 * A buffer returns to the pool when the garbage collector has let go of the batch's last frame (the finalizer runs on the
 * JavaScript thread, like every call into this addon); the pool holds a few, the rest are freed.
 * Finalizers do not run inside a synchronous loop, though, and that is how a host drains 256 streams: every flush would then
 * page-lock a fresh 33 MB (3.5-6 ms with hipHostMalloc; 0.6 since round 6: aacg_host_alloc).  So a helper thread keeps the NEXT buffers ready: when
 * one is taken, it makes another of that size while JavaScript slices the batch, and it does the freeing too. */
#define PCM_POOL_MAX 8
#define PCM_READY_MAX 3
typedef struct { void* ptr; size_t bytes; } pcm_buf;
static pcm_buf g_pool[PCM_POOL_MAX];               /* recycled by finalizers (the JavaScript thread of whichever environment — main or a
                                                      worker — let go of the buffer: under g_pool_lock) */
static int g_pool_n = 0;
static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;
static int pool_put(void* p, size_t bytes)          /* 1: kept for the next batch of that size */
{
    int kept = 0;
    pthread_mutex_lock(&g_pool_lock);
    if (g_pool_n < PCM_POOL_MAX) { g_pool[g_pool_n].ptr = p; g_pool[g_pool_n].bytes = bytes; g_pool_n++; kept = 1; }
    pthread_mutex_unlock(&g_pool_lock);
    return kept;
}
static pthread_mutex_t g_prep_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t g_prep_wake = PTHREAD_COND_INITIALIZER;
static pthread_cond_t g_ready_wake = PTHREAD_COND_INITIALIZER;   /* the helper has put a buffer into g_ready */
static pcm_buf g_ready[PCM_READY_MAX];             /* made ahead by the helper (under g_prep_lock) */
static int g_ready_n = 0;
static size_t g_want_bytes = 0;                    /* the size the helper keeps ready */
static void* g_trash[64];                          /* buffers for the helper to free */
static int g_trash_n = 0;
static int g_prep_started = 0;

static void* prep_main(void* arg)
{
    (void)arg;
    pthread_mutex_lock(&g_prep_lock);
    for (;;) {
        if (g_trash_n) {
            void* p = g_trash[--g_trash_n];
            pthread_mutex_unlock(&g_prep_lock);
            L.host_free(p);
            pthread_mutex_lock(&g_prep_lock);
            continue;
        }
        if (g_want_bytes && g_ready_n < PCM_READY_MAX) {
            const size_t bytes = g_want_bytes;
            pthread_mutex_unlock(&g_prep_lock);
            void* p = L.host_alloc(bytes);
            pthread_mutex_lock(&g_prep_lock);
            if (p) {
                if (g_ready_n < PCM_READY_MAX && bytes == g_want_bytes) { g_ready[g_ready_n].ptr = p; g_ready[g_ready_n].bytes = bytes; g_ready_n++; pthread_cond_broadcast(&g_ready_wake); }
                else if (g_trash_n < 64) g_trash[g_trash_n++] = p;
            } else { g_want_bytes = 0; pthread_cond_broadcast(&g_ready_wake); }      /* out of page-locked memory: the caller's own attempt will report it */
            continue;
        }
        pthread_cond_wait(&g_prep_wake, &g_prep_lock);
    }
    return NULL;
}

static void pcm_discard(void* p)                   /* free off the JavaScript thread where possible */
{
    pthread_mutex_lock(&g_prep_lock);
    const int queued = g_prep_started && g_trash_n < 64;
    if (queued) { g_trash[g_trash_n++] = p; pthread_cond_signal(&g_prep_wake); }
    pthread_mutex_unlock(&g_prep_lock);
    if (!queued) L.host_free(p);
}

static void pcm_finalize(napi_env env, void* data, void* hint)
{
    const size_t bytes = (size_t)hint;
    (void)env;
    if (!pool_put(data, bytes)) pcm_discard(data);
}

static void* pcm_take(size_t bytes, size_t* got)
{
    pthread_mutex_lock(&g_pool_lock);
    for (int i = 0; i < g_pool_n; i++)
        if (g_pool[i].bytes >= bytes && g_pool[i].bytes <= 2 * bytes + 4096) {
            void* p = g_pool[i].ptr; *got = g_pool[i].bytes;
            g_pool[i] = g_pool[--g_pool_n];
            pthread_mutex_unlock(&g_pool_lock);
            return p;
        }
    pthread_mutex_unlock(&g_pool_lock);
    void* p = NULL;
    pthread_mutex_lock(&g_prep_lock);
    if (!g_prep_started) {
        pthread_t t;
        if (pthread_create(&t, NULL, prep_main, NULL) == 0) { pthread_detach(t); g_prep_started = 1; }
    }
    for (int i = 0; i < g_ready_n && !p; i++)
        if (g_ready[i].bytes == bytes) { p = g_ready[i].ptr; g_ready[i] = g_ready[--g_ready_n]; }
    const int same_size = g_want_bytes == bytes;
    if (!same_size) {                              /* another batch size: what was made ahead for the old one goes */
        while (g_ready_n && g_trash_n < 64) g_trash[g_trash_n++] = g_ready[--g_ready_n].ptr;
        g_want_bytes = bytes;
    }
    if (g_prep_started) pthread_cond_signal(&g_prep_wake);
    /* none ready, but the helper is at one of this size: wait for that one rather than allocate beside it (two threads
     * page-locking 32 MiB at the same time take longer than one after the other: tools/micro/pinned_alloc.hip) */
    if (!p && g_prep_started && same_size) {
        struct timespec until;
        clock_gettime(CLOCK_REALTIME, &until);
        until.tv_nsec += 20 * 1000 * 1000;
        if (until.tv_nsec >= 1000000000L) { until.tv_sec++; until.tv_nsec -= 1000000000L; }
        while (!p && g_want_bytes == bytes) {
            for (int i = 0; i < g_ready_n && !p; i++)
                if (g_ready[i].bytes == bytes) { p = g_ready[i].ptr; g_ready[i] = g_ready[--g_ready_n]; }
            if (p) { pthread_cond_signal(&g_prep_wake); break; }
            if (pthread_cond_timedwait(&g_ready_wake, &g_prep_lock, &until) != 0) break;
        }
    }
    pthread_mutex_unlock(&g_prep_lock);
    *got = bytes;
    return p ? p : L.host_alloc(bytes);
}

/* pipelineDecode(pipeline, bytes:Uint8Array, frames:Uint32Array(2 * S * F) [offset, length]..., slots:Uint32Array(S), framesPerStream,
 *                results:Uint8Array(8 * S * F), channels [, ring, ringElems])
 *   -> { pcm: Float32Array|Int16Array(S * F * 1024 * channels) on page-locked memory, refused }
 * A pipeline made with { resample }: pcm holds what the batch emits at the new rate, stream after stream, and the result carries
 * lengths: Uint32Array(S), the samples per channel of each stream (aacg_pipeline_out_samples, asked before the batch is submitted).
 * framesPerStream may be a Uint32Array(S) of per-stream counts instead (aacg_pipeline_decode_ragged / _submit_ragged): stream s
 * brings counts[s] frames, and S * F above reads as the counts' sum — frames, results and PCM are packed stream after stream.
 * ring = 0 / absent: the PCM array's memory is the caller's for as long as any view of it lives (a buffer per call, recycled by
 * the garbage collector's finalizer).  ring = K: the pipeline's K buffers of ringElems elements, made at the first call, are
 * handed out in turn — what a call returns is overwritten by the K-th call after it. */
typedef struct {
    handle_box* pb;
    const uint8_t* db; size_t nb; const aacg_parse_frame* df; const uint32_t* ds; size_t ns; uint32_t F; aacg_parse_result* dr;
    const uint32_t* counts;                            /* ragged: per-stream frame counts (read during the call only), else NULL */
    void* pcm; size_t got, elems; int slot;
    uint32_t* lengths;                                 /* a resampled pipeline: each stream's samples per channel (malloc), else NULL */
    napi_ref keep[4];                                  /* the four argument arrays: theirs is the memory the native call reads and writes */
    int n_keep;
    uint64_t ticket; int submitted;                    /* pipelineSubmit: aacg_pipeline_submit's ticket */
    int rc; uint32_t refused; char msg[1024];
} pipe_job;

/* argument checking and the PCM buffer: everything that needs the JavaScript thread before the native call */
static pipe_job* pipe_prepare(napi_env env, napi_callback_info info, int keep_args)
{
    size_t argc = 9; napi_value argv[9];
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok) return NULL;
    if (argc < 7) { napi_throw_error(env, NULL, "aacgpu: pipelineDecode takes at least 7 arguments"); return NULL; }
    uint32_t ring = 0, ring_elems = 0;
    if (argc >= 9) { napi_get_value_uint32(env, argv[7], &ring); napi_get_value_uint32(env, argv[8], &ring_elems); }
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    if (pb->n_jobs && !keep_args) { napi_throw_error(env, NULL, "aacgpu: submitted batches have not been collected yet (pipelineCollect)"); return NULL; }
    if (pb->n_jobs >= 3) { napi_throw_error(env, NULL, "aacgpu: pipelineSubmit: three batches are in flight already (pipelineCollect)"); return NULL; }
    napi_typedarray_type t; size_t nb, nf, ns, nr, nc = 0; void *db, *df, *ds, *dr, *dc = NULL; uint32_t F = 0, C = 0;
    napi_get_value_uint32(env, argv[6], &C);
    int ragged = 0, counts_ok = 1;
    {
        bool is_ta = false;
        napi_is_typedarray(env, argv[4], &is_ta);
        if (is_ta) { ragged = 1; counts_ok = typed(env, argv[4], &t, &nc, &dc) && t == napi_uint32_array; }
        else napi_get_value_uint32(env, argv[4], &F);
    }
    size_t total = 0;                                  /* the batch's frames: S * F, or the counts' sum */
    if (!typed(env, argv[3], &t, &ns, &ds) || t != napi_uint32_array) counts_ok = 0;
    if (counts_ok && ragged) {
        if (nc != ns) counts_ok = 0;
        for (size_t s = 0; counts_ok && s < nc; s++) total += ((const uint32_t*)dc)[s];
    } else total = ns * F;
    if (!counts_ok || !typed(env, argv[1], &t, &nb, &db) || t != napi_uint8_array || !typed(env, argv[2], &t, &nf, &df) || t != napi_uint32_array ||
        (!ragged && !F) || !total || nf != 2 * total || C < 1 || C > AACG_MAX_CHANNELS ||
        !typed(env, argv[5], &t, &nr, &dr) || t != napi_uint8_array || nr != total * sizeof(aacg_parse_result)) {
        napi_throw_type_error(env, NULL, "pipelineDecode(pipeline, Uint8Array bytes, Uint32Array frames (2 per frame), Uint32Array slots, framesPerStream | Uint32Array counts (one per stream), Uint8Array results (8 per frame), channels)");
        return NULL;
    }
    {   /* the PCM's size follows the pipeline: the mix's channels where it has one (aacg_pipeline_out_channels) */
        const int oc = L.pipeline_out_channels((const aacg_pipeline*)pb->ptr);
        if (oc > 0) C = (uint32_t)oc;
    }
    size_t samples = total * 1024u;                     /* per channel, the whole batch */
    uint32_t* lengths = NULL;
    if (pb->resampled) {                                /* ragged: what the pipeline's clocks say these streams will emit */
        uint32_t* cnt = (uint32_t*)malloc(2 * ns * sizeof(uint32_t));
        if (!cnt) { napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
        lengths = cnt + ns;
        for (size_t s = 0; s < ns; s++) cnt[s] = ragged ? ((const uint32_t*)dc)[s] : F;
        pthread_mutex_lock(&pb->lock);
        const int rc = L.pipeline_out_samples((aacg_pipeline*)pb->ptr, (const uint32_t*)ds, cnt, (uint32_t)ns, lengths);
        pthread_mutex_unlock(&pb->lock);
        if (rc) { free(cnt); napi_throw_error(env, NULL, "aacgpu: aacg_pipeline_out_samples failed (a slot out of range, or more frames than maxFrames)"); return NULL; }
        samples = 0;
        for (size_t s = 0; s < ns; s++) { samples += lengths[s]; cnt[s] = lengths[s]; }
        lengths = cnt;                                  /* (the block's first half now holds them: one allocation, freed as one) */
    }
    const size_t elems = samples * C, bytes = elems ? elems * (pb->out_i16 ? 2u : 4u) : 16u;      /* (a trimmed batch may keep nothing: a buffer all the same) */
    size_t got = 0;
    void* pcm = NULL;
    int slot = -1;
    if (ring) {
        if (ring > PCM_RING_MAX || ring_elems < elems) { free(lengths); napi_throw_range_error(env, NULL, "aacgpu: pipelineDecode: ring of at most 16 buffers, each at least one batch long"); return NULL; }
        if (!pb->ring_n) {                                 /* the pipeline's ring: made once, kept alive by references until the pipeline goes */
            pb->ring_bytes = (size_t)ring_elems * (pb->out_i16 ? 2u : 4u);
            uint32_t made = 0;
            for (; made < ring; made++) {
                void* m = L.host_alloc(pb->ring_bytes);
                napi_value rab;
                if (!m) break;
                /* once the ArrayBuffer exists the memory is ITS (ring_finalize frees it when the buffer is collected); before, ours */
                if (napi_create_external_arraybuffer(env, m, pb->ring_bytes, ring_finalize, NULL, &rab) != napi_ok) { L.host_free(m); break; }
                if (napi_create_reference(env, rab, 1, &pb->ring_ab[made]) != napi_ok) break;
                pb->ring_ptr[made] = m;
            }
            if (made < ring) {                             /* all K or none: a shorter ring would overwrite frames earlier than the caller was told */
                for (uint32_t i = 0; i < made; i++) { napi_delete_reference(env, pb->ring_ab[i]); pb->ring_ab[i] = NULL; pb->ring_ptr[i] = NULL; }
                napi_throw_error(env, NULL, "aacgpu: out of page-locked memory (pcmRing)");
                free(lengths);
                return NULL;
            }
            pb->ring_n = (int)ring;
        }
        if (bytes > pb->ring_bytes) { free(lengths); napi_throw_range_error(env, NULL, "aacgpu: pipelineDecode: batch larger than the ring's buffers"); return NULL; }
        slot = (int)(pb->ring_next++ % (unsigned)pb->ring_n);
        pcm = pb->ring_ptr[slot]; got = pb->ring_bytes;
    } else {
        pcm = pcm_take(bytes, &got);
        if (!pcm) { free(lengths); napi_throw_error(env, NULL, "aacgpu: out of page-locked memory"); return NULL; }
    }
    pipe_job* j = (pipe_job*)calloc(1, sizeof *j);
    if (!j) { free(lengths); if (slot < 0 && !pool_put(pcm, got)) pcm_discard(pcm); napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    j->pb = pb; j->db = (const uint8_t*)db; j->nb = nb; j->df = (const aacg_parse_frame*)df; j->ds = (const uint32_t*)ds; j->ns = ns; j->F = F;
    j->dr = (aacg_parse_result*)dr; j->pcm = pcm; j->got = got; j->elems = elems; j->slot = slot; j->counts = (const uint32_t*)dc;
    j->lengths = lengths;
    if (keep_args) {
        const int which[4] = {1, 2, 3, 5};
        for (int k = 0; k < 4; k++)
            if (napi_create_reference(env, argv[which[k]], 1, &j->keep[j->n_keep]) == napi_ok) j->n_keep++;
    }
    return j;
}

/* the synchronous call (pipelineDecode), or the enqueue half of the asynchronous pair (pipelineSubmit: aacg_pipeline_submit
 * stages the bytes and returns when the batch is on its lane — no thread of the addon's is involved, round 5's was) */
static void pipe_run(pipe_job* j, int submit_only)
{
    pthread_mutex_lock(&j->pb->lock);
    aacg_pipeline* p = (aacg_pipeline*)j->pb->ptr;
    if (submit_only) {
        j->rc = j->counts ? L.pipeline_submit_ragged(p, j->db, j->nb, j->df, j->ds, (uint32_t)j->ns, j->counts, j->pcm, j->dr, &j->refused, &j->ticket)
                          : L.pipeline_submit(p, j->db, j->nb, j->df, j->ds, (uint32_t)j->ns, j->F, j->pcm, j->dr, &j->refused, &j->ticket);
        j->submitted = j->rc == 0;
    } else j->rc = j->counts ? L.pipeline_decode_ragged(p, j->db, j->nb, j->df, j->ds, (uint32_t)j->ns, j->counts, j->pcm, j->dr, &j->refused)
                             : L.pipeline_decode(p, j->db, j->nb, j->df, j->ds, (uint32_t)j->ns, j->F, j->pcm, j->dr, &j->refused);
    j->counts = NULL;                                  /* the counts are read by the call only (the pipeline keeps a copy) */
    if (j->rc) snprintf(j->msg, sizeof j->msg, "aacgpu: %s%s failed (%d): %.800s", submit_only ? "aacg_pipeline_submit" : "aacg_pipeline_decode",
                        j->F ? "" : "_ragged", j->rc, L.pipeline_last_error(p));
    pthread_mutex_unlock(&j->pb->lock);
}
static void pipe_wait(pipe_job* j)
{
    if (!j->submitted) return;
    pthread_mutex_lock(&j->pb->lock);
    aacg_pipeline* p = (aacg_pipeline*)j->pb->ptr;
    j->rc = L.pipeline_collect(p, j->ticket);
    if (j->rc) snprintf(j->msg, sizeof j->msg, "aacgpu: aacg_pipeline_collect failed (%d): %.800s", j->rc, L.pipeline_last_error(p));
    j->submitted = 0;
    pthread_mutex_unlock(&j->pb->lock);
}

/* back on the JavaScript thread: { pcm, refused } or the error; the job is freed */
static napi_value pipe_finish(napi_env env, pipe_job* j)
{
    napi_value out = NULL, v, ab;
    handle_box* pb = j->pb;
    for (int k = 0; k < j->n_keep; k++) napi_delete_reference(env, j->keep[k]);
    if (j->rc) {
        if (j->slot < 0 && !pool_put(j->pcm, j->got)) pcm_discard(j->pcm);
        napi_throw_error(env, NULL, j->msg);
        free(j->lengths);
        free(j);
        return NULL;
    }
    uint32_t* lengths = j->lengths; const size_t n_streams = j->ns;
    const size_t elems = j->elems, got = j->got; void* pcm = j->pcm; const int slot = j->slot; const uint32_t refused = j->refused;
    free(j);
    napi_value lv = NULL;
    if (lengths) {                                      /* copied out first, so that no exit below leaves the block behind */
        void* ld = NULL; napi_value lab;
        const napi_status st = napi_create_arraybuffer(env, n_streams * sizeof(uint32_t), &ld, &lab);
        if (st == napi_ok) memcpy(ld, lengths, n_streams * sizeof(uint32_t));
        free(lengths);
        if (st != napi_ok || napi_create_typedarray(env, napi_uint32_array, n_streams, lab, 0, &lv) != napi_ok) lv = NULL;
    }
    if (slot >= 0) CHECK(env, napi_get_reference_value(env, pb->ring_ab[slot], &ab));
    else
    /* (the engine is not told about the buffer's size with napi_adjust_external_memory: it answers 33 MB of external memory
     * per batch with a full collection per batch; the views are short-lived objects, ordinary collections find the buffers) */
    if (napi_create_external_arraybuffer(env, pcm, got, pcm_finalize, (void*)got, &ab) != napi_ok) { L.host_free(pcm); napi_throw_error(env, NULL, "aacgpu: napi_create_external_arraybuffer failed"); return NULL; }
    CHECK(env, napi_create_typedarray(env, pb->out_i16 ? napi_int16_array : napi_float32_array, elems, ab, 0, &v));
    CHECK(env, napi_create_object(env, &out));
    CHECK(env, napi_set_named_property(env, out, "pcm", v));
    CHECK(env, napi_create_uint32(env, refused, &v));
    CHECK(env, napi_set_named_property(env, out, "refused", v));
    if (lv) CHECK(env, napi_set_named_property(env, out, "lengths", lv));
    return out;
}

static void pipe_abandon(napi_env env, void* job)
{
    pipe_job* j = (pipe_job*)job;
    pipe_wait(j);                                       /* the device writes into j->pcm and the results array until then */
    for (int k = 0; k < j->n_keep; k++) napi_delete_reference(env, j->keep[k]);
    if (j->slot < 0) pcm_discard(j->pcm);
    free(j->lengths);
    free(j);
}

static napi_value js_pipeline_decode(napi_env env, napi_callback_info info)
{
    pipe_job* j = pipe_prepare(env, info, 0);
    if (!j) return NULL;
    pipe_run(j, 0);
    return pipe_finish(env, j);
}

/* pipelineSubmit(same arguments as pipelineDecode): the batch is staged and enqueued (aacg_pipeline_submit) and the call returns
 * while the device works — JavaScript slices the batch before, say.  The bytes / frames / slots arrays may be reused at once; the
 * results array belongs to the batch until pipelineCollect(pipeline) -> { pcm, refused } has returned the OLDEST submitted batch
 * (it waits for it, bounded).  Up to three batches in flight per pipeline. */
static napi_value js_pipeline_submit(napi_env env, napi_callback_info info)
{
    pipe_job* j = pipe_prepare(env, info, 1);
    if (!j) return NULL;
    pipe_run(j, 1);
    if (j->rc) return pipe_finish(env, j);              /* refused at once: thrown here, nothing to collect */
    j->pb->jobs[j->pb->n_jobs++] = j;
    return NULL;
}

static napi_value js_pipeline_collect(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    if (!pb->n_jobs) { napi_throw_error(env, NULL, "aacgpu: pipelineCollect: nothing has been submitted"); return NULL; }
    pipe_job* j = (pipe_job*)pb->jobs[0];
    for (int i = 1; i < pb->n_jobs; i++) pb->jobs[i - 1] = pb->jobs[i];
    pb->n_jobs--;
    pipe_wait(j);
    return pipe_finish(env, j);
}

/* pipelineWalkSubmit(pipeline, bytes:Uint8Array, spans:Uint32Array(2 * n) [offset, length]..., maxFrames,
 *                    frames:Uint32Array(2 * n * maxFrames), results:Uint32Array(4 * n) [n_frames, status, bytes_consumed, 0]...)
 * aacg_pipeline_walk_submit: the bytes and spans may be reused at once; frames / results belong to the walk until
 * pipelineWalkCollect(pipeline) has returned the OLDEST submitted walk (it waits for it, bounded).  Two walks in flight at most. */
typedef struct { handle_box* pb; uint64_t ticket; napi_ref keep[2]; } walk_job;

static void walk_release(napi_env env, walk_job* w)
{
    for (int k = 0; k < 2; k++) if (w->keep[k]) napi_delete_reference(env, w->keep[k]);
    free(w);
}

static void walk_abandon(napi_env env, void* job) { walk_release(env, (walk_job*)job); }

static napi_value js_pipeline_walk_submit(napi_env env, napi_callback_info info)
{
    size_t argc = 6; napi_value argv[6];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 6) { napi_throw_error(env, NULL, "aacgpu: pipelineWalkSubmit takes 6 arguments"); return NULL; }
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    if (pb->n_walks >= 2) { napi_throw_error(env, NULL, "aacgpu: pipelineWalkSubmit: two walks are in flight already (pipelineWalkCollect)"); return NULL; }
    napi_typedarray_type t; size_t nb, ns, nf, nr; void *db, *ds, *df, *dr; uint32_t M = 0;
    napi_get_value_uint32(env, argv[3], &M);
    if (!typed(env, argv[1], &t, &nb, &db) || t != napi_uint8_array || !typed(env, argv[2], &t, &ns, &ds) || t != napi_uint32_array ||
        !typed(env, argv[4], &t, &nf, &df) || t != napi_uint32_array || !typed(env, argv[5], &t, &nr, &dr) || t != napi_uint32_array ||
        !M || !ns || (ns & 1) || nf != ns * M || nr != 2 * ns) {
        napi_throw_type_error(env, NULL, "pipelineWalkSubmit(pipeline, Uint8Array bytes, Uint32Array spans (2 per span), maxFrames, Uint32Array frames (2 * maxFrames per span), Uint32Array results (4 per span))");
        return NULL;
    }
    walk_job* w = (walk_job*)calloc(1, sizeof *w);
    if (!w) { napi_throw_error(env, NULL, "aacgpu: out of memory"); return NULL; }
    w->pb = pb;
    pthread_mutex_lock(&pb->lock);
    const int rc = L.pipeline_walk_submit((aacg_pipeline*)pb->ptr, (const uint8_t*)db, nb, (const aacg_parse_frame*)ds, (uint32_t)(ns / 2), M,
                                          (aacg_parse_frame*)df, (aacg_walk_result*)dr, &w->ticket);
    char msg[1024] = "";
    if (rc) snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_walk_submit failed (%d): %.800s", rc, L.pipeline_last_error((aacg_pipeline*)pb->ptr));
    pthread_mutex_unlock(&pb->lock);
    if (rc) { free(w); napi_throw_error(env, NULL, msg); return NULL; }
    napi_create_reference(env, argv[4], 1, &w->keep[0]);
    napi_create_reference(env, argv[5], 1, &w->keep[1]);
    pb->walks[pb->n_walks++] = w;
    return NULL;
}

static napi_value js_pipeline_walk_collect(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    if (!pb->n_walks) { napi_throw_error(env, NULL, "aacgpu: pipelineWalkCollect: nothing has been submitted"); return NULL; }
    walk_job* w = (walk_job*)pb->walks[0];
    for (int i = 1; i < pb->n_walks; i++) pb->walks[i - 1] = pb->walks[i];
    pb->n_walks--;
    pthread_mutex_lock(&pb->lock);
    const int rc = L.pipeline_walk_collect((aacg_pipeline*)pb->ptr, w->ticket);
    char msg[1024] = "";
    if (rc) snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_walk_collect failed (%d): %.800s", rc, L.pipeline_last_error((aacg_pipeline*)pb->ptr));
    pthread_mutex_unlock(&pb->lock);
    walk_release(env, w);
    if (rc) napi_throw_error(env, NULL, msg);
    return NULL;
}

static napi_value js_pipeline_reset_stream(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2]; uint32_t slot = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    napi_get_value_uint32(env, argv[1], &slot);
    pthread_mutex_lock(&pb->lock);
    int rc = L.pipeline_reset_stream((aacg_pipeline*)pb->ptr, slot);
    pthread_mutex_unlock(&pb->lock);
    if (rc) napi_throw_error(env, NULL, "aacgpu: aacg_pipeline_reset_stream failed");
    return NULL;
}

/* pipelineStreamWindowShape(pipeline, slot) -> Uint8Array(8): the window shape (0 sine, 1 KBD) each channel of the slot carries into
 * its next frame (aacg_pipeline_stream_window_shape; finishes the batches in flight first) */
static napi_value js_pipeline_stream_window_shape(napi_env env, napi_callback_info info)
{
    size_t argc = 2; napi_value argv[2], ab, out; uint32_t slot = 0; void* data = NULL;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    napi_get_value_uint32(env, argv[1], &slot);
    uint8_t shapes[8] = {0};
    pthread_mutex_lock(&pb->lock);
    int rc = L.pipeline_stream_window_shape((aacg_pipeline*)pb->ptr, slot, shapes);
    pthread_mutex_unlock(&pb->lock);
    if (rc) { napi_throw_error(env, NULL, "aacgpu: aacg_pipeline_stream_window_shape failed"); return NULL; }
    CHECK(env, napi_create_arraybuffer(env, 8, &data, &ab));
    memcpy(data, shapes, 8);
    CHECK(env, napi_create_typedarray(env, napi_uint8_array, 8, ab, 0, &out));
    return out;
}

/* pipelineOutChannels(pipeline) -> the channels of the PCM the pipeline delivers (aacg_pipeline_out_channels) */
static napi_value js_pipeline_out_channels(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    CHECK(env, napi_create_int32(env, L.pipeline_out_channels((const aacg_pipeline*)pb->ptr), &out));
    return out;
}

/* mixStandard(channels, outChannels, surroundGain, normalise) -> Float32Array(outChannels * channels): the project's standard downmix
 * (aacg_mix_standard, include/aacgpu.h has the table); host code, no device */
static napi_value js_mix_standard(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4], ab, out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    uint32_t ch = 0, oc = 0; double gain = 0.70710678118654752440; bool norm = true;
    if (argc < 2 || napi_get_value_uint32(env, argv[0], &ch) != napi_ok || napi_get_value_uint32(env, argv[1], &oc) != napi_ok ||
        (argc >= 3 && napi_get_value_double(env, argv[2], &gain) != napi_ok) || (argc >= 4 && napi_coerce_to_bool(env, argv[3], &argv[3]) != napi_ok) ||
        (argc >= 4 && napi_get_value_bool(env, argv[3], &norm) != napi_ok)) {
        napi_throw_type_error(env, NULL, "mixStandard(channels, outChannels [, surroundGain, normalise])"); return NULL; }
    float m[16];
    const int rc = L.mix_standard(ch, oc, (float)gain, norm ? 1 : 0, m);
    if (rc) { char msg[128]; snprintf(msg, sizeof msg, "aacgpu: aacg_mix_standard failed (%d)", rc); napi_throw_error(env, NULL, msg); return NULL; }
    void* data = NULL;
    CHECK(env, napi_create_arraybuffer(env, (size_t)ch * oc * sizeof(float), &data, &ab));
    memcpy(data, m, (size_t)ch * oc * sizeof(float));
    CHECK(env, napi_create_typedarray(env, napi_float32_array, (size_t)ch * oc, ab, 0, &out));
    return out;
}

/* a count of samples from a JavaScript number: an integer in 0 .. 2^53 - 1; `all`: undefined / null mean AACG_TRIM_ALL */
static int get_samples(napi_env env, napi_value v, int all, uint64_t* out)
{
    napi_valuetype vt = napi_undefined;
    double d = 0.0;
    if (napi_typeof(env, v, &vt) != napi_ok) return 0;
    if (all && (vt == napi_undefined || vt == napi_null)) { *out = AACG_TRIM_ALL; return 1; }
    if (vt != napi_number || napi_get_value_double(env, v, &d) != napi_ok || !(d >= 0.0) || d > 9007199254740991.0 || d != (double)(uint64_t)d) return 0;
    *out = (uint64_t)d;
    return 1;
}

/* pipelineSetStreamTrim(pipeline, slot, skip [, keep]): aacg_pipeline_set_stream_trim — the slot's window (keep absent: all) and position 0,
 * from the next batch enqueued that holds the slot */
static napi_value js_pipeline_set_stream_trim(napi_env env, napi_callback_info info)
{
    size_t argc = 4; napi_value argv[4], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = argc >= 3 ? box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle") : NULL;
    uint32_t slot = 0; uint64_t skip = 0, keep = AACG_TRIM_ALL;
    if (!pb) { if (argc < 3) napi_throw_type_error(env, NULL, "pipelineSetStreamTrim(pipeline, slot, skip [, keep])"); return NULL; }
    if (napi_get_value_uint32(env, argv[1], &slot) != napi_ok || !get_samples(env, argv[2], 0, &skip) || (argc >= 4 && !get_samples(env, argv[3], 1, &keep))) {
        napi_throw_type_error(env, NULL, "pipelineSetStreamTrim(pipeline, slot, skip [, keep]): counts of samples are integers in 0 .. 2^53 - 1"); return NULL; }
    pthread_mutex_lock(&pb->lock);
    const int rc = L.pipeline_set_stream_trim((aacg_pipeline*)pb->ptr, slot, skip, keep);
    char msg[1024] = "";
    if (rc) snprintf(msg, sizeof msg, "aacgpu: aacg_pipeline_set_stream_trim failed (%d): %.800s", rc, L.pipeline_last_error((aacg_pipeline*)pb->ptr));
    pthread_mutex_unlock(&pb->lock);
    if (rc) { napi_throw_error(env, NULL, msg); return NULL; }
    CHECK(env, napi_get_undefined(env, &out));
    return out;
}

/* trimDesign(skipIn, keepIn | undefined, limiter, L, M, taps) -> { skip, keep | null, residualNum, residualDen }: aacg_trim_design
 * (include/aacgpu.h) — the window at the trim's input for a window in the stream's own samples; host code, no device */
static napi_value js_trim_design(napi_env env, napi_callback_info info)
{
    size_t argc = 6; napi_value argv[6], out, v;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    uint64_t skip_in = 0, keep_in = AACG_TRIM_ALL, skip = 0, keep = 0, num = 0, den = 1;
    uint32_t rl = 1, rm = 1, taps = 0; bool limiter = false;
    if (argc < 1 || !get_samples(env, argv[0], 0, &skip_in) || (argc >= 2 && !get_samples(env, argv[1], 1, &keep_in)) ||
        (argc >= 3 && (napi_coerce_to_bool(env, argv[2], &v) != napi_ok || napi_get_value_bool(env, v, &limiter) != napi_ok)) ||
        (argc >= 6 && (napi_get_value_uint32(env, argv[3], &rl) != napi_ok || napi_get_value_uint32(env, argv[4], &rm) != napi_ok || napi_get_value_uint32(env, argv[5], &taps) != napi_ok))) {
        napi_throw_type_error(env, NULL, "trimDesign(skipIn, keepIn | undefined, limiter [, L, M, taps])"); return NULL; }
    const int rc = L.trim_design(skip_in, keep_in, limiter ? 1 : 0, rl, rm, taps, &skip, &keep, &num, &den);
    if (rc) { char msg[128]; snprintf(msg, sizeof msg, "aacgpu: aacg_trim_design failed (%d)", rc); napi_throw_error(env, NULL, msg); return NULL; }
    CHECK(env, napi_create_object(env, &out));
    CHECK(env, napi_create_double(env, (double)skip, &v)); CHECK(env, napi_set_named_property(env, out, "skip", v));
    if (keep == AACG_TRIM_ALL) CHECK(env, napi_get_null(env, &v)); else CHECK(env, napi_create_double(env, (double)keep, &v));
    CHECK(env, napi_set_named_property(env, out, "keep", v));
    CHECK(env, napi_create_double(env, (double)num, &v)); CHECK(env, napi_set_named_property(env, out, "residualNum", v));
    CHECK(env, napi_create_double(env, (double)den, &v)); CHECK(env, napi_set_named_property(env, out, "residualDen", v));
    return out;
}

/* resampleDesign(inRate, outRate, taps [, rolloff, beta]) -> { L, M, taps, table: Float32Array(L * taps) }: the project's default
 * resampling table (aacg_resample_design, include/aacgpu.h), what pipelineCreate({ resample }) takes; host code, no device */
static napi_value js_resample_design(napi_env env, napi_callback_info info)
{
    size_t argc = 5; napi_value argv[5], ab, out, v;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    uint32_t in_rate = 0, out_rate = 0, taps = 0, rl = 0, rm = 0; double rolloff = 0.0, beta = 0.0;
    if (argc < 3 || napi_get_value_uint32(env, argv[0], &in_rate) != napi_ok || napi_get_value_uint32(env, argv[1], &out_rate) != napi_ok ||
        napi_get_value_uint32(env, argv[2], &taps) != napi_ok || (argc >= 4 && napi_get_value_double(env, argv[3], &rolloff) != napi_ok) ||
        (argc >= 5 && napi_get_value_double(env, argv[4], &beta) != napi_ok)) {
        napi_throw_type_error(env, NULL, "resampleDesign(inRate, outRate, taps [, rolloff, beta])"); return NULL; }
    int rc = L.resample_design(in_rate, out_rate, taps, rolloff, beta, &rl, &rm, NULL, 0);      /* the ratio first: it sizes the table */
    void* data = NULL;
    if (!rc) {
        CHECK(env, napi_create_arraybuffer(env, (size_t)rl * taps * sizeof(float), &data, &ab));
        rc = L.resample_design(in_rate, out_rate, taps, rolloff, beta, &rl, &rm, (float*)data, (size_t)rl * taps);
    }
    if (rc) { char msg[128]; snprintf(msg, sizeof msg, "aacgpu: aacg_resample_design failed (%d)", rc); napi_throw_error(env, NULL, msg); return NULL; }
    CHECK(env, napi_create_object(env, &out));
    CHECK(env, napi_create_uint32(env, rl, &v)); CHECK(env, napi_set_named_property(env, out, "L", v));
    CHECK(env, napi_create_uint32(env, rm, &v)); CHECK(env, napi_set_named_property(env, out, "M", v));
    CHECK(env, napi_create_uint32(env, taps, &v)); CHECK(env, napi_set_named_property(env, out, "taps", v));
    CHECK(env, napi_create_typedarray(env, napi_float32_array, (size_t)rl * taps, ab, 0, &v)); CHECK(env, napi_set_named_property(env, out, "table", v));
    return out;
}

/* pipelinePlanBuilds(pipeline) -> how many plans the pipeline has built (one per batch shape it had not kept; aacgpu_tools.h) */
static napi_value js_pipeline_plan_builds(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1], out;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    pthread_mutex_lock(&pb->lock);
    const uint64_t n = L.pipeline_plan_builds((const aacg_pipeline*)pb->ptr);
    pthread_mutex_unlock(&pb->lock);
    CHECK(env, napi_create_double(env, (double)n, &out));
    return out;
}

/* pipelineLaunchCounts(pipeline) -> { shaped, chained, launches }: batches whose plan was shaped on the device, transform launches
 * that continued their predecessor through the cross-launch cells, transform launches in all (aacgpu_tools.h) */
static napi_value js_pipeline_launch_counts(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1], out, v;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_box* pb = box_of(env, argv[0], BOX_PIPELINE, "aacgpu: bad pipeline handle");
    if (!pb) return NULL;
    uint64_t n[3] = {0, 0, 0};
    pthread_mutex_lock(&pb->lock);
    const int rc = L.pipeline_launch_counts((const aacg_pipeline*)pb->ptr, &n[0], &n[1], &n[2]);
    pthread_mutex_unlock(&pb->lock);
    if (rc) { napi_throw_error(env, NULL, "aacgpu: aacg_pipeline_launch_counts failed"); return NULL; }
    static const char* const names[3] = {"shaped", "chained", "launches"};
    CHECK(env, napi_create_object(env, &out));
    for (int i = 0; i < 3; i++) {
        CHECK(env, napi_create_double(env, (double)n[i], &v));
        CHECK(env, napi_set_named_property(env, out, names[i], v));
    }
    return out;
}

/* parseStatusString(code) -> the reference's message for a per-frame status */
static napi_value js_parse_status_string(napi_env env, napi_callback_info info)
{
    size_t argc = 1; napi_value argv[1], out; int32_t code = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.dl) { napi_throw_error(env, NULL, "aacgpu: call load(path) first"); return NULL; }
    napi_get_value_int32(env, argv[0], &code);
    CHECK(env, napi_create_string_utf8(env, L.parse_status_string(code), NAPI_AUTO_LENGTH, &out));
    return out;
}

static napi_value init(napi_env env, napi_value exports)
{
    napi_property_descriptor props[] = {
        {"load", NULL, js_load, NULL, NULL, NULL, napi_default, NULL},
        {"create", NULL, js_create, NULL, NULL, NULL, napi_default, NULL},
        {"decodeBatch", NULL, js_decode_batch, NULL, NULL, NULL, napi_default, NULL},
        {"decodeBatchAsync", NULL, js_decode_batch_async, NULL, NULL, NULL, napi_default, NULL},
        {"resetStream", NULL, js_reset_stream, NULL, NULL, NULL, napi_default, NULL},
        {"getOverlap", NULL, js_get_overlap, NULL, NULL, NULL, napi_default, NULL},
        {"setOverlap", NULL, js_set_overlap, NULL, NULL, NULL, napi_default, NULL},
        {"parserCreate", NULL, js_parser_create, NULL, NULL, NULL, napi_default, NULL},
        {"parseBatch", NULL, js_parse_batch, NULL, NULL, NULL, napi_default, NULL},
        {"parseStatusString", NULL, js_parse_status_string, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineCreate", NULL, js_pipeline_create, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineDecode", NULL, js_pipeline_decode, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineSubmit", NULL, js_pipeline_submit, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineCollect", NULL, js_pipeline_collect, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineResetStream", NULL, js_pipeline_reset_stream, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineStreamWindowShape", NULL, js_pipeline_stream_window_shape, NULL, NULL, NULL, napi_default, NULL},
        {"pipelinePlanBuilds", NULL, js_pipeline_plan_builds, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineOutChannels", NULL, js_pipeline_out_channels, NULL, NULL, NULL, napi_default, NULL},
        {"mixStandard", NULL, js_mix_standard, NULL, NULL, NULL, napi_default, NULL},
        {"resampleDesign", NULL, js_resample_design, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineSetStreamTrim", NULL, js_pipeline_set_stream_trim, NULL, NULL, NULL, napi_default, NULL},
        {"trimDesign", NULL, js_trim_design, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineLaunchCounts", NULL, js_pipeline_launch_counts, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineWalkSubmit", NULL, js_pipeline_walk_submit, NULL, NULL, NULL, napi_default, NULL},
        {"pipelineWalkCollect", NULL, js_pipeline_walk_collect, NULL, NULL, NULL, napi_default, NULL},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
