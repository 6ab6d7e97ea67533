/*
 * limiter_tp_emu.cpp — the source of the limiter with a true-peak detector (aac.js_amd/csrc/aacg_pcm_limit_tp.h: limit_tp_detect_body and
 * limit_tp_walk_body, the bodies the host's switch would launch, one behind the other) run lane by lane on CPU threads
 * (tests/emu/devport_emu.h, tests/emu/devport_limit_emu.h) over packed PCM buffers, per-stream records, a table, the two state blocks and
 * a scratch that the test made, for tests/test_pcm_limiter_tp_emu.py, which compiles it into a library of its own and applies the rule
 * in numpy float32 (tests/limiter_tp_kit.py).
 * With -DLIMITER_TP_EMU_MAIN the same driver is a program: a ragged batch, int16 and f32, 1, 2, 3 and 8 channels over exactly sized heap
 * blocks, for a build with -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_limit_tp.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of the detector's workgroup and of the walk's, streams of a walk's workgroup, bytes of
 * a stream's record, floats in front of a state buffer's held block, samples of a block, floats of scratch a frame, the detector's LDS of
 * a channel count (0 .. 8) */
void emu_limit_tp_sizes(uint32_t out[16])
{
    out[0] = AACG_LIMIT_TP_THREADS; out[1] = AACG_LIMIT_THREADS; out[2] = AACG_LIMIT_WAVES; out[3] = (uint32_t)sizeof(aacg_limit_stream);
    out[4] = AACG_LIMIT_STATE_HEAD; out[5] = AACG_LIMIT_BLOCK; out[6] = AACG_LIMIT_TP_FRAME_BLOCKS;
    for (uint32_t c = 0; c <= 8; c++) out[7 + c] = AACG_LIMIT_TP_LDS_BYTES(c);
}

/* One pair of launches: the detector in `detect_blocks` workgroups, then the walk in `walk_blocks`, each run in the order given by
 * `reverse` (workgroups of a launch run in any order).  Returns 0 if no body serves the launch. */
int emu_limit_tp(const void* src, void* dst, const void* rec, uint32_t n_streams, float* state, float* hist, float* peak, const float* table,
                 uint32_t phases, uint32_t taps, float ceiling, float release, uint32_t channels, uint32_t elem, uint32_t detect_blocks,
                 uint32_t walk_blocks, int reverse)
{
    if (!n_streams || !detect_blocks || !walk_blocks || !aacg_limit_config_ok(ceiling, release) || aacg_truepeak_check(phases, taps)) return 0;
    aacg_limit_tp_args A;
    A.lim.src = src; A.lim.dst = dst; A.lim.rec = (const aacg_limit_stream*)rec; A.lim.state = state; A.lim.n_streams = n_streams; A.lim.n_frames = 0;
    for (uint32_t k = 0; k < n_streams; k++) A.lim.n_frames += A.lim.rec[k].frames;
    A.lim.ceiling = ceiling; A.lim.release = release; A.lim.channels = channels; A.lim.elem = elem;
    A.table = table; A.hist = hist; A.peak = peak; A.phases = phases; A.taps = taps;
    const int order = reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD;
    int ran = 0;
    /* the bodies the host's switch picks (aacg_limit_tp_launch): the detector with its static LDS, the walk with none */
#define EMU_LIMIT_TP_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { \
        ran = 1; \
        emu_launch((int)detect_blocks, AACG_LIMIT_TP_THREADS, AACG_LIMIT_TP_LDS_BYTES(C), order, [&] { aacg_pipe::limit_tp_detect_body<T, C>(A, detect_blocks); }); \
        emu_launch((int)walk_blocks, AACG_LIMIT_THREADS, 0, order, [&] { aacg_pipe::limit_tp_walk_body<T, C>(A, walk_blocks); }); \
    }
    AACG_LIMIT_BODIES(EMU_LIMIT_TP_RUN)
    return ran;
}

}  // extern "C"

#ifdef LIMITER_TP_EMU_MAIN
/* one case: the ragged batch of three streams (1, 3 and 2 frames; the second not fresh, with a state of zeros and nodes at 1) over heap
 * blocks of exactly the buffers' sizes.  The table is two phases of four taps, (1, 0, 0, 0) and (0, -2, 0, 0), so a sample's detector value
 * is max(|x[j]|, 2 |x[j - 1]|) and D = 2; the samples are small integers over 2^6 (int16: over 2^15), the ceiling is so high that no block
 * limits, the gain is 1 and the release 1: what leaves is the input delayed by 64 + 2 samples, and the scratch is checked in double. */
template <typename T>
static int one_case(uint32_t C, uint32_t detect_blocks, uint32_t walk_blocks, int reverse)
{
    const uint32_t frames[3] = {1, 3, 2}, taps = 4, phases = 2, D = taps / 2, delay = AACG_LIMIT_BLOCK + D;
    aacg_limit_stream* rec = (aacg_limit_stream*)malloc(3 * sizeof(aacg_limit_stream));
    if (!rec) return 2;
    uint32_t first = 0;
    for (uint32_t s = 0; s < 3; s++) { rec[s] = {first, frames[s], s, s & 1u, s == 1 ? 0u : 1u, 1.0f, {0u, 0u}}; first += frames[s]; }
    const size_t n = (size_t)first * 1024 * C, SF = AACG_LIMIT_STATE(C), H = AACG_LIMIT_TP_HIST(taps, C), n_peak = (size_t)first * AACG_LIMIT_TP_FRAME_BLOCKS;
    T* src = (T*)aligned_alloc(16, n * sizeof(T));
    T* dst = (T*)aligned_alloc(16, n * sizeof(T));
    float* state = (float*)aligned_alloc(16, 3 * 2 * SF * sizeof(float));
    float* hist = (float*)calloc(3 * 2 * H, sizeof(float));
    float* peak = (float*)malloc(n_peak * sizeof(float));
    float* table = (float*)aligned_alloc(16, phases * taps * sizeof(float));
    if (!src || !dst || !state || !hist || !peak || !table) return 2;
    const float h[8] = {1, 0, 0, 0, 0, -2, 0, 0};
    std::memcpy(table, h, sizeof h);
    for (size_t i = 0; i < 3 * 2 * SF; i++) state[i] = 0.0f;
    state[(1 * 2 + 1) * SF] = state[(1 * 2 + 1) * SF + 1] = 1.0f;       /* stream 1 reads parity 1: a0 = th = 1, a held block of zeros */
    const double scale = sizeof(T) == 2 ? 1.0 / 32768.0 : 1.0 / 64.0;
    for (size_t i = 0; i < n; i++) { const int v = (int)((i * 7u + 1u) % 13u) - 6; src[i] = sizeof(T) == 2 ? (T)v : (T)((double)v / 64.0); }
    std::memset(dst, 0x55, n * sizeof(T));
    const int ran = emu_limit_tp(src, dst, rec, 3, state, hist, peak, table, phases, taps, 1000.0f, 1.0f, C, (uint32_t)sizeof(T), detect_blocks, walk_blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < 3; s++) {
        const size_t base = (size_t)rec[s].frame_first * 1024, len = (size_t)frames[s] * 1024;
        auto x = [&](ptrdiff_t j, uint32_t c) { return j < 0 ? 0.0 : (double)(sizeof(T) == 2 ? (double)src[(base + (size_t)j) * C + c] : (double)src[(base + (size_t)j) * C + c] * 64.0) * scale; };
        for (size_t j = 0; j < len; j++)
            for (uint32_t c = 0; c < C; c++) {
                const double got = (double)dst[(base + j) * C + c] * (sizeof(T) == 2 ? 1.0 / 32768.0 : 1.0);
                wrong += got != x((ptrdiff_t)j - (ptrdiff_t)delay, c);
            }
        for (size_t b = 0; b < len / AACG_LIMIT_BLOCK; b++) {
            double p = 0.0;
            for (size_t j = b * AACG_LIMIT_BLOCK; j < (b + 1) * AACG_LIMIT_BLOCK; j++)
                for (uint32_t c = 0; c < C; c++) {
                    const double v[3] = {std::fabs(x((ptrdiff_t)j - (ptrdiff_t)D, c)), std::fabs(x((ptrdiff_t)j, c)), 2.0 * std::fabs(x((ptrdiff_t)j - 1, c))};
                    for (double q : v) p = q > p ? q : p;
                }
            wrong += (double)peak[(size_t)rec[s].frame_first * AACG_LIMIT_TP_FRAME_BLOCKS + b] != p;
        }
        const float* st = state + ((size_t)s * 2 + ((s & 1u) ^ 1u)) * SF;
        wrong += st[0] != 1.0f || st[1] != 1.0f;
        for (uint32_t i = 0; i < AACG_LIMIT_BLOCK; i++)                   /* the held block: z's last, x[len - 64 - D + i] */
            for (uint32_t c = 0; c < C; c++) wrong += (double)st[AACG_LIMIT_STATE_HEAD + i * C + c] != x((ptrdiff_t)(len - AACG_LIMIT_BLOCK - D + i), c);
        const float* hs = hist + ((size_t)s * 2 + ((s & 1u) ^ 1u)) * H;
        for (uint32_t t = 0; t + 1 < taps; t++)                           /* ... and the last three samples */
            for (uint32_t c = 0; c < C; c++) wrong += (double)hs[(size_t)t * C + c] != x((ptrdiff_t)(len - (taps - 1) + t), c);
    }
    free(src); free(dst); free(state); free(hist); free(peak); free(table); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "limiter_tp_emu: %u channels of %zu bytes, %u and %u workgroups%s: %zu values differ\n", C, sizeof(T), detect_blocks, walk_blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 2u, 3u, 8u}) {
        bad |= one_case<int16_t>(C, 1, 1, 0);
        bad |= one_case<float>(C, 2, 2, 1);
        bad |= one_case<float>(C, 7, 1, 0);
        bad |= one_case<int16_t>(C, 6, 3, 1);
    }
    std::printf(bad ? "limiter_tp_emu: FAILED\n" : "limiter_tp_emu: ok\n");
    return bad;
}
#endif
