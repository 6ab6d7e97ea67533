/*
 * truepeak_emu.cpp — the true-peak stage's source (aac.js_amd/csrc/aacg_pcm_truepeak.h: truepeak_body, the body the host's switch would
 * launch) run lane by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer, the meter's per-stream records, a table
 * and a state block that the test made, for tests/test_pcm_truepeak_emu.py, which compiles it into a library of its own and applies the
 * rule in numpy float32 (tests/truepeak_kit.py).
 * With -DTRUEPEAK_EMU_MAIN the same driver is a program: a ragged batch, int16 and f32, 1, 2, 3 and 8 channels over exactly sized heap
 * blocks, for a build with -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_truepeak.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, bytes of a stream's record, the LDS of a channel count (0 .. 8) */
void emu_truepeak_sizes(uint32_t out[11])
{
    out[0] = AACG_TRUEPEAK_THREADS; out[1] = (uint32_t)sizeof(aacg_loudness_stream);
    for (uint32_t c = 0; c <= 8; c++) out[2 + c] = AACG_TRUEPEAK_LDS_BYTES(c);
}

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order).  dst is zero when
 * it arrives, as the host clears it.  Returns 0 if no body serves the launch. */
int emu_truepeak(const void* src, uint32_t* dst, const void* rec, uint32_t n_streams, const float* table, float* state, uint32_t hop,
                 uint32_t phases, uint32_t taps, uint32_t channels, uint32_t elem, uint32_t blocks, int reverse)
{
    if (!n_streams || hop < 1u || hop > AACG_LOUDNESS_MAX_HOP || !blocks || aacg_truepeak_check(phases, taps)) return 0;
    aacg_truepeak_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_loudness_stream*)rec; A.table = table; A.state = state; A.n_streams = n_streams; A.n_frames = 0;
    A.hop = hop; A.phases = phases; A.taps = taps;
    for (uint32_t k = 0; k < n_streams; k++) A.n_frames += A.rec[k].frames;
    A.channels = channels; A.elem = elem;
    int ran = 0;
    /* the body the host's switch picks (aacg_truepeak_launch), in workgroups of four waves with the body's static LDS */
#define EMU_TRUEPEAK_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { ran = 1; emu_launch((int)blocks, AACG_TRUEPEAK_THREADS, AACG_TRUEPEAK_LDS_BYTES(C), reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::truepeak_body<T, C>(A, blocks); }); }
    AACG_TRUEPEAK_BODIES(EMU_TRUEPEAK_RUN)
    return ran;
}

}  // extern "C"

#ifdef TRUEPEAK_EMU_MAIN
/* one case: the ragged batch of three streams (1, 3 and 2 frames; the second in mid-hop with a state of zeros) over heap blocks of exactly
 * the buffers' sizes; the table is two phases of four taps, (1, 0, 0, 0) and (0, -2, 0, 0), so a sample's value is max(|x[i]|, 2 |x[i - 1]|),
 * checked here in double (the samples are small integers over 2^15 or small integers: everything is exact) */
template <typename T>
static int one_case(uint32_t C, uint32_t hop, uint32_t blocks, int reverse)
{
    const uint32_t frames[3] = {1, 3, 2}, n0[3] = {0, 7 % hop, 0}, taps = 4, phases = 2;
    aacg_loudness_stream* rec = (aacg_loudness_stream*)malloc(3 * sizeof(aacg_loudness_stream));
    if (!rec) return 2;
    uint32_t total = 0, first = 0;
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t n = (uint32_t)aacg_loudness_emits(hop, n0[s], 1024ull * frames[s]);
        rec[s] = {first, frames[s], total, n, n0[s], s, s & 1u, s == 1 ? 0u : 1u};
        total += n; first += frames[s];
    }
    const size_t n_src = (size_t)first * 1024 * C, n_dst = (size_t)total * C, SZ = AACG_TRUEPEAK_STATE(taps, C), n_state = (size_t)3 * 2 * SZ;
    T* src = (T*)aligned_alloc(16, n_src * sizeof(T));
    uint32_t* dst = (uint32_t*)calloc(n_dst + 2, sizeof(uint32_t));      /* (exactly sized, ragged as the output is; + 2: never an allocation of 0) */
    float* state = (float*)calloc(n_state, sizeof(float));               /* stream 1's history and partial: seven samples of nothing */
    float* table = (float*)aligned_alloc(16, phases * taps * sizeof(float));
    if (!src || !dst || !state || !table) return 2;
    const float h[8] = {1, 0, 0, 0, 0, -2, 0, 0};
    std::memcpy(table, h, sizeof h);
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int)((i * 7u + 1u) % 13u) - (T)6;
    const double scale = sizeof(T) == 2 ? 1.0 / 32768.0 : 1.0;
    const int ran = emu_truepeak(src, dst, rec, 3, table, state, hop, phases, taps, C, (uint32_t)sizeof(T), blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < 3; s++)
        for (uint32_t c = 0; c < C; c++) {
            double tp = 0.0, before = 0.0;
            uint32_t left = hop - n0[s], j = 0;
            for (uint32_t i = 0; i < 1024u * frames[s]; i++) {
                const double v = (double)src[((size_t)rec[s].frame_first * 1024 + i) * C + c] * scale;
                const double m = std::fabs(v) > 2.0 * std::fabs(before) ? std::fabs(v) : 2.0 * std::fabs(before);
                tp = m > tp ? m : tp; before = v;
                if (--left == 0) {
                    float got; std::memcpy(&got, dst + ((size_t)rec[s].out_first + j) * C + c, 4);
                    wrong += (double)got != tp;
                    j++; tp = 0.0; left = hop;
                }
            }
            wrong += j != rec[s].n_out;
            const float* st = state + ((size_t)s * 2 + ((s & 1u) ^ 1u)) * SZ;
            wrong += (double)st[(size_t)(taps - 1) * C + c] != tp;        /* the partial maximum left behind */
            for (uint32_t t = 0; t + 1 < taps; t++)                       /* ... and the last three samples */
                wrong += (double)st[(size_t)t * C + c] != (double)src[((size_t)(rec[s].frame_first + frames[s]) * 1024 - (taps - 1) + t) * C + c] * scale;
        }
    free(src); free(dst); free(state); free(table); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "truepeak_emu: %u channels of %zu bytes, hop %u, %u workgroups%s: %zu values differ\n", C, sizeof(T), hop, blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 2u, 3u, 8u}) {
        bad |= one_case<int16_t>(C, 1000, 1, 0);
        bad |= one_case<float>(C, 7, 2, 1);
        bad |= one_case<float>(C, 4800, 3, 0);
        bad |= one_case<int16_t>(C, 1024, 6, 1);
    }
    std::printf(bad ? "truepeak_emu: FAILED\n" : "truepeak_emu: ok\n");
    return bad;
}
#endif
