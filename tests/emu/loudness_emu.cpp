/*
 * loudness_emu.cpp — the loudness tap's source (aac.js_amd/csrc/aacg_pcm_loudness.h: loudness_body, the body the host's switch would
 * launch) run lane by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer, per-stream records and a state block that
 * the test made, for tests/test_pcm_loudness_emu.py, which compiles it into a library of its own and applies the rule in numpy float32.
 * With -DLOUDNESS_EMU_MAIN the same driver is a program: a ragged batch, int16 and f32, 1, 2, 3 and 8 channels over exactly sized heap
 * blocks, for a build with -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_loudness.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, bytes of a stream's record, floats of a chain's state, the LDS */
void emu_loudness_sizes(uint32_t out[4]) { out[0] = AACG_LOUDNESS_THREADS; out[1] = (uint32_t)sizeof(aacg_loudness_stream); out[2] = AACG_LOUDNESS_STATE; out[3] = AACG_LOUDNESS_LDS_BYTES; }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order).  Returns 0 if no
 * body serves the launch. */
int emu_loudness(const void* src, float* dst, const void* rec, uint32_t n_streams, float* state, uint32_t hop, const float* coeffs,
                 uint32_t channels, uint32_t elem, uint32_t blocks, int reverse)
{
    if (!n_streams || hop < 1u || hop > AACG_LOUDNESS_MAX_HOP || !blocks) return 0;
    aacg_loudness_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_loudness_stream*)rec; A.state = state; A.n_streams = n_streams; A.n_frames = 0; A.hop = hop;
    for (uint32_t k = 0; k < n_streams; k++) A.n_frames += A.rec[k].frames;
    std::memcpy(A.coeffs, coeffs, sizeof A.coeffs);
    A.channels = channels; A.elem = elem;
    int ran = 0;
    /* the body the host's switch picks (aacg_loudness_launch), in workgroups of one wave with the body's static LDS */
#define EMU_LOUDNESS_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { ran = 1; emu_launch((int)blocks, AACG_LOUDNESS_THREADS, AACG_LOUDNESS_LDS_BYTES, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::loudness_body<T, C>(A, blocks); }); }
    AACG_LOUDNESS_BODIES(EMU_LOUDNESS_RUN)
    return ran;
}

}  // extern "C"

#ifdef LOUDNESS_EMU_MAIN
/* one case: the ragged batch of three streams (1, 3 and 2 frames; the second in mid-hop with a state) over heap blocks of exactly the
 * buffers' sizes; the sections are (1, 0, 0, 0, 0) twice, so a record is the hop's sum of squares and its peak, checked here in double
 * (the samples are small integers over 2^15 or small integers: every sum is exact) */
template <typename T>
static int one_case(uint32_t C, uint32_t hop, uint32_t blocks, int reverse)
{
    const uint32_t frames[3] = {1, 3, 2}, n0[3] = {0, 7 % hop, 0};
    aacg_loudness_stream* rec = (aacg_loudness_stream*)malloc(3 * sizeof(aacg_loudness_stream));
    uint32_t total = 0, first = 0;
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t n = (uint32_t)aacg_loudness_emits(hop, n0[s], 1024ull * frames[s]);
        rec[s] = {first, frames[s], total, n, n0[s], s, s & 1u, s == 1 ? 0u : 1u};
        total += n; first += frames[s];
    }
    const size_t n_src = (size_t)first * 1024 * C, n_dst = (size_t)total * C * 2, n_state = (size_t)3 * 2 * C * AACG_LOUDNESS_STATE;
    T* src = (T*)aligned_alloc(16, n_src * sizeof(T));
    float* dst = (float*)malloc(n_dst * sizeof(float) + 8);              /* (exactly sized, ragged as the output is; + 8: never a malloc of 0) */
    float* state = (float*)malloc(n_state * sizeof(float));
    if (!src || !dst || !state || !rec) return 2;
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int)((i * 7u + 1u) % 13u) - (T)6;
    for (size_t i = 0; i < n_state; i++) state[i] = 0.0f;                /* stream 1's partial hop: seven samples of nothing */
    const float coeffs[10] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0};
    const double scale = sizeof(T) == 2 ? 1.0 / 32768.0 : 1.0;
    const int ran = emu_loudness(src, dst, rec, 3, state, hop, coeffs, C, (uint32_t)sizeof(T), blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < 3; s++)
        for (uint32_t c = 0; c < C; c++) {
            double e = 0.0, pk = 0.0;
            uint32_t left = hop - n0[s], j = 0;
            for (uint32_t i = 0; i < 1024u * frames[s]; i++) {
                const double v = (double)src[((size_t)rec[s].frame_first * 1024 + i) * C + c] * scale;
                e += v * v; pk = std::fabs(v) > pk ? std::fabs(v) : pk;
                if (--left == 0) {
                    const float* got = dst + (((size_t)rec[s].out_first + j) * C + c) * 2;
                    wrong += (double)got[0] != e || (double)got[1] != pk;
                    j++; e = pk = 0.0; left = hop;
                }
            }
            wrong += j != rec[s].n_out;
            const float* st = state + (((size_t)s * 2 + ((s & 1u) ^ 1u)) * C + c) * AACG_LOUDNESS_STATE;
            wrong += (double)st[4] != e || (double)st[5] != pk;
        }
    free(src); free(dst); free(state); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "loudness_emu: %u channels of %zu bytes, hop %u, %u workgroups%s: %zu values differ\n", C, sizeof(T), hop, blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 2u, 3u, 8u}) {
        bad |= one_case<int16_t>(C, 1000, 1, 0);
        bad |= one_case<float>(C, 7, 2, 1);
        bad |= one_case<float>(C, 4800, 3, 0);
        bad |= one_case<int16_t>(C, 1024, 1, 1);
    }
    std::printf(bad ? "loudness_emu: FAILED\n" : "loudness_emu: ok\n");
    return bad;
}
#endif
