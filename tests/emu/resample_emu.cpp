/*
 * resample_emu.cpp — the PCM resample kernel's source (aac.js_amd/csrc/aacg_pcm_resample.h: resample_body, the body the host's switch
 * would launch) run lane by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer, a table, per-stream records and a
 * history block that the test made, for tests/test_pcm_resample_emu.py, which compiles it into a library of its own and applies the rule
 * in numpy float32.  With -DRESAMPLE_EMU_MAIN the same driver is a program: int16 and f32 cases of 1, 2, 3 and 8 channels over exactly
 * sized heap blocks, for a build with -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_resample.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, bytes of a stream's record, the largest tap count */
void emu_resample_sizes(uint32_t out[3]) { out[0] = AACG_RESAMPLE_THREADS; out[1] = (uint32_t)sizeof(aacg_resample_stream); out[2] = AACG_RESAMPLE_MAX_TAPS; }

/* the limits as the host's part checks them: 0, or which one (L, M, taps) breaks */
int emu_resample_check(uint32_t L, uint32_t M, uint32_t taps) { return aacg_resample_check(L, M, taps); }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order).  Returns 0 if no
 * body serves the launch. */
int emu_resample(const void* src, void* dst, const void* rec, uint32_t n_streams, uint32_t n_frames, const float* table, float* hist,
                 uint32_t L, uint32_t M, uint32_t taps, uint32_t row, uint32_t channels, uint32_t elem, uint32_t blocks, int reverse)
{
    if (aacg_resample_check(L, M, taps) || !n_frames || !n_streams) return 0;
    aacg_resample_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_resample_stream*)rec; A.table = table; A.hist = hist;
    A.n_streams = n_streams; A.n_frames = n_frames; A.L = L; A.M = M; A.taps = taps; A.row = row; A.channels = channels; A.elem = elem;
    int ran = 0;
    /* the body the host's switch picks (aacg_resample_launch), in workgroups of AACG_RESAMPLE_THREADS lanes with the body's static LDS */
#define EMU_RESAMPLE_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { ran = 1; emu_launch((int)blocks, AACG_RESAMPLE_THREADS, AACG_RESAMPLE_LDS_BYTES(C), reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::resample_body<T, C>(A, blocks); }); }
    AACG_RESAMPLE_BODIES(EMU_RESAMPLE_RUN)
    return ran;
}

}  // extern "C"

#ifdef RESAMPLE_EMU_MAIN
/* one case: two streams (2 frames fresh, 1 frame mid-phase with a history) over heap blocks of exactly the buffers' sizes; every row of
 * the table is (1, 0, 0, ...), so an output is the input sample it stands on and is checked here */
template <typename T>
static int one_case(uint32_t C, uint32_t L, uint32_t M, uint32_t taps, int planar, uint32_t blocks, int reverse)
{
    const uint32_t frames[2] = {2, 1}, n0[2] = {0, 7 % M};
    aacg_resample_stream* rec = (aacg_resample_stream*)malloc(2 * sizeof(aacg_resample_stream));
    uint32_t total = 0, longest = 0;
    for (uint32_t s = 0; s < 2; s++) {
        const uint32_t n = aacg_resample_ceil(n0[s] + 1024u * frames[s], L, M) - aacg_resample_ceil(n0[s], L, M);
        rec[s] = {s ? frames[0] : 0u, frames[s], total, n, n0[s], s, s, s ? 0u : 1u};
        total += n;
        if (n > longest) longest = n;
    }
    const uint32_t row = planar ? ((longest + 1023u) / 1024u) * 1024u : 0u;
    const size_t n_src = (size_t)3 * 1024 * C, n_dst = planar ? (size_t)2 * C * row : (size_t)total * C, n_hist = (size_t)2 * 2 * (taps - 1) * C;
    T* src = (T*)aligned_alloc(16, n_src * sizeof(T));
    T* dst = (T*)malloc(n_dst * sizeof(T));               /* (16-byte aligned as malloc makes it; exactly sized, ragged as the output is) */
    float* table = (float*)aligned_alloc(16, (size_t)L * taps * sizeof(float));
    float* hist = (float*)malloc(n_hist * sizeof(float));
    if (!src || !dst || !table || !hist || !rec) return 2;
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int16_t)(uint16_t)(i * 7u + 1u);
    for (size_t i = 0; i < n_hist; i++) hist[i] = (float)(int)(i % 97u);
    for (uint32_t p = 0; p < L; p++) for (uint32_t t = 0; t < taps; t++) table[(size_t)p * taps + t] = t ? 0.0f : 1.0f;
    std::memset(dst, 0x7f, n_dst * sizeof(T));
    const int ran = emu_resample(src, dst, rec, 2, 3, table, hist, L, M, taps, row, C, (uint32_t)sizeof(T), blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < 2; s++) {
        const uint32_t m0 = aacg_resample_ceil(n0[s], L, M);
        for (uint32_t j = 0; j < (planar ? row : rec[s].n_out); j++)
            for (uint32_t c = 0; c < C; c++) {
                const T got = planar ? dst[((size_t)s * C + c) * row + j] : dst[((size_t)rec[s].out_first + j) * C + c];
                const size_t i = (size_t)((uint64_t)(m0 + j) * M / L) - n0[s];
                const T want = j < rec[s].n_out ? src[((size_t)rec[s].frame_first * 1024 + i) * C + c] : (T)0;
                wrong += got != want;
            }
    }
    free(src); free(dst); free(table); free(hist); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "resample_emu: %u channels of %zu bytes, %u / %u, %u taps, %s, %u workgroups%s: %zu elements differ\n", C, sizeof(T), L, M, taps,
                                    planar ? "planar" : "packed", blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 2u, 3u, 8u}) {
        bad |= one_case<int16_t>(C, 1, 3, 4, 0, 1, 0);
        bad |= one_case<int16_t>(C, 160, 441, 32, 1, 2, 1);
        bad |= one_case<float>(C, 2, 1, 64, 0, 3, 0);
        bad |= one_case<float>(C, 160, 147, 8, 1, 5, 1);
    }
    std::printf(bad ? "resample_emu: FAILED\n" : "resample_emu: ok\n");
    return bad;
}
#endif
