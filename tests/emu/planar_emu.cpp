/*
 * planar_emu.cpp — the planar PCM kernel's source (aac.js_amd/csrc/aacg_pcm_planar.h: planar_body, the body the host's switch would launch)
 * run lane by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer and a per-stream table that the test made, for
 * tests/test_pcm_planar_emu.py, which compiles it into a library of its own and transposes in numpy.  With -DPLANAR_EMU_MAIN the
 * same driver is a program: the int16 cases of 1, 3 and 7 channels over exactly sized heap blocks, for a build with
 * -fsanitize=address,undefined (a vector access that is out of bounds or not naturally aligned ends it).  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_pcm_planar.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* AACG_PLANAR_THREADS, sizeof(aacg_pipe_stream), sizeof(aacg_shape_stream): what the test lays its launches and tables out by */
void emu_planar_sizes(uint32_t out[3]) { out[0] = AACG_PLANAR_THREADS; out[1] = (uint32_t)sizeof(aacg_pipe_stream); out[2] = (uint32_t)sizeof(aacg_shape_stream); }

/* the items of a launch as the host's part counts them (0: more than the kernel counts) */
uint32_t emu_planar_items(uint32_t n_streams, uint32_t stride_frames, uint32_t elem) { return aacg_planar_items(n_streams, stride_frames, elem); }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order). */
void emu_planar(const void* src, void* dst, const void* tab, uint32_t tab_stride, uint32_t n_streams, uint32_t stride_frames, uint32_t channels, uint32_t elem,
                uint32_t blocks, int reverse)
{
    aacg_planar_args A;
    A.src = src; A.dst = dst; A.tab = tab; A.tab_stride = tab_stride; A.n_streams = n_streams; A.stride_frames = stride_frames; A.channels = channels; A.elem = elem;
    /* the body the host's switch picks (aacg_planar_launch), in workgroups of AACG_PLANAR_THREADS lanes as hipLaunchKernelGGL runs them */
#define EMU_PLANAR_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) emu_launch((int)blocks, AACG_PLANAR_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::planar_body<T, C>(A, blocks); });
    AACG_PLANAR_BODIES(EMU_PLANAR_RUN)
}

}  // extern "C"

#ifdef PLANAR_EMU_MAIN
/* one int16 case: heap blocks of exactly the source's and the destination's size (16-byte aligned), the transposition checked here */
static int one_case(uint32_t C, const std::vector<uint32_t>& counts, uint32_t stride, uint32_t blocks, int reverse)
{
    const uint32_t S = (uint32_t)counts.size();
    uint32_t n = 0;
    std::vector<aacg_pipe_stream> tab(S);
    for (uint32_t s = 0; s < S; s++) { tab[s] = aacg_pipe_stream{n, counts[s], 0u, 0u}; n += counts[s]; }
    const size_t n_src = (size_t)n * 1024 * C, T = (size_t)stride * 1024, n_dst = (size_t)S * C * T;
    int16_t* src = (int16_t*)aligned_alloc(16, n_src * 2);
    int16_t* dst = (int16_t*)aligned_alloc(16, n_dst * 2);
    if (!src || !dst) return 2;
    for (size_t i = 0; i < n_src; i++) src[i] = (int16_t)(uint16_t)(i * 7u + 1u);
    std::memset(dst, 0x7f, n_dst * 2);
    emu_planar(src, dst, tab.data(), (uint32_t)sizeof(aacg_pipe_stream), S, stride, C, 2, blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t c = 0; c < C; c++)
            for (size_t t = 0; t < T; t++) {
                const int16_t want = t < (size_t)counts[s] * 1024 ? src[((size_t)tab[s].frame_first * 1024 + t) * C + c] : (int16_t)0;
                wrong += dst[((size_t)s * C + c) * T + t] != want;
            }
    free(src);
    free(dst);
    if (wrong) std::fprintf(stderr, "planar_emu: %u channels, %u streams, stride %u, %u workgroups%s: %zu elements differ\n", C, S, stride, blocks, reverse ? " in reverse" : "", wrong);
    return wrong ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 3u, 7u}) {
        bad |= one_case(C, {3, 1, 2}, 3, 2, 0);
        bad |= one_case(C, {3, 1, 2}, 4, 3, 1);
        bad |= one_case(C, {1}, 1, 1, 0);
        bad |= one_case(C, std::vector<uint32_t>(17, 1u), 1, 2, 1);
    }
    std::printf(bad ? "planar_emu: FAILED\n" : "planar_emu: ok\n");
    return bad;
}
#endif
