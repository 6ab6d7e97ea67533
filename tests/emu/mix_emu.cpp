/*
 * mix_emu.cpp — the PCM mix kernel's source (aac.js_amd/csrc/aacg_pcm_mix.h: mix_body, the body the host's switch would launch) run lane
 * by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer and a matrix that the test made, for
 * tests/test_pcm_mix_emu.py, which compiles it into a library of its own and applies the rule in numpy float32.  With -DMIX_EMU_MAIN the
 * same driver is a program: int16 and f32 cases of 1, 3, 6 and 7 channels over exactly sized heap blocks, for a build with
 * -fsanitize=address,undefined (a vector access that is out of bounds or not naturally aligned ends it).  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_mix.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* AACG_MIX_THREADS and the matrix's places in the launch arguments: what the test lays its launches out by */
void emu_mix_sizes(uint32_t out[2]) { out[0] = AACG_MIX_THREADS; out[1] = AACG_MIX_MAX_OUT * AACG_MIX_MAX_IN; }

/* the items of a launch as the host's part counts them (0: more than the kernel counts) */
uint32_t emu_mix_items(uint32_t n_frames, uint32_t elem) { return aacg_mix_items(n_frames, elem); }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order); matrix: out_channels
 * rows of `channels` floats.  Returns 0 if no body serves the launch. */
int emu_mix(const void* src, void* dst, uint32_t n_frames, uint32_t channels, uint32_t out_channels, uint32_t elem, const float* matrix, uint32_t blocks, int reverse)
{
    if (channels < 1 || channels > AACG_MIX_MAX_IN || out_channels < 1 || out_channels > AACG_MIX_MAX_OUT) return 0;
    aacg_mix_args A;
    A.src = src; A.dst = dst; A.n_frames = n_frames; A.channels = channels; A.out_channels = out_channels; A.elem = elem;
    std::memset(A.m, 0, sizeof A.m);
    std::memcpy(A.m, matrix, (size_t)channels * out_channels * sizeof(float));
    int ran = 0;
    /* the body the host's switch picks (aacg_mix_launch), in workgroups of AACG_MIX_THREADS lanes as hipLaunchKernelGGL runs them */
#define EMU_MIX_RUN(T, NAME, C, O) \
    if (elem == sizeof(T) && channels == C && out_channels == O) { ran = 1; emu_launch((int)blocks, AACG_MIX_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::mix_body<T, C, O>(A, blocks); }); }
    AACG_MIX_BODIES(EMU_MIX_RUN)
    return ran;
}

}  // extern "C"

#ifdef MIX_EMU_MAIN
/* one case: heap blocks of exactly the source's and the destination's size (16-byte aligned); coefficients of 1 and 0 pick channel
 * o (modulo C) for output o, so the mix is a copy of that channel and is checked here */
template <typename T>
static int one_case(uint32_t C, uint32_t O, uint32_t frames, uint32_t blocks, int reverse)
{
    const size_t n = (size_t)frames * 1024, n_src = n * C, n_dst = n * O;
    T* src = (T*)aligned_alloc(16, n_src * sizeof(T));
    T* dst = (T*)aligned_alloc(16, n_dst * sizeof(T));
    if (!src || !dst) return 2;
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int16_t)(uint16_t)(i * 7u + 1u);
    std::memset(dst, 0x7f, n_dst * sizeof(T));
    float m[16] = {};
    for (uint32_t o = 0; o < O; o++) m[o * C + o % C] = 1.0f;
    const int ran = emu_mix(src, dst, frames, C, O, (uint32_t)sizeof(T), m, blocks, reverse);
    size_t wrong = 0;
    for (size_t t = 0; t < n; t++)
        for (uint32_t o = 0; o < O; o++) wrong += dst[t * O + o] != src[t * C + o % C];
    free(src);
    free(dst);
    if (wrong || !ran) std::fprintf(stderr, "mix_emu: %u -> %u channels of %zu bytes, %u frames, %u workgroups%s: %zu elements differ\n", C, O, sizeof(T), frames, blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 3u, 6u, 7u})
        for (uint32_t O : {1u, 2u}) {
            bad |= one_case<int16_t>(C, O, 1, 1, 0);
            bad |= one_case<int16_t>(C, O, 3, 2, 1);
            bad |= one_case<float>(C, O, 1, 3, 0);
            bad |= one_case<float>(C, O, 2, 1, 1);
        }
    std::printf(bad ? "mix_emu: FAILED\n" : "mix_emu: ok\n");
    return bad;
}
#endif
