/*
 * aacg_engine_mix.hip — a resident batch's packed PCM mixed to one or two channels on the device (aacg_pcm_mix.h: mix_body): ONE launch
 * per batch of a pipeline with a mix matrix (aacg_pipeline_set_mix, include/aacgpu.h) on the lane's stream behind aacg_pipeline_join
 * writes [frame][1024][O] from the lane's [frame][1024][C].  One lane per 16 bytes of every input channel; non-temporal vector loads,
 * plain vector stores; the matrix by value in the kernel's arguments.
 *
 * Thirty-two kernel entries, one per body (f32 / int16 x 1..8 channels in x 1 or 2 out: aacg_pcm_mix_f32_c1_o1 ..
 * aacg_pcm_mix_i16_c8_o2), switched on the host; each has its row in the Makefile's gate.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_mix.h"

#define AACG_MIX_KERNEL(T, NAME, C, O) \
    extern "C" __global__ __launch_bounds__(AACG_MIX_THREADS) void aacg_pcm_mix_##NAME##_c##C##_o##O(const aacg_mix_args A) { aacg_pipe::mix_body<T, C, O>(A, gridDim.x); }
AACG_MIX_BODIES(AACG_MIX_KERNEL)

/* false: not a launch these kernels serve (channels in or out, element size, or more items than a body counts) — nothing is enqueued */
bool aacg_mix_launch(const aacg_mix_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_mix_args) = nullptr;
#define AACG_MIX_PICK(T, NAME, C, O) if (A.elem == sizeof(T) && A.channels == C && A.out_channels == O) kernel = aacg_pcm_mix_##NAME##_c##C##_o##O;
    AACG_MIX_BODIES(AACG_MIX_PICK)
    const uint32_t items = kernel ? aacg_mix_items(A.n_frames, A.elem) : 0u;
    if (!items) return false;
    const uint32_t want = (items + AACG_MIX_THREADS - 1u) / AACG_MIX_THREADS, blocks = want < AACG_MIX_MAX_BLOCKS ? want : AACG_MIX_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_MIX_THREADS), 0, s, A);
    return true;
}
