/*
 * aacg_engine_planar.hip — a resident batch's PCM into a caller's planar tensor on the device (aacg_pcm_planar.h: planar_body): ONE
 * launch per AACG_PCM_PLANAR batch on the lane's stream behind aacg_pipeline_join writes [stream][channel][stride_frames * 1024]
 * from the lane's packed PCM and the batch's per-stream table, padding included (aacg_pipeline_submit_device, include/aacgpu.h).
 * One lane per 16 bytes of every channel; non-temporal vector loads, plain vector stores.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_planar_f32_c1 .. aacg_pcm_planar_i16_c8), switched on
 * the host; each has its row in the Makefile's gate.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_planar.h"

#define AACG_PLANAR_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_PLANAR_THREADS) void aacg_pcm_planar_##NAME##_c##C(const aacg_planar_args A) { aacg_pipe::planar_body<T, C>(A, gridDim.x); }
AACG_PLANAR_BODIES(AACG_PLANAR_KERNEL)

/* false: not a launch these kernels serve (channels, element size, or more items than a body counts) — nothing is enqueued */
bool aacg_planar_launch(const aacg_planar_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_planar_args) = nullptr;
#define AACG_PLANAR_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_planar_##NAME##_c##C;
    AACG_PLANAR_BODIES(AACG_PLANAR_PICK)
    const uint32_t items = kernel ? aacg_planar_items(A.n_streams, A.stride_frames, A.elem) : 0u;
    if (!items) return false;
    const uint32_t want = (items + AACG_PLANAR_THREADS - 1u) / AACG_PLANAR_THREADS, blocks = want < AACG_PLANAR_MAX_BLOCKS ? want : AACG_PLANAR_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_PLANAR_THREADS), 0, s, A);
    return true;
}
