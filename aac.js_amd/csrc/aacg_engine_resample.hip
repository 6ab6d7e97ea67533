/*
 * aacg_engine_resample.hip — a resident batch's packed PCM resampled by L / M on the device (aacg_pcm_resample.h: resample_body): ONE
 * launch per batch of a pipeline with a resampler (aacg_pipeline_set_resample, include/aacgpu.h) on the lane's stream behind
 * aacg_pipeline_join and the mix.  One workgroup per input frame: the frame and the T - 1 samples in front of it in LDS as floats, a
 * lane per output sample with all its channels, the phase rows through the cache; packed or planar out, ragged per stream.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_resample_f32_c1 .. aacg_pcm_resample_i16_c8), switched on
 * the host; each has its row in the Makefile's gate, with its LDS.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_resample.h"

#define AACG_RESAMPLE_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_RESAMPLE_THREADS) void aacg_pcm_resample_##NAME##_c##C(const aacg_resample_args A) { aacg_pipe::resample_body<T, C>(A, gridDim.x); }
AACG_RESAMPLE_BODIES(AACG_RESAMPLE_KERNEL)

/* false: not a launch these kernels serve (channels, element size, a table outside the limits, no frame) — nothing is enqueued */
bool aacg_resample_launch(const aacg_resample_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_resample_args) = nullptr;
#define AACG_RESAMPLE_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_resample_##NAME##_c##C;
    AACG_RESAMPLE_BODIES(AACG_RESAMPLE_PICK)
    if (!kernel || !A.n_frames || !A.n_streams || aacg_resample_check(A.L, A.M, A.taps)) return false;
    const uint32_t blocks = A.n_frames < AACG_RESAMPLE_MAX_BLOCKS ? A.n_frames : AACG_RESAMPLE_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_RESAMPLE_THREADS), 0, s, A);
    return true;
}
