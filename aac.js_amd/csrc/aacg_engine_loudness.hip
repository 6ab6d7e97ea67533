/*
 * aacg_engine_loudness.hip — a loudness tap on a resident batch's transform PCM (aacg_pcm_loudness.h: loudness_body): ONE launch per
 * batch of a pipeline with a meter (aacg_pipeline_set_loudness, include/aacgpu.h) on the lane's stream behind aacg_pipeline_join.  One
 * wave per workgroup, a lane per (stream, channel) chain, 64 / C streams a workgroup; the PCM through LDS in tiles of 32 samples, two
 * floats per hop and channel out.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_loudness_f32_c1 .. aacg_pcm_loudness_i16_c8), switched on
 * the host; each has its row in the Makefile's gate, with its LDS.  The unit is built without any flush-to-zero flag: subnormals are
 * part of the rule.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_loudness.h"

#define AACG_LOUDNESS_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_LOUDNESS_THREADS) void aacg_pcm_loudness_##NAME##_c##C(const aacg_loudness_args A) { aacg_pipe::loudness_body<T, C>(A, gridDim.x); }
AACG_LOUDNESS_BODIES(AACG_LOUDNESS_KERNEL)

/* false: not a launch these kernels serve (channels, element size, a hop outside the limits, no stream, 64 GiB of PCM or more) — nothing is enqueued */
bool aacg_loudness_launch(const aacg_loudness_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_loudness_args) = nullptr;
#define AACG_LOUDNESS_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_loudness_##NAME##_c##C;
    AACG_LOUDNESS_BODIES(AACG_LOUDNESS_PICK)
    if (!kernel || !A.n_streams || !A.n_frames || A.hop < 1u || A.hop > AACG_LOUDNESS_MAX_HOP) return false;
    if ((uint64_t)A.n_frames * (1024u * A.channels * A.elem / 16u) > AACG_LOUDNESS_MAX_VECTORS) return false;
    const uint32_t G = 64u / A.channels, groups = (A.n_streams + G - 1u) / G;
    const uint32_t blocks = groups < AACG_LOUDNESS_MAX_BLOCKS ? groups : AACG_LOUDNESS_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_LOUDNESS_THREADS), 0, s, A);
    return true;
}
