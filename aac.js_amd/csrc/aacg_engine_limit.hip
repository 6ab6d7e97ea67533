/*
 * aacg_engine_limit.hip — a per-stream gain and a look-ahead limiter on a resident batch's PCM (aacg_pcm_limit.h: limit_body): ONE launch
 * per batch of a pipeline with a limiter (aacg_pipeline_set_limiter, include/aacgpu.h) on the lane's stream behind the mix.  Four waves
 * per workgroup, a wave per stream, a lane per sample of a block of 64; no LDS.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_limit_f32_c1 .. aacg_pcm_limit_i16_c8), switched on the
 * host; each has its row in the Makefile's gate.  The unit is built without any flush-to-zero or fast-math flag: subnormals and a
 * correctly rounded division are part of the rule.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_limit.h"

#define AACG_LIMIT_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_LIMIT_THREADS) void aacg_pcm_limit_##NAME##_c##C(const aacg_limit_args A) { aacg_pipe::limit_body<T, C>(A, gridDim.x); }
AACG_LIMIT_BODIES(AACG_LIMIT_KERNEL)

/* false: not a launch these kernels serve (channels, element size, settings outside the limits, no stream) — nothing is enqueued */
bool aacg_limit_launch(const aacg_limit_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_limit_args) = nullptr;
#define AACG_LIMIT_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_limit_##NAME##_c##C;
    AACG_LIMIT_BODIES(AACG_LIMIT_PICK)
    if (!kernel || !A.n_streams || !A.n_frames || !aacg_limit_config_ok(A.ceiling, A.release)) return false;
    const uint32_t groups = (A.n_streams + AACG_LIMIT_WAVES - 1u) / AACG_LIMIT_WAVES;
    const uint32_t blocks = groups < AACG_LIMIT_MAX_BLOCKS ? groups : AACG_LIMIT_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_LIMIT_THREADS), 0, s, A);
    return true;
}
