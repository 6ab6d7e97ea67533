/*
 * aacg_engine_truepeak.hip — the true peak of a resident batch's transform PCM (aacg_pcm_truepeak.h: truepeak_body): ONE launch per batch
 * of a pipeline with a true-peak stage (aacg_pipeline_set_true_peak, include/aacgpu.h) on the lane's stream behind aacg_pipeline_join,
 * beside the meter's launch.  One workgroup of four waves per input frame; the frame through LDS, a lane a sample with all its phases and
 * channels, one float per hop and channel out — stored where a hop lies inside a frame, by a vector atomic maximum where it does not.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_truepeak_f32_c1 .. aacg_pcm_truepeak_i16_c8), switched on
 * the host; each has its row in the Makefile's gate, with its LDS.  The unit is built without any flush-to-zero flag: subnormals are
 * part of the rule.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_truepeak.h"

#define AACG_TRUEPEAK_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_TRUEPEAK_THREADS) void aacg_pcm_truepeak_##NAME##_c##C(const aacg_truepeak_args A) { aacg_pipe::truepeak_body<T, C>(A, gridDim.x); }
AACG_TRUEPEAK_BODIES(AACG_TRUEPEAK_KERNEL)

/* false: not a launch these kernels serve (channels, element size, a table or a hop outside the limits, no stream, too many frames) — nothing is enqueued */
bool aacg_truepeak_launch(const aacg_truepeak_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_truepeak_args) = nullptr;
#define AACG_TRUEPEAK_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_truepeak_##NAME##_c##C;
    AACG_TRUEPEAK_BODIES(AACG_TRUEPEAK_PICK)
    if (!kernel || !A.n_streams || !A.n_frames || A.n_frames > AACG_TRUEPEAK_MAX_FRAMES || A.hop < 1u || A.hop > AACG_LOUDNESS_MAX_HOP) return false;
    if (aacg_truepeak_check(A.phases, A.taps)) return false;
    const uint32_t blocks = A.n_frames < AACG_TRUEPEAK_MAX_BLOCKS ? A.n_frames : AACG_TRUEPEAK_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_TRUEPEAK_THREADS), 0, s, A);
    return true;
}
