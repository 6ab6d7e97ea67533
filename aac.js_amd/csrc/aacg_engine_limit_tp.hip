/*
 * aacg_engine_limit_tp.hip — the limiter with a true-peak detector on a resident batch's PCM (aacg_pcm_limit_tp.h: limit_tp_detect_body,
 * limit_tp_walk_body): TWO launches per batch of a pipeline whose limiter has the detector (aacg_pipeline_set_limiter_true_peak,
 * include/aacgpu.h) on the lane's stream behind the mix, in the place of aacg_engine_limit.hip's one.  The detector: four waves per
 * workgroup, a workgroup per frame, one float per block of 64 into the lane's scratch.  The walk: four waves per workgroup, a wave per
 * stream, a lane per sample of a block; no LDS.
 *
 * Thirty-two kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_limit_tp_detect_f32_c1 .. aacg_pcm_limit_tp_detect_i16_c8
 * and aacg_pcm_limit_tp_f32_c1 .. aacg_pcm_limit_tp_i16_c8), switched on the host; each has its row in the Makefile's gate.  The unit is
 * built without any flush-to-zero or fast-math flag: subnormals and a correctly rounded division are part of the rule.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_limit_tp.h"

#define AACG_LIMIT_TP_KERNELS(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_LIMIT_TP_THREADS) void aacg_pcm_limit_tp_detect_##NAME##_c##C(const aacg_limit_tp_args A) { aacg_pipe::limit_tp_detect_body<T, C>(A, gridDim.x); } \
    extern "C" __global__ __launch_bounds__(AACG_LIMIT_THREADS) void aacg_pcm_limit_tp_##NAME##_c##C(const aacg_limit_tp_args A) { aacg_pipe::limit_tp_walk_body<T, C>(A, gridDim.x); }
AACG_LIMIT_BODIES(AACG_LIMIT_TP_KERNELS)

/* false: not a launch these kernels serve (channels, element size, settings or a table outside the limits, no stream) — nothing is enqueued */
bool aacg_limit_tp_launch(const aacg_limit_tp_args& A, hipStream_t s)
{
    void (*detect)(const aacg_limit_tp_args) = nullptr;
    void (*walk)(const aacg_limit_tp_args) = nullptr;
#define AACG_LIMIT_TP_PICK(T, NAME, C) if (A.lim.elem == sizeof(T) && A.lim.channels == C) { detect = aacg_pcm_limit_tp_detect_##NAME##_c##C; walk = aacg_pcm_limit_tp_##NAME##_c##C; }
    AACG_LIMIT_BODIES(AACG_LIMIT_TP_PICK)
    if (!detect || !A.lim.n_streams || !A.lim.n_frames || !aacg_limit_config_ok(A.lim.ceiling, A.lim.release) || aacg_truepeak_check(A.phases, A.taps)) return false;
    const uint32_t frames = A.lim.n_frames < AACG_LIMIT_TP_MAX_BLOCKS ? A.lim.n_frames : AACG_LIMIT_TP_MAX_BLOCKS;
    hipLaunchKernelGGL(detect, dim3(frames), dim3(AACG_LIMIT_TP_THREADS), 0, s, A);
    const uint32_t groups = (A.lim.n_streams + AACG_LIMIT_WAVES - 1u) / AACG_LIMIT_WAVES;
    const uint32_t blocks = groups < AACG_LIMIT_MAX_BLOCKS ? groups : AACG_LIMIT_MAX_BLOCKS;
    hipLaunchKernelGGL(walk, dim3(blocks), dim3(AACG_LIMIT_THREADS), 0, s, A);
    return true;
}
