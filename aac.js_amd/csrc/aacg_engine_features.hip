/*
 * aacg_engine_features.hip — a resident batch's one-channel PCM framed and transformed to (log-)mel features on the device
 * (aacg_pcm_features.h: features_body): ONE launch per batch of a pipeline with the stage (aacg_pipeline_set_features, include/aacgpu.h)
 * on the lane's stream, the last stage of the way out.  One workgroup per sixteen feature frames of a stream: the samples in LDS, rows x
 * frames on v_mfma_f32_16x16x4_f32, power and mel chains behind it; packed or planar out, ragged per stream.
 *
 * Two kernel entries, one per input element (aacg_pcm_features_f32, aacg_pcm_features_i16), switched on the host; each has its row
 * in the Makefile's gate, with its LDS.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_features.h"

extern "C" __global__ __launch_bounds__(AACG_FEATURES_THREADS) void aacg_pcm_features_f32(const aacg_features_args A) { aacg_pipe::features_body<float>(A, gridDim.x); }
extern "C" __global__ __launch_bounds__(AACG_FEATURES_THREADS) void aacg_pcm_features_i16(const aacg_features_args A) { aacg_pipe::features_body<int16_t>(A, gridDim.x); }

/* false: not a launch these kernels serve (the element size, tables outside the limits, no item) — nothing is enqueued */
bool aacg_features_launch(const aacg_features_args& A, hipStream_t s)
{
    if ((A.elem != 4u && A.elem != 2u) || !A.n_items || !A.n_streams || aacg_features_check(A.K, A.H, 0u, A.R, A.n_mels)) return false;
    const uint32_t blocks = A.n_items < AACG_FEATURES_MAX_BLOCKS ? A.n_items : AACG_FEATURES_MAX_BLOCKS;
    hipLaunchKernelGGL(A.elem == 4u ? aacg_pcm_features_f32 : aacg_pcm_features_i16, dim3(blocks), dim3(AACG_FEATURES_THREADS), 0, s, A);
    return true;
}
