/*
 * aacg_engine_trim.hip — a resident batch's packed PCM cut to each stream's window on the device (aacg_pcm_trim.h: trim_body): ONE launch
 * per batch of a pipeline with a trim (aacg_pipeline_set_trim, include/aacgpu.h) on the lane's stream, the last PCM stage of the way
 * out.  One workgroup per item, a tile of kept samples of one stream: the source's aligned vectors into LDS as they lie, whole aligned
 * vectors out, element stores at a segment's ends; packed or planar out, ragged per stream.  No device state.
 *
 * Sixteen kernel entries, one per body (f32 / int16 x 1..8 channels: aacg_pcm_trim_f32_c1 .. aacg_pcm_trim_i16_c8), switched on the
 * host; each has its row in the Makefile's gate, with its LDS.
 */
#include <hip/hip_runtime.h>

#include "aacg_pcm_trim.h"

#define AACG_TRIM_KERNEL(T, NAME, C) \
    extern "C" __global__ __launch_bounds__(AACG_TRIM_THREADS) void aacg_pcm_trim_##NAME##_c##C(const aacg_trim_args A) { aacg_pipe::trim_body<T, C>(A, gridDim.x); }
AACG_TRIM_BODIES(AACG_TRIM_KERNEL)

/* false: not a launch these kernels serve (channels, element size, no stream, no item, a planar row that is no multiple of 1024) —
 * nothing is enqueued */
bool aacg_trim_launch(const aacg_trim_args& A, hipStream_t s)
{
    void (*kernel)(const aacg_trim_args) = nullptr;
#define AACG_TRIM_PICK(T, NAME, C) if (A.elem == sizeof(T) && A.channels == C) kernel = aacg_pcm_trim_##NAME##_c##C;
    AACG_TRIM_BODIES(AACG_TRIM_PICK)
    if (!kernel || !A.n_items || !A.n_streams || (A.row & 1023u)) return false;
    const uint32_t blocks = A.n_items < AACG_TRIM_MAX_BLOCKS ? A.n_items : AACG_TRIM_MAX_BLOCKS;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AACG_TRIM_THREADS), 0, s, A);
    return true;
}
