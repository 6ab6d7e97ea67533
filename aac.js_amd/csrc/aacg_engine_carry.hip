/*
 * aacg_engine_carry.hip — each channel's window shape carried from frame to frame on the device (aacg_shape_carry.h: carry_body): ONE
 * launch per batch behind aacg_units_refresh on the same stream sets window_shape_prev of a plan set's unit records from the frame
 * before — or, for a stream's first frame of the batch, from the engine's per-channel state, which the stream's last frame leaves
 * for the next batch (aacg_plan_carry_window_shape, include/aacgpu.h).  One lane per unit; plain vector loads and stores.
 */
#include <hip/hip_runtime.h>

#include "aacg_shape_carry.h"

extern "C" __global__ __launch_bounds__(AACG_CARRY_THREADS)
void aacg_units_carry_shape(const aacg_carry_args A)
{
    aacg_pipe::carry_body(A, gridDim.x);
}

void aacg_carry_launch(const aacg_carry_args& A, hipStream_t s)
{
    const uint32_t want = (A.n_units + AACG_CARRY_THREADS - 1u) / AACG_CARRY_THREADS, blocks = want < AACG_CARRY_MAX_BLOCKS ? want : AACG_CARRY_MAX_BLOCKS;
    if (!blocks) return;
    hipLaunchKernelGGL(aacg_units_carry_shape, dim3(blocks), dim3(AACG_CARRY_THREADS), 0, s, A);
}
