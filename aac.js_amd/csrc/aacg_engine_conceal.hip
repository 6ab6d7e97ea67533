/*
 * aacg_engine_conceal.hip — refused frames concealed on the device (aacg_units_conceal.h: conceal_body): ONE launch per batch behind
 * aacg_units_refresh on the same stream and in front of aacg_units_carry_shape substitutes, for a frame the parser or the refresh
 * refused, the records of its stream's last good frame with a fade — unit record, spectrum blocks, band words — and leaves each
 * stream's last good frame in the slot's state for the next batch (aacg_plan_conceal_refused, include/aacgpu.h).  One wave per
 * (frame, channel block); 16-byte vector loads and stores.
 */
#include <hip/hip_runtime.h>

#include "aacg_units_conceal.h"

extern "C" __global__ __launch_bounds__(AACG_CONCEAL_THREADS)
void aacg_units_conceal(const aacg_conceal_args A)
{
    aacg_pipe::conceal_body(A, gridDim.x);
}

void aacg_conceal_launch(const aacg_conceal_args& A, hipStream_t s)
{
    const uint32_t jobs = A.n_streams * A.longest * A.Cp, want = (jobs + AACG_CONCEAL_WAVES - 1u) / AACG_CONCEAL_WAVES;
    const uint32_t blocks = want < AACG_CONCEAL_MAX_BLOCKS ? want : AACG_CONCEAL_MAX_BLOCKS;
    if (!blocks) return;
    hipLaunchKernelGGL(aacg_units_conceal, dim3(blocks), dim3(AACG_CONCEAL_THREADS), 0, s, A);
}
