/*
 * aacg_engine_shape.hip — a resident batch's plan shaped on the device (aacg_plan_shape.h: shape_body): ONE launch per batch on the
 * lane's stream writes the refresh map, the unit records' planner part, the rendezvous cut of the run table and its link records
 * from the batch's per-stream table, in the place of aacg_pipe_map and of the host planner's build and upload
 * (aacg_plan_shape_launch, include/aacgpu.h).  A workgroup of one wave per stream; plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "aacg_plan_shape.h"

extern "C" __global__ __launch_bounds__(AACG_SHAPE_THREADS)
void aacg_plan_shape(const aacg_shape_args A)
{
    aacg_pipe::shape_body(A, gridDim.x);
}

void aacg_shape_launch(const aacg_shape_args& A, hipStream_t s)
{
    const uint32_t blocks = A.n_streams < 256u ? A.n_streams : 256u;
    hipLaunchKernelGGL(aacg_plan_shape, dim3(blocks), dim3(AACG_SHAPE_THREADS), 0, s, A);
}
