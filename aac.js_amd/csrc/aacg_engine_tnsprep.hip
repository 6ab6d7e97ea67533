/*
 * aacg_engine_tnsprep.hip — a batch's TNS records made on the device from the parser's outputs (aacg_tns_prep.h:
 * tns_records_body), with their transition matrices behind them (aacg_tns_matrices, aacg_engine_spectral.hip, on the same stream):
 * aacg_tns_records_from_parse, include/aacgpu.h.  A side kernel of one lane per record; plain vector stores.
 */
#include <hip/hip_runtime.h>

#include "aacg_tns_prep.h"

extern "C" __global__ __launch_bounds__(AACG_TNSPREP_THREADS)
void aacg_tns_records(const aacg_tnsprep_args A)
{
    aacg_tnsprep::tns_records_body(A, gridDim.x);
}

void aacg_tns_records_launch(const aacg_tnsprep_args& A, hipStream_t s)
{
    const uint32_t n = A.n_frames * A.parse_channels, want = (n + AACG_TNSPREP_THREADS - 1u) / AACG_TNSPREP_THREADS;
    const uint32_t blocks = want < 1024u ? want : 1024u;
    hipLaunchKernelGGL(aacg_tns_records, dim3(blocks), dim3(AACG_TNSPREP_THREADS), 0, s, A);
}
