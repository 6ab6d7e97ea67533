/*
 * aacg_truepeak.cpp — the true-peak stage's host-only part (include/aacgpu.h): the project's default oversampling table
 * (aacg_true_peak_design), which is the resampler's default table for a rate of 1 into a rate of `phases`.  No device, no pipeline.
 */
#include <cstddef>
#include <cstdint>

#include "../../include/aacgpu.h"
#define AACG_LOUDNESS_HOST_ONLY
#define AACG_TRUEPEAK_HOST_ONLY                           /* the limits, not the kernel body */
#include "aacg_pcm_truepeak.h"

extern "C" {

int aacg_true_peak_design(uint32_t phases, uint32_t taps, double rolloff, double beta, float* table, size_t capacity)
{
    if (aacg_truepeak_check(phases, taps)) return AACG_ERR_INVALID_ARG;
    uint32_t L = 0, M = 0;
    return aacg_resample_design(1u, phases, taps, rolloff, beta, &L, &M, table, capacity);      /* (L = phases, M = 1; its defaults, its refusals) */
}

}  // extern "C"
