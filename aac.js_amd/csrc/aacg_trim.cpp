/*
 * aacg_trim.cpp — the trim's host-only part (include/aacgpu.h): the share of a window's kept range that each of consecutive pieces owns
 * (aacg_trim_counts) and the window at the stage's input for a window given in the stream's own samples, with the route's latencies
 * compensated (aacg_trim_design).  No device, no pipeline, exact integers; the rule and the limits are aacg_pcm_trim.h's, which the
 * kernels and aacg_pipeline_set_trim share.
 */
#include <cstdint>

#include "../../include/aacgpu.h"
#define AACG_TRIM_HOST_ONLY                               /* the limits, the records and the rule, not the kernel body */
#include "aacg_pcm_trim.h"

extern "C" {

int aacg_trim_counts(uint64_t position, uint64_t skip, uint64_t keep, const uint32_t* n_in, uint32_t n, uint32_t* first_of, uint32_t* kept_of)
{
    if ((n && !n_in) || !first_of || !kept_of || aacg_trim_check(skip, keep)) return AACG_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; i++) {
        if (position + n_in[i] < position) return AACG_ERR_INVALID_ARG;      /* (a position at the end of 64 bits) */
        aacg_trim_span(position, skip, keep, n_in[i], &first_of[i], &kept_of[i]);
        position += n_in[i];
    }
    return AACG_OK;
}

int aacg_trim_design(uint64_t skip_in, uint64_t keep_in, int limiter, uint32_t L, uint32_t M, uint32_t taps, uint64_t* skip, uint64_t* keep,
                     uint64_t* residual_num, uint64_t* residual_den)
{
    if (!skip || !keep || aacg_trim_check(skip_in, keep_in)) return AACG_ERR_INVALID_ARG;
    if (L < 1 || M < 1 || L > 1024 || M > 1024 || taps > 64) return AACG_ERR_INVALID_ARG;
    /* A(t) = 2 L t + 128 L limiter + L taps - 1: twice the place, in upsampled samples, where input sample t comes out — behind the
     * limiter's 64 samples and a linear-phase table's (L taps - 1) / 2.  taps 0: no resampler pass, and no filter term.  Below 2^53 */
    const uint64_t lat = (limiter ? 128ull * L : 0ull) + (taps ? (uint64_t)L * taps - 1u : 0ull), den = 2ull * M;
    const uint64_t a0 = 2ull * L * skip_in + lat, s = (a0 + den - 1u) / den;
    uint64_t k = AACG_TRIM_KEEP_ALL;
    if (keep_in != AACG_TRIM_KEEP_ALL) k = (2ull * L * (skip_in + keep_in) + lat + den - 1u) / den - s;
    if (aacg_trim_check(s, k)) return AACG_ERR_INVALID_ARG;
    *skip = s; *keep = k;
    if (residual_num) *residual_num = s * den - a0;
    if (residual_den) *residual_den = den;
    return AACG_OK;
}

}  // extern "C"
