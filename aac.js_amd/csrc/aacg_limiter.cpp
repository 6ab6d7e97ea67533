/*
 * aacg_limiter.cpp — the limiter's host-only part (include/aacgpu.h): a ceiling in dB and a release time at a rate into the two
 * settings of aacg_pipeline_set_limiter (aacg_limiter_design), everything in double; and the trim's window behind a limiter whose delay
 * is given in samples (aacg_trim_design_delay), exact integers.  No device, no pipeline.
 */
#include <cmath>
#include <cstdint>

#include "../../include/aacgpu.h"
#define AACG_LIMIT_HOST_ONLY                              /* the limits, not the kernel body */
#include "aacg_pcm_limit.h"
#define AACG_TRIM_HOST_ONLY                               /* the window's limits (aacg_trim_check) */
#include "aacg_pcm_trim.h"

extern "C" {

int aacg_limiter_design(uint32_t rate, double ceiling_db, double release_ms, aacg_limiter_config* cfg)
{
    if (!rate || !cfg) return AACG_ERR_INVALID_ARG;
    const double c = std::pow(10.0, ceiling_db / 20.0);
    const double r = 1.0 - std::exp(-(double)AACG_LIMIT_BLOCK / ((double)rate * release_ms / 1000.0));
    if (!(c > 0.0 && c <= 3.402823466e+38) || !(r > 0.0 && r <= 1.0)) return AACG_ERR_INVALID_ARG;      /* (a NaN fails both) */
    const float ceiling = (float)c, release = (float)r;
    if (!aacg_limit_config_ok(ceiling, release)) return AACG_ERR_INVALID_ARG;                          /* (a value that rounds to 0) */
    cfg->ceiling = ceiling; cfg->release = release;
    return AACG_OK;
}

/* aacg_trim_design (aacg_trim.cpp) with the limiter's delay in samples — 64, or 64 + taps / 2 with the true-peak detector
 * (aacg_pipeline_limiter_delay) — in the place of its 64 x limiter: A(t) = 2 L t + 2 L delay + L taps - 1, below 2^53 */
int aacg_trim_design_delay(uint64_t skip_in, uint64_t keep_in, uint32_t delay, uint32_t L, uint32_t M, uint32_t taps, uint64_t* skip, uint64_t* keep,
                           uint64_t* residual_num, uint64_t* residual_den)
{
    if (!skip || !keep || aacg_trim_check(skip_in, keep_in)) return AACG_ERR_INVALID_ARG;
    if (L < 1 || M < 1 || L > 1024 || M > 1024 || taps > 64) return AACG_ERR_INVALID_ARG;
    const uint64_t lat = 2ull * L * delay + (taps ? (uint64_t)L * taps - 1u : 0ull), den = 2ull * M;
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
