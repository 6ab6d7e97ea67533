/*
 * aacg_limiter.cpp — the limiter's host-only part (include/aacgpu.h): a ceiling in dB and a release time at a rate into the two
 * settings of aacg_pipeline_set_limiter (aacg_limiter_design).  No device, no pipeline; everything in double.
 */
#include <cmath>
#include <cstdint>

#include "../../include/aacgpu.h"
#define AACG_LIMIT_HOST_ONLY                              /* the limits, not the kernel body */
#include "aacg_pcm_limit.h"

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

}  // extern "C"
