/*
 * aacg_loudness.cpp — the loudness tap's host-only part (include/aacgpu.h): what a stream's samples emit at a clock
 * (aacg_loudness_counts), BS.1770's K-weighting re-derived for any rate (aacg_loudness_design) and the gated integration of the hop
 * records into LUFS (aacg_loudness_integrate).  No device, no pipeline; everything in double.
 */
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/aacgpu.h"
#define AACG_LOUDNESS_HOST_ONLY                           /* the limits and the records, not the kernel body */
#include "aacg_pcm_loudness.h"

extern "C" {

int aacg_loudness_counts(uint32_t hop, uint64_t n0, uint64_t samples, uint64_t* n)
{
    if (!n || hop < 1u || hop > AACG_LOUDNESS_MAX_HOP) return AACG_ERR_INVALID_ARG;
    *n = aacg_loudness_emits(hop, n0, samples);
    return AACG_OK;
}

int aacg_loudness_design(uint32_t rate, float coeffs[2][5])
{
    if (!rate || !coeffs) return AACG_ERR_INVALID_ARG;
    const double pi = 3.141592653589793238462643383279;
    {   /* the shelf */
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        coeffs[0][0] = (float)((Vh + Vb * K / Q + K * K) / a0);
        coeffs[0][1] = (float)(2.0 * (K * K - Vh) / a0);
        coeffs[0][2] = (float)((Vh - Vb * K / Q + K * K) / a0);
        coeffs[0][3] = (float)(2.0 * (K * K - 1.0) / a0);
        coeffs[0][4] = (float)((1.0 - K / Q + K * K) / a0);
    }
    {   /* the high-pass */
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)rate), a0 = 1.0 + K / Q + K * K;
        coeffs[1][0] = 1.0f; coeffs[1][1] = -2.0f; coeffs[1][2] = 1.0f;
        coeffs[1][3] = (float)(2.0 * (K * K - 1.0) / a0);
        coeffs[1][4] = (float)((1.0 - K / Q + K * K) / a0);
    }
    for (int i = 0; i < 2; i++) for (int k = 0; k < 5; k++) if (!std::isfinite(coeffs[i][k])) return AACG_ERR_INVALID_ARG;
    return AACG_OK;
}

int aacg_loudness_integrate(const float* records, size_t n_hops, uint32_t channels, uint32_t hop, const double* weights,
                            double* integrated_lufs, double* momentary_lufs)
{
    if ((!records && n_hops) || !integrated_lufs || channels < 1u || channels > 8u || hop < 1u || hop > AACG_LOUDNESS_MAX_HOP) return AACG_ERR_INVALID_ARG;
    const double ninf = -std::numeric_limits<double>::infinity();
    *integrated_lufs = ninf;
    if (n_hops < 4) return AACG_OK;
    /* blocks of four consecutive hops, one hop apart */
    const size_t n_blocks = n_hops - 3;
    std::vector<double> z(n_blocks), l(n_blocks);
    for (size_t b = 0; b < n_blocks; b++) {
        double sum = 0.0;
        for (uint32_t c = 0; c < channels; c++) {
            double e = 0.0;
            for (size_t h = b; h < b + 4; h++) e += (double)records[(h * channels + c) * 2u];
            sum += (weights ? weights[c] : 1.0) * e / (4.0 * (double)hop);
        }
        z[b] = sum;
        l[b] = sum > 0.0 ? -0.691 + 10.0 * std::log10(sum) : ninf;
        if (momentary_lufs) momentary_lufs[b] = l[b];
    }
    /* the absolute gate, then the relative one at the kept blocks' mean minus 10 LU */
    double acc = 0.0; size_t kept = 0;
    for (size_t b = 0; b < n_blocks; b++) if (l[b] > -70.0) { acc += z[b]; kept++; }
    if (!kept) return AACG_OK;
    const double gate = -0.691 + 10.0 * std::log10(acc / (double)kept) - 10.0;
    acc = 0.0; kept = 0;
    for (size_t b = 0; b < n_blocks; b++) if (l[b] > -70.0 && l[b] > gate) { acc += z[b]; kept++; }
    if (kept) *integrated_lufs = -0.691 + 10.0 * std::log10(acc / (double)kept);
    return AACG_OK;
}

}  // extern "C"
