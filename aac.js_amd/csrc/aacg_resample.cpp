/*
 * aacg_resample.cpp — the resampler's host-only part (include/aacgpu.h): what a stream's frames emit at a clock (aacg_resample_counts)
 * and the default polyphase table (aacg_resample_design).  No device, no pipeline; the limits are aacg_pcm_resample.h's, which the
 * kernels and aacg_pipeline_set_resample share.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/aacgpu.h"
#define AACG_RESAMPLE_HOST_ONLY                           /* the limits and the records, not the kernel body */
#include "aacg_pcm_resample.h"

namespace {

uint32_t gcd_u32(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

/* the modified Bessel function of the first kind, order zero: its power series, every term positive, to double precision */
double bessel_i0(double x)
{
    const double q = x * x * 0.25;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-17) break;
    }
    return sum;
}

}  // namespace

extern "C" {

int aacg_resample_counts(uint32_t L, uint32_t M, uint32_t n0, uint32_t frames, uint32_t* per_frame, uint32_t* n0_after)
{
    if (L < 1 || M < 1 || L > AACG_RESAMPLE_MAX_LM || M > AACG_RESAMPLE_MAX_LM) return AACG_ERR_INVALID_ARG;
    uint32_t n = n0 % M;                                  /* only the clock modulo M counts: ceil((q M + n) L / M) = q L + ceil(n L / M) */
    for (uint32_t f = 0; f < frames; f++) {
        if (per_frame) per_frame[f] = aacg_resample_ceil(n + 1024u, L, M) - aacg_resample_ceil(n, L, M);
        n = (n + 1024u) % M;
    }
    if (n0_after) *n0_after = n;
    return AACG_OK;
}

int aacg_resample_design(uint32_t in_rate, uint32_t out_rate, uint32_t taps, double rolloff, double beta, uint32_t* L_out, uint32_t* M_out, float* table, size_t capacity)
{
    if (!in_rate || !out_rate || !L_out || !M_out) return AACG_ERR_INVALID_ARG;
    if (rolloff == 0.0) rolloff = 0.95;
    if (beta == 0.0) beta = 9.0;
    if (!(rolloff > 0.0 && rolloff <= 1.0) || !(beta > 0.0 && beta <= 30.0)) return AACG_ERR_INVALID_ARG;
    const uint32_t g = gcd_u32(in_rate, out_rate), L = out_rate / g, M = in_rate / g;
    if (aacg_resample_check(L, M, taps)) return AACG_ERR_INVALID_ARG;
    *L_out = L; *M_out = M;
    const size_t n = (size_t)L * taps;
    if (!table) return capacity ? AACG_ERR_INVALID_ARG : AACG_OK;      /* (no table and no capacity: the ratio alone) */
    if (capacity < n) return AACG_ERR_INVALID_ARG;
    /* the prototype g[0 .. L T - 1], centred at (L T - 1) / 2: sinc at the cutoff under a Kaiser window.  Its scale is immaterial: every
     * phase row is divided by its sum */
    const double pi = 3.14159265358979323846, centre = ((double)n - 1.0) * 0.5, fc = 0.5 * rolloff / (double)(L > M ? L : M), i0b = bessel_i0(beta);
    std::vector<double> proto(n);
    for (size_t k = 0; k < n; k++) {
        const double d = (double)k - centre, a = 2.0 * fc * d, r = d / centre;
        const double sinc = a == 0.0 ? 1.0 : std::sin(pi * a) / (pi * a);
        const double w = 1.0 - r * r;
        proto[k] = sinc * bessel_i0(beta * std::sqrt(w > 0.0 ? w : 0.0)) / i0b;
    }
    for (uint32_t p = 0; p < L; p++) {
        double sum = 0.0;
        for (uint32_t t = 0; t < taps; t++) sum += proto[p + (size_t)t * L];
        for (uint32_t t = 0; t < taps; t++) table[(size_t)p * taps + t] = (float)(proto[p + (size_t)t * L] / sum);
    }
    return AACG_OK;
}

}  // extern "C"
