/*
 * aacg_features.cpp — the feature stage's host-only part (include/aacgpu.h): what a stream's samples emit at a clock
 * (aacg_features_counts) and the usual tables, a Hann-windowed Fourier basis and a Slaney mel filterbank (aacg_features_design).  No
 * device, no pipeline; the limits are aacg_pcm_features.h's, which the kernels and aacg_pipeline_set_features share.
 */
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/aacgpu.h"
#define AACG_FEATURES_HOST_ONLY                           /* the limits and the records, not the kernel body */
#include "aacg_pcm_features.h"

namespace {

/* the Slaney mel scale: 200 / 3 Hz per mel below 1 kHz, steps of ln(6.4) / 27 above it */
const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp;
double logstep() { return std::log(6.4) / 27.0; }
double hz_to_mel(double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep() : f / f_sp; }
double mel_to_hz(double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep() * (m - min_log_mel)) : f_sp * m; }

}  // namespace

extern "C" {

int aacg_features_counts(uint32_t frame_length, uint32_t hop, uint32_t pad_left, uint64_t n0, uint64_t samples, uint64_t* n_frames)
{
    if (!n_frames || aacg_features_check(frame_length, hop, pad_left, 2u, 1u)) return AACG_ERR_INVALID_ARG;
    if (n0 + samples < n0) return AACG_ERR_INVALID_ARG;
    *n_frames = aacg_features_count(frame_length, hop, pad_left, n0 + samples) - aacg_features_count(frame_length, hop, pad_left, n0);
    return AACG_OK;
}

int aacg_features_design(uint32_t rate, uint32_t frame_length, uint32_t hop, uint32_t n_bins, uint32_t n_mels, double f_min, double f_max,
                         float* basis, size_t basis_capacity, float* fb, size_t fb_capacity)
{
    const uint32_t K = frame_length, B = n_bins;
    if (!rate || !basis || !fb || B > AACG_FEATURES_MAX_R / 2u || aacg_features_check(K, hop, 0u, 2u * B, n_mels)) return AACG_ERR_INVALID_ARG;
    if (f_max == 0.0) f_max = 0.5 * (double)rate;
    if (!(f_min >= 0.0) || !(f_max > f_min) || !(f_max <= 0.5 * (double)rate)) return AACG_ERR_INVALID_ARG;
    if (basis_capacity < (size_t)2u * B * K || fb_capacity < (size_t)n_mels * B) return AACG_ERR_INVALID_ARG;
    const double two_pi = 6.283185307179586476925286766559;
    /* the basis: the periodic Hann window on the bin's cosine and minus its sine; the angle from (b k) mod K, exactly reduced */
    for (uint32_t b = 0; b < B; b++)
        for (uint32_t k = 0; k < K; k++) {
            const double w = 0.5 - 0.5 * std::cos(two_pi * (double)k / (double)K);
            const double a = two_pi * (double)(((uint64_t)b * k) % K) / (double)K;
            basis[(size_t)(2u * b) * K + k] = (float)(w * std::cos(a));
            basis[(size_t)(2u * b + 1u) * K + k] = (float)(-(w * std::sin(a)));
        }
    /* the filterbank: n_mels + 2 edges equally spaced in mel, triangles between them over the bins' frequencies b rate / K, each
     * scaled by 2 / (its width in Hz) */
    std::vector<double> edge((size_t)n_mels + 2u);
    const double m_lo = hz_to_mel(f_min), m_hi = hz_to_mel(f_max);
    for (uint32_t i = 0; i < n_mels + 2u; i++) edge[i] = mel_to_hz(m_lo + (m_hi - m_lo) * (double)i / (double)(n_mels + 1u));
    for (uint32_t m = 0; m < n_mels; m++)
        for (uint32_t b = 0; b < B; b++) {
            const double f = (double)b * (double)rate / (double)K;
            const double lower = (f - edge[m]) / (edge[m + 1u] - edge[m]), upper = (edge[m + 2u] - f) / (edge[m + 2u] - edge[m + 1u]);
            const double tri = lower < upper ? lower : upper;
            fb[(size_t)m * B + b] = (float)((tri > 0.0 ? tri : 0.0) * (2.0 / (edge[m + 2u] - edge[m])));
        }
    return AACG_OK;
}

}  // extern "C"
