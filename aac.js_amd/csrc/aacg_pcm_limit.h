/*
 * aacg_pcm_limit.h — a per-stream gain and a channel-linked look-ahead limiter on a resident batch's PCM (aacg_pipeline_set_limiter,
 * aacg_pipeline_set_gain, include/aacgpu.h): a STAGE of the way out (aacg_pipe_exit.h: AACG_EXIT_LIMIT), behind the mix and in front of
 * the resampler and the feature stage.  ONE launch per batch (aacg_pcm_limit_*, aacg_engine_limit.hip) on the lane's stream; it reads
 * the last lane buffer written and writes the next, sample for sample, delayed by one block.
 *
 * The rule (include/aacgpu.h states it for callers).  Blocks of B = 64 samples x C channels; per slot a held block xh, the node gain a0
 * at its start and its target th.  For every arriving block xk, with the pipeline's ceiling c and release r and the slot's gain G:
 *     p  = max |xk|  (fmaxf from +0)          tk = (G p > c) ? c / p : G          u = a0 + (r (G - a0))
 *     a1 = fminf(fminf(th, tk), u)            d  = a1 - a0                        out[i][ch] = (a0 + (d (i / 64))) xh[i][ch]
 *     xh = xk;  a0 = a1;  th = tk
 * float32, every operation rounded on its own, nothing fused (#pragma clang fp contract(off) as loudness_body has it), subnormals kept,
 * the division correctly rounded (the compiler's default for HIP; the unit is built without any fast-math or flush-to-zero flag).
 * int16 PCM: x is the sample times 2^-15 (exact), out goes through dp_pcm16_pair, the mix's rounding and saturation.
 *
 * Work.  A stream's blocks are serial in a0 and th alone: a handful of scalar operations per block.  One WAVE owns a stream for the whole
 * batch, lane i sample i of every block: a lane's C elements of a block are one vector (limit_vec: as wide as C elements are aligned,
 * 16 bytes at the most), the block's peak is the wave-wide maximum of the lanes' own (dp_wave_max), the recurrence is computed alike in
 * every lane, and the held block stays in registers — no LDS.  Blocks go in GROUPS of eight (half a frame): the group's eight vectors are
 * loaded back to back, the NEXT group's are issued before the current one is walked, the eight peaks of a group are reduced side by side
 * (their exchanges are independent: 6 steps of 8, not 8 chains of 6), then the eight blocks are walked and stored.  A workgroup is four
 * waves, four streams, which share nothing; the grid strides over the batch's streams.
 * Decided by reading, not measured: the group of eight (sixteen would hold 2 x 128 registers for eight float channels), the butterfly
 * through ds_bpermute in the place of DPP row operations, a wave per stream (a batch of few long streams leaves most of the chip idle:
 * its peaks and its outputs could be split over waves and only the recurrence kept serial), plain loads and stores.
 *
 * State: [slot][parity]{a0, th, two unused floats, xh[64][C]} floats — double-buffered like the resampler's history: a stream reads
 * parity `parity` (a fresh slot reads nothing: a block of zeros, a0 = th = G) and writes parity ^ 1; the host orders consecutive
 * launches with an event and flips the parity.  The slot's gain travels in the record.
 *
 * Written against devport.h like aacg_pcm_loudness.h, and executed lane by lane on the CPU by tests/emu/limiter_emu.cpp.
 */
#ifndef AACG_PCM_LIMIT_H
#define AACG_PCM_LIMIT_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/aacgpu.h"
#ifndef AACG_LIMIT_HOST_ONLY                             /* (aacg_limiter.cpp and aacg_pipeline.hip take the limits and the records alone) */
#include "devport.h"
#endif

/* X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of a body, and the HOST
 * picks the body — each is a kernel entry of its own (aacg_pcm_limit_<name>_c<C>, aacg_engine_limit.hip). */
#define AACG_LIMIT_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_LIMIT_WAVES 4                               /* streams of a workgroup */
#define AACG_LIMIT_THREADS (64 * AACG_LIMIT_WAVES)
#define AACG_LIMIT_GROUP 8                               /* blocks loaded and reduced together: 1024 / 64 / 8 = 2 groups a frame */
#define AACG_LIMIT_MAX_BLOCKS 4096
#define AACG_LIMIT_MAX_GAIN 1024.0f
#define AACG_LIMIT_STATE_HEAD 4                          /* floats in front of a state buffer's held block: a0, th and two unused */
#define AACG_LIMIT_STATE(C) (AACG_LIMIT_STATE_HEAD + AACG_LIMIT_BLOCK * (C))      /* floats of one state buffer */

/* one stream of a launch; travels up in the lane's staging block behind the meter's records */
typedef struct aacg_limit_stream {
    uint32_t frame_first;      /* the stream's first frame in the packed PCM, source and destination alike                     */
    uint32_t frames;           /* >= 1                                                                                         */
    uint32_t slot;
    uint32_t parity;           /* the state buffer the stream reads; it writes parity ^ 1                                      */
    uint32_t fresh;            /* nothing consumed since the slot's reset: a block of zeros, a0 = th = gain, nothing is read   */
    float    gain;             /* the slot's G as it stood when the batch was enqueued                                         */
    uint32_t unused[2];
} aacg_limit_stream;

/* what one launch limits */
typedef struct aacg_limit_args {
    const void* src;           /* packed PCM: [frame][1024][C] elements, 16-byte aligned                                       */
    void*       dst;           /* the same shape, another buffer                                                               */
    const aacg_limit_stream* rec;         /* n_streams records, frame_first ascending from 0, no gaps                          */
    float*      state;         /* [slot][2][AACG_LIMIT_STATE(C)] floats                                                        */
    uint32_t n_streams, n_frames;
    float    ceiling, release;
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_LIMIT_BODIES); a body does not read them         */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_limit_args;

/* the settings' limits (aacg_pipeline_set_limiter, aacg_limiter_design; written so that a NaN fails) */
static inline int aacg_limit_config_ok(float ceiling, float release)
{
    return ceiling > 0.0f && ceiling <= 3.402823466e+38f && release > 0.0f && release <= 1.0f;
}
static inline int aacg_limit_gain_ok(float gain) { return gain >= 0.0f && gain <= AACG_LIMIT_MAX_GAIN; }

#ifndef AACG_LIMIT_HOST_ONLY
namespace aacg_pipe {

/* a lane's C elements of a block, one memory access as wide as their alignment allows */
constexpr size_t limit_align(size_t bytes) { return bytes % 16u == 0 ? 16u : bytes % 8u == 0 ? 8u : bytes % 4u == 0 ? 4u : 2u; }
template <typename T, int C> struct alignas(limit_align(sizeof(T) * C)) limit_vec { T v[C]; };

/* Wave w of workgroup b of `blocks`: streams b 4 + w, then b 4 + w + blocks 4 ... */
template <typename ELEM, int C>
DP_DEVICE void limit_body(const aacg_limit_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    typedef limit_vec<ELEM, C> V;
    typedef limit_vec<float, C> VF;
    constexpr uint32_t NB = AACG_LIMIT_GROUP, B = AACG_LIMIT_BLOCK, SF = AACG_LIMIT_STATE(C);
    const uint32_t lane = (uint32_t)dp_lane();
    const float w = (float)lane * 0.015625f, c = A.ceiling, r = A.release;
    for (uint32_t s = (uint32_t)dp_block() * AACG_LIMIT_WAVES + (uint32_t)dp_wave(); s < A.n_streams; s += blocks * AACG_LIMIT_WAVES) {
        const aacg_limit_stream R = A.rec[s];
        const float G = R.gain;
        float a0 = G, th = G, xh[C];
        #pragma unroll
        for (int ch = 0; ch < C; ch++) xh[ch] = 0.0f;
        if (!R.fresh) {                                                   /* a fresh slot's state is the rule's and nothing is read */
            const float* const old = A.state + ((size_t)R.slot * 2u + R.parity) * SF;
            a0 = old[0]; th = old[1];
            const VF h = *((const VF*)(old + AACG_LIMIT_STATE_HEAD) + lane);
            #pragma unroll
            for (int ch = 0; ch < C; ch++) xh[ch] = h.v[ch];
        }
        /* this lane's sample of the stream's block j: src[j B], and where the block that leaves in its place goes: dst[j B] */
        const V* const src = (const V*)A.src + (size_t)R.frame_first * 1024u + lane;
        V* const dst = (V*)A.dst + (size_t)R.frame_first * 1024u + lane;
        const uint32_t n_groups = R.frames * (1024u / B / NB);
        V cur[NB], nxt[NB];
        #pragma unroll
        for (uint32_t b = 0; b < NB; b++) cur[b] = nxt[b] = src[b * B];
        for (uint32_t g = 0; g < n_groups; g++) {
            if (g + 1u < n_groups) {                                      /* in flight while this group is reduced and walked */
                #pragma unroll
                for (uint32_t b = 0; b < NB; b++) nxt[b] = src[((size_t)(g + 1u) * NB + b) * B];
            }
            float x[NB][C], pk[NB];
            #pragma unroll
            for (uint32_t b = 0; b < NB; b++) {
                pk[b] = 0.0f;
                #pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    if constexpr (sizeof(ELEM) == 4) x[b][ch] = cur[b].v[ch];
                    else x[b][ch] = (float)cur[b].v[ch] * 0.000030517578125f;      /* exact */
                    pk[b] = __builtin_fmaxf(pk[b], __builtin_fabsf(x[b][ch]));      /* (a NaN sample is ignored) */
                }
            }
            dp_wave_max(pk);
            #pragma unroll
            for (uint32_t b = 0; b < NB; b++) {
                const float p = pk[b];
                const float tk = G * p > c ? c / p : G;
                const float u = a0 + (r * (G - a0));
                const float a1 = __builtin_fminf(__builtin_fminf(th, tk), u);
                const float d = a1 - a0;
                const float k = a0 + (d * w);
                V o;
                if constexpr (sizeof(ELEM) == 4) {
                    #pragma unroll
                    for (int ch = 0; ch < C; ch++) o.v[ch] = k * xh[ch];
                } else {
                    #pragma unroll
                    for (int ch = 0; ch < C; ch += 2) {
                        const int q = dp_pcm16_pair(k * xh[ch], ch + 1 < C ? k * xh[ch + 1 < C ? ch + 1 : ch] : 0.0f);
                        o.v[ch] = (int16_t)(uint16_t)((uint32_t)q & 0xffffu);
                        if (ch + 1 < C) o.v[ch + 1 < C ? ch + 1 : ch] = (int16_t)(uint16_t)((uint32_t)q >> 16);
                    }
                }
                dst[((size_t)g * NB + b) * B] = o;
                #pragma unroll
                for (int ch = 0; ch < C; ch++) xh[ch] = x[b][ch];
                a0 = a1; th = tk;
            }
            #pragma unroll
            for (uint32_t b = 0; b < NB; b++) cur[b] = nxt[b];
        }
        float* const next = A.state + ((size_t)R.slot * 2u + (R.parity ^ 1u)) * SF;
        if (lane == 0u) { next[0] = a0; next[1] = th; }
        VF h;
        #pragma unroll
        for (int ch = 0; ch < C; ch++) h.v[ch] = xh[ch];
        *((VF*)(next + AACG_LIMIT_STATE_HEAD) + lane) = h;
    }
}

}  // namespace aacg_pipe
#endif

#endif
