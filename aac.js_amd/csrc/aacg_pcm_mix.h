/*
 * aacg_pcm_mix.h — a resident batch's packed PCM of C channels mixed down (or up) to O = 1 or 2 channels on the device
 * (aacg_pipeline_set_mix, include/aacgpu.h).  ONE launch per batch (aacg_pcm_mix_*, aacg_engine_mix.hip) on the lane's stream behind
 * aacg_pipeline_join, in front of whatever takes the PCM out: the copy down, the planar launch, or nothing (a caller's packed buffer).
 *
 * The rule (include/aacgpu.h states it for callers).  The transform leaves src[(f * 1024 + t) * C + c]; with the matrix M, O rows of
 * C floats, for every sample of the batch's n_frames frames and every o < O
 *     acc = M[o][0] * x[0];   acc = acc + M[o][c] * x[c]  for c = 1 .. C-1, in that order
 * every product rounded to float and every sum rounded to float — never a fused multiply-add (#pragma clang fp contract(off), as
 * epilogue() has it), every term computed whatever its coefficient — so that float32 arithmetic anywhere reproduces the bits.
 * f32: x[c] is the sample, dst[(f * 1024 + t) * O + o] = acc, no clamp.  int16: x[c] is the lane buffer's ALREADY ROUNDED int16
 * sample converted to float (exact), and dst is acc rounded to nearest even and saturated to [-32768, 32767]: dp_pcm16_pair(acc *
 * 2^-15, ...), whose scaling by a power of two is exact and whose one fused multiply-add is the rounding.
 *
 * Memory-bound, no LDS, no wave layout, no division.  An item is G = 16 / sizeof(ELEM) consecutive samples (4 of f32, 8 of int16): a
 * lane loads the item's C x G contiguous elements as C 16-byte vectors — read once: the non-temporal load —, computes G x O outputs
 * in registers (C, O and ELEM are compile-time constants: every index is one; the matrix arrives by value in the kernel's arguments,
 * wave-uniform) and stores them packed, G x O contiguous elements: O 16-byte vectors, plain stores — the copy down or the planar
 * kernel reads them next.  Alignment: item i's source begins at byte i * G * C * sizeof(ELEM) = 16 C i and its destination at byte
 * i * G * O * sizeof(ELEM) = 16 O i, so with 16-byte aligned bases every vector of either side lies at a multiple of 16 bytes, for
 * every C in 1..8, both O and both element sizes: no narrower access is needed anywhere.  The output keeps the source's frame order,
 * so items need no notion of frame or stream: grid-stride over n_frames * 1024 / G of them.  The host's part checks that the count
 * fits 31 bits (aacg_mix_items).
 *
 * Written against devport.h like aacg_pcm_planar.h, and executed lane by lane on the CPU by tests/emu/mix_emu.cpp.
 */
#ifndef AACG_PCM_MIX_H
#define AACG_PCM_MIX_H

#include <stddef.h>
#include <stdint.h>

#include "devport.h"

/* X(element type, its name in the kernel's name, channels in, channels out) */
#define AACG_MIX_BODIES_O(X, T, NAME, O) \
    X(T, NAME, 1, O) X(T, NAME, 2, O) X(T, NAME, 3, O) X(T, NAME, 4, O) X(T, NAME, 5, O) X(T, NAME, 6, O) X(T, NAME, 7, O) X(T, NAME, 8, O)
/* The thirty-two bodies: C, O and the element size are compile-time constants of a body, and the HOST picks the body — each is a kernel
 * entry of its own (aacg_pcm_mix_<name>_c<C>_o<O>, aacg_engine_mix.hip). */
#define AACG_MIX_BODIES(X) \
    AACG_MIX_BODIES_O(X, float, f32, 1) AACG_MIX_BODIES_O(X, float, f32, 2) AACG_MIX_BODIES_O(X, int16_t, i16, 1) AACG_MIX_BODIES_O(X, int16_t, i16, 2)

#define AACG_MIX_THREADS 256
#define AACG_MIX_MAX_BLOCKS 2048
#define AACG_MIX_MAX_IN 8
#define AACG_MIX_MAX_OUT 2

/* what one launch mixes */
typedef struct aacg_mix_args {
    const void* src;           /* the lane's packed PCM: [frame][1024][C] elements, 16-byte aligned                           */
    void*       dst;           /* [frame][1024][O] elements, 16-byte aligned                                                  */
    uint32_t n_frames;
    uint32_t channels;         /* 1..8   }                                                                                    */
    uint32_t out_channels;     /* 1 or 2 } which body the host launches (AACG_MIX_BODIES); a body does not read them          */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
    float m[AACG_MIX_MAX_OUT * AACG_MIX_MAX_IN];      /* M[o][c] at m[o * channels + c]: row-major, as the caller gave it     */
} aacg_mix_args;

/* items of a launch: n_frames x (1024 / G); 0 if that does not fit 31 bits (the kernel counts them in 32) */
static inline uint32_t aacg_mix_items(uint32_t n_frames, uint32_t elem)
{
    const uint64_t n = (uint64_t)n_frames * (1024u / (16u / elem));
    return n < (1ull << 31) ? (uint32_t)n : 0u;
}

namespace aacg_pipe {

DP_DEVICE float mix_bits_f32(int w) { float f; __builtin_memcpy(&f, &w, 4); return f; }
DP_DEVICE int mix_f32_bits(float f) { int w; __builtin_memcpy(&w, &f, 4); return w; }

/* one output channel of one sample: the rule's sum, in its order */
template <int C>
DP_DEVICE float mix_row(const float* m, const float (&x)[C])
{
#pragma clang fp contract(off)
    float acc = m[0] * x[0];
    #pragma unroll
    for (int c = 1; c < C; c++) acc = acc + m[c] * x[c];
    return acc;
}

/* Workgroup b of `blocks`: items b * AACG_MIX_THREADS + lane, then `blocks` workgroups on. */
template <typename ELEM, int C, int O>
DP_DEVICE void mix_body(const aacg_mix_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= AACG_MIX_MAX_IN && O >= 1 && O <= AACG_MIX_MAX_OUT, "f32 or int16 PCM, 1..8 channels to 1 or 2");
    constexpr uint32_t G = 16u / (uint32_t)sizeof(ELEM);         /* samples of an item */
    const uint32_t n_items = A.n_frames * (1024u / G);
    for (uint32_t i = (uint32_t)dp_block() * AACG_MIX_THREADS + (uint32_t)dp_tid(); i < n_items; i += blocks * AACG_MIX_THREADS) {
        /* the item's C x G elements: 4 C words, element (j, c) — sample j, channel c — at position j * C + c */
        const dpi4* in = (const dpi4*)A.src + (size_t)i * C;
        int w[4 * C];
        #pragma unroll
        for (int k = 0; k < C; k++) { const dpi4 v = dp_load_nt(in + k); w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
        float acc[G][O];
        #pragma unroll
        for (int j = 0; j < (int)G; j++) {
            float x[C];
            #pragma unroll
            for (int c = 0; c < C; c++) {
                const int e = j * C + c;
                if constexpr (sizeof(ELEM) == 4) x[c] = mix_bits_f32(w[e]);
                else x[c] = (float)(int16_t)(uint16_t)((uint32_t)w[e >> 1] >> (16 * (e & 1)));      /* exact */
            }
            #pragma unroll
            for (int o = 0; o < O; o++) acc[j][o] = mix_row<C>(A.m + o * C, x);
        }
        /* G x O outputs, sample by sample: 4 O words */
        int r[4 * O];
        if constexpr (sizeof(ELEM) == 4) {
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                #pragma unroll
                for (int o = 0; o < O; o++) r[j * O + o] = mix_f32_bits(acc[j][o]);
            }
        } else {
            #pragma unroll
            for (int k = 0; k < 4 * O; k++) {                     /* word k: output elements 2 k and 2 k + 1, element e = sample e / O, channel e % O */
                const int e0 = 2 * k, e1 = 2 * k + 1;
                r[k] = dp_pcm16_pair(acc[e0 / O][e0 % O] * 0.000030517578125f, acc[e1 / O][e1 % O] * 0.000030517578125f);
            }
        }
        dpi4* out = (dpi4*)A.dst + (size_t)i * O;
        #pragma unroll
        for (int k = 0; k < O; k++) { dpi4 v; v.x = r[4 * k]; v.y = r[4 * k + 1]; v.z = r[4 * k + 2]; v.w = r[4 * k + 3]; out[k] = v; }
    }
}

}  // namespace aacg_pipe

#endif
