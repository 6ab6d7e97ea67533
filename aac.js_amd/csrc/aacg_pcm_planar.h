/*
 * aacg_pcm_planar.h — a resident batch's PCM from the lane's packed buffer into a caller's planar tensor on the device
 * (AACG_PCM_PLANAR, aacg_pipeline_submit_device, include/aacgpu.h).  ONE launch per batch (aacg_pcm_planar_*, aacg_engine_planar.hip)
 * on the lane's stream behind aacg_pipeline_join, where the copy down sits for a host batch.
 *
 * The rule.  The transform leaves src[(frame_first[s] * 1024 + t) * C + c]: stream s's frames one behind the other, the channels of
 * a sample next to each other (what a host caller gets).  With T = stride_frames * 1024,
 *     dst[(s * C + c) * T + t] = t < frames[s] * 1024 ? src[((frame_first[s] * 1024) + t) * C + c] : 0
 * for every s < n_streams, c < C, t < T: every element of the n_streams x C x T block is written exactly once — the padding behind a
 * short stream too, so the caller need not clear the tensor — and nothing outside it.  frame_first and frames are the first two words
 * of the batch's per-stream table, which travels with the bytes in either plan mode (aacg_pipe_stream, 16 bytes a stream;
 * aacg_shape_stream, 48): the kernel reads it where aacg_pipe_map and the shaping kernel read it, with the record's size as a stride.
 *
 * Memory-bound, no LDS, no wave layout.  An item is 16 bytes per channel: G = 16 / sizeof(ELEM) consecutive samples of one stream
 * (4 of f32, 8 of int16).  A lane loads the item's C x G contiguous elements as C 16-byte vectors — read once and not again: the
 * non-temporal load —, sorts the words by channel in registers (C and ELEM are compile-time constants: every index is one) and stores
 * one 16-byte vector per channel, so a wave's store per channel is one contiguous kilobyte; plain stores, the consumer reads them next.
 * An item of the padding is C stores of zeros of the same width.  Alignment: a frame is 1024 samples and an item G of them, so with
 * 16-byte aligned bases every source vector lies at a multiple of 16 C bytes and every destination vector at a multiple of 16 bytes,
 * for every C in 1..8 and both element sizes: no narrower access is needed anywhere.
 * Grid-stride over the items, (stream, frame of the row, item of the frame) in that order, like carry_body over units: a frame has a
 * power of two of items, so only the split of the row index into stream and frame is a division.  The host's part checks that the item
 * count fits 31 bits (aacg_planar_items).
 *
 * Written against devport.h like aacg_pipe_map.h and aacg_shape_carry.h, and executed lane by lane on the CPU by tests/emu/planar_emu.cpp.
 */
#ifndef AACG_PCM_PLANAR_H
#define AACG_PCM_PLANAR_H

#include "aacg_pipe_map.h"

/* The sixteen bodies, X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of
 * a body, and the HOST picks the body — each is a kernel entry of its own (aacg_pcm_planar_<name>_c<C>, aacg_engine_planar.hip), so a
 * stereo launch has the stereo body's registers and code, not the eight-channel body's. */
#define AACG_PLANAR_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_PLANAR_THREADS 256
#define AACG_PLANAR_MAX_BLOCKS 2048

/* what one launch moves */
typedef struct aacg_planar_args {
    const void* src;           /* the lane's packed PCM: [frame][1024][C] elements                                            */
    void*       dst;           /* the caller's tensor: [n_streams][C][stride_frames * 1024] elements                          */
    const void* tab;           /* the batch's per-stream table on the device: records of tab_stride bytes, frame_first and
                                  frames their first two words                                                                */
    uint32_t tab_stride;
    uint32_t n_streams;
    uint32_t stride_frames;    /* frames per row, >= every stream's count                                                     */
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_PLANAR_BODIES); a body does not read them             */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_planar_args;

/* items of a launch: n_streams x stride_frames x (1024 / G); 0 if that does not fit 31 bits (the kernel counts them in 32) */
static inline uint32_t aacg_planar_items(uint32_t n_streams, uint32_t stride_frames, uint32_t elem)
{
    const uint64_t n = (uint64_t)n_streams * stride_frames * (1024u / (16u / elem));
    return n < (1ull << 31) ? (uint32_t)n : 0u;
}

namespace aacg_pipe {

/* Workgroup b of `blocks`: items b * AACG_PLANAR_THREADS + lane, then `blocks` workgroups on. */
template <typename ELEM, int C>
DP_DEVICE void planar_body(const aacg_planar_args& A, uint32_t blocks)
{
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    constexpr uint32_t G = 16u / (uint32_t)sizeof(ELEM);         /* samples of an item: 16 bytes a channel */
    constexpr uint32_t PER_FRAME = 1024u / G, SHIFT = sizeof(ELEM) == 4 ? 8u : 7u;
    static_assert(PER_FRAME == (1u << SHIFT), "items of a frame");
    const uint32_t n_items = A.n_streams * A.stride_frames * PER_FRAME;
    const size_t T = (size_t)A.stride_frames * 1024u;
    for (uint32_t i = (uint32_t)dp_block() * AACG_PLANAR_THREADS + (uint32_t)dp_tid(); i < n_items; i += blocks * AACG_PLANAR_THREADS) {
        const uint32_t row = i >> SHIFT, g = i & (PER_FRAME - 1u);
        const uint32_t s = row / A.stride_frames, f = row - s * A.stride_frames;
        const uint32_t* t = (const uint32_t*)((const char*)A.tab + (size_t)s * A.tab_stride);
        const uint32_t frame_first = t[0], frames = t[1];
        dpi4 out[C];
        if (f < frames) {
            /* the item's C x G elements: 4 C words, element (j, c) — sample j, channel c — at position j * C + c */
            const dpi4* in = (const dpi4*)((const ELEM*)A.src + ((size_t)(frame_first + f) * 1024u + (size_t)g * G) * C);
            int w[4 * C];
            #pragma unroll
            for (int k = 0; k < C; k++) { const dpi4 v = dp_load_nt(in + k); w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
            #pragma unroll
            for (int c = 0; c < C; c++) {
                int o[4];
                if (sizeof(ELEM) == 4) {
                    #pragma unroll
                    for (int j = 0; j < 4; j++) o[j] = w[j * C + c];
                } else {
                    #pragma unroll
                    for (int j = 0; j < 4; j++) {                     /* word j of the channel's vector: samples 2 j and 2 j + 1 */
                        const int e0 = 2 * j * C + c, e1 = (2 * j + 1) * C + c;
                        const uint32_t lo = ((uint32_t)w[e0 >> 1] >> (16 * (e0 & 1))) & 0xffffu, hi = ((uint32_t)w[e1 >> 1] >> (16 * (e1 & 1))) & 0xffffu;
                        o[j] = (int)(lo | (hi << 16));
                    }
                }
                out[c].x = o[0]; out[c].y = o[1]; out[c].z = o[2]; out[c].w = o[3];
            }
        } else {
            #pragma unroll
            for (int c = 0; c < C; c++) { out[c].x = 0; out[c].y = 0; out[c].z = 0; out[c].w = 0; }
        }
        ELEM* d = (ELEM*)A.dst + (size_t)s * C * T + (size_t)f * 1024u + (size_t)g * G;
        #pragma unroll
        for (int c = 0; c < C; c++) *(dpi4*)(d + (size_t)c * T) = out[c];
    }
}

}  // namespace aacg_pipe

#endif
