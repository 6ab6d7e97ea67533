/*
 * aacg_pcm_resample.h — a resident batch's packed PCM resampled by a rational factor L / M on the device (aacg_pipeline_set_resample,
 * include/aacgpu.h).  ONE launch per batch (aacg_pcm_resample_*, aacg_engine_resample.hip) on the lane's stream behind aacg_pipeline_join
 * and behind the mix if there is one, where the planar launch or the copy down reads for a pipeline without a resampler.
 *
 * The rule (include/aacgpu.h states it for callers).  With the polyphase table h[L][T], output sample m = 0, 1, 2, ... of a stream's
 * channel is, with i = floor(m M / L) and p = (m M) mod L,
 *     acc = h[p][0] * x[i];   acc = acc + h[p][t] * x[i - t]   for t = 1 .. T-1, in that order
 * every product and every sum a float32 operation of its own, never fused (#pragma clang fp contract(off), as mix_row has it), every
 * term computed whatever its coefficient, x[j] = 0 for j < 0.  x is the stream's PCM as the pipeline would have delivered it; int16:
 * the already rounded sample as a float (exact), and the output is acc rounded to nearest even and saturated, dp_pcm16_pair(acc * 2^-15).
 *
 * State.  A stream slot carries its clock N (input samples consumed since its reset) and, per channel, its last T - 1 input samples.
 * The counts depend only on N mod M — ceil((q M + n0) L / M) = q L + ceil(n0 L / M) — so the HOST keeps the clock modulo M and passes
 * n0 < M per stream: with n = n0 + 1024 k the clock at frame k of a stream's frames in this batch, nn = n mod M and q = n / M, the
 * frame owns the outputs m with n <= i(m) < n + 1024, which are q L + ceil(nn L / M) .. q L + ceil((nn + 1024) L / M) - 1.  Everything
 * but q L is below 2^21 and q L cancels wherever an index into the frame or into the stream's output is formed: 32-bit arithmetic.
 * The history is float, [slot][parity][T - 1][C], double-buffered: a stream's first frame of a launch reads parity `parity` (or takes
 * zeros if the stream is fresh: after a reset nothing is read, so nothing need be cleared) while its last frame writes parity ^ 1.
 * The host orders consecutive launches (an event behind each, awaited by the next on its own stream) and flips the parity.
 *
 * Work.  One workgroup per input frame of the batch (grid-stride over frames).  It stages the frame's 1024 x C elements into LDS as
 * floats — 16-byte non-temporal loads, int16 converted on the way in — and in front of them the T - 1 samples that precede the frame:
 * from the previous frame in the lane's buffer, or for a stream's first frame from the slot's history.  LDS holds sample j of the frame
 * at float (T + j) * C + c, the preceding samples at (1 .. T-1) * C: the frame begins 16-byte aligned (T is a multiple of 4).  A lane
 * then takes an output of the frame at a time with all its C channels: one 32-bit division by L per output gives i and p, the phase
 * row h[p] arrives as T / 4 16-byte loads, the C accumulators run side by side.  A stream's last frame writes the new history from
 * LDS.  LDS: (64 + 1024) x C x 4 bytes, static — 4352 bytes a channel, 34816 for eight.
 *
 * The table comes THROUGH THE CACHE, not from LDS: it is at most 64 KiB, read-only and shared by every workgroup of every launch, so it
 * stays in the L2 and mostly in a CU's L1, and a lane reads its row as consecutive 16-byte vectors whatever the row stride — no
 * padding question.  In LDS it would have cost each workgroup up to 64 KiB of staging for the 1024 x C samples it filters.  Decided by
 * reading; neither this, nor the workgroup size, nor the LDS layout's bank behaviour has been tuned (adjacent lanes read x at a
 * stride of about C M / L floats).
 *
 * Writes.  Packed: [stream of the batch][n_out[s]][C], tight, stream s at sample out_first[s]; a lane stores its C elements.
 * Planar (row != 0): [stream][C][row], and the padding behind n_out[s] is written as zeros, the stream's frames each a share of it:
 * every element of the n_streams x C x row block is written exactly once, and nothing outside it.
 *
 * Written against devport.h like aacg_pcm_mix.h, and executed lane by lane on the CPU by tests/emu/resample_emu.cpp.
 */
#ifndef AACG_PCM_RESAMPLE_H
#define AACG_PCM_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifndef AACG_RESAMPLE_HOST_ONLY                          /* (aacg_resample.cpp takes the limits and the records alone) */
#include "devport.h"
#endif

/* X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of a body, and the HOST
 * picks the body — each is a kernel entry of its own (aacg_pcm_resample_<name>_c<C>, aacg_engine_resample.hip). */
#define AACG_RESAMPLE_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_RESAMPLE_THREADS 256
#define AACG_RESAMPLE_MAX_BLOCKS 4096
#define AACG_RESAMPLE_MAX_TAPS 64
#define AACG_RESAMPLE_MAX_LM 1024
#define AACG_RESAMPLE_MAX_TABLE 16384      /* L x T floats: 64 KiB */
#define AACG_RESAMPLE_LDS_BYTES(C) ((AACG_RESAMPLE_MAX_TAPS + 1024) * (C) * 4)

/* one stream of a launch; travels up in the lane's staging block behind the batch's per-stream table */
typedef struct aacg_resample_stream {
    uint32_t frame_first;      /* the stream's first frame in the lane's packed PCM                                            */
    uint32_t frames;           /* >= 1                                                                                         */
    uint32_t out_first;        /* packed layout: the stream's first output sample (the sum of n_out of the streams before it)  */
    uint32_t n_out;            /* samples per channel this launch emits for the stream                                         */
    uint32_t n0;               /* the slot's clock modulo M at the stream's first frame                                        */
    uint32_t slot;
    uint32_t parity;           /* the history buffer the stream's first frame reads; its last frame writes parity ^ 1          */
    uint32_t fresh;            /* nothing consumed since the slot's reset: the history is zeros and is not read                */
} aacg_resample_stream;

/* what one launch resamples */
typedef struct aacg_resample_args {
    const void* src;           /* the lane's packed PCM: [frame][1024][C] elements, 16-byte aligned                            */
    void*       dst;           /* packed [sum n_out][C] or planar [n_streams][C][row] elements                                 */
    const aacg_resample_stream* rec;      /* n_streams records, frame_first ascending from 0, no gaps                          */
    const float* table;        /* h[L][T], 16-byte aligned                                                                     */
    float*      hist;          /* [slot][2][T - 1][C] floats                                                                   */
    uint32_t n_streams, n_frames;
    uint32_t L, M, taps;
    uint32_t row;              /* 0: packed; else planar, elements per row (stride_frames x 1024 >= every n_out)               */
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_RESAMPLE_BODIES); a body does not read them      */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_resample_args;

/* 0 if (L, M, T) is a resampler the kernels serve, else which limit it breaks (aacg_resample_why) */
static inline int aacg_resample_check(uint32_t L, uint32_t M, uint32_t T)
{
    if (T < 4 || T > AACG_RESAMPLE_MAX_TAPS || (T & 3u)) return 1;
    if (L < 1 || M < 1 || L > AACG_RESAMPLE_MAX_LM || M > AACG_RESAMPLE_MAX_LM) return 2;
    if (L * T > AACG_RESAMPLE_MAX_TABLE) return 3;
    if (L > 8u * M || M > 8u * L) return 4;
    return 0;
}
static inline const char* aacg_resample_why(int code)
{
    return code == 1 ? "taps is not a multiple of 4 in 4..64" : code == 2 ? "L and M are not both in 1..1024" :
           code == 3 ? "L x taps is more than 16384 coefficients" : code == 4 ? "L / M is not within 1/8 .. 8" : "";
}
/* ceil(n L / M) for n < 2^21 and L, M <= 1024 */
#define AACG_RESAMPLE_CEIL(n, L, M) (((n) * (L) + (M) - 1u) / (M))      /* (a macro: host and device code share it) */
static inline uint32_t aacg_resample_ceil(uint32_t n, uint32_t L, uint32_t M) { return AACG_RESAMPLE_CEIL(n, L, M); }

#ifndef AACG_RESAMPLE_HOST_ONLY
namespace aacg_pipe {

/* Workgroup b of `blocks`: frames b, b + blocks, ... of the batch. */
template <typename ELEM, int C>
DP_DEVICE void resample_body(const aacg_resample_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    float* const x = (float*)dp_lds_fixed<AACG_RESAMPLE_LDS_BYTES(C)>();
    const uint32_t T = A.taps, L = A.L, M = A.M, tid = (uint32_t)dp_tid(), H = (T - 1u) * C;
    for (uint32_t f = (uint32_t)dp_block(); f < A.n_frames; f += blocks) {
        /* the frame's stream: the last record that begins at or before it */
        uint32_t s = 0;
        for (uint32_t hi = A.n_streams; hi - s > 1u;) { const uint32_t mid = (s + hi) >> 1; if (A.rec[mid].frame_first <= f) s = mid; else hi = mid; }
        const aacg_resample_stream R = A.rec[s];
        const uint32_t k = f - R.frame_first;
        const ELEM* const frame = (const ELEM*)A.src + (size_t)f * 1024u * C;
        /* the frame into LDS: 16 bytes a lane and turn */
        if constexpr (sizeof(ELEM) == 4) {
            for (uint32_t v = tid; v < 256u * C; v += AACG_RESAMPLE_THREADS) ((dpi4*)(x + T * C))[v] = dp_load_nt((const dpi4*)frame + v);
        } else {
            for (uint32_t v = tid; v < 128u * C; v += AACG_RESAMPLE_THREADS) {
                const dpi4 w = dp_load_nt((const dpi4*)frame + v);
                const int q[4] = {w.x, w.y, w.z, w.w};
                dpf4 a, b;
                a.x = (float)(int16_t)(uint16_t)(uint32_t)q[0]; a.y = (float)(int16_t)(uint16_t)((uint32_t)q[0] >> 16);      /* exact */
                a.z = (float)(int16_t)(uint16_t)(uint32_t)q[1]; a.w = (float)(int16_t)(uint16_t)((uint32_t)q[1] >> 16);
                b.x = (float)(int16_t)(uint16_t)(uint32_t)q[2]; b.y = (float)(int16_t)(uint16_t)((uint32_t)q[2] >> 16);
                b.z = (float)(int16_t)(uint16_t)(uint32_t)q[3]; b.w = (float)(int16_t)(uint16_t)((uint32_t)q[3] >> 16);
                ((dpf4*)(x + T * C))[2u * v] = a; ((dpf4*)(x + T * C))[2u * v + 1u] = b;
            }
        }
        /* the T - 1 samples in front of it: the previous frame's last, the slot's history, or — a fresh stream — zeros */
        const float* const old = A.hist + ((size_t)R.slot * 2u + R.parity) * H;
        for (uint32_t e = tid; e < H; e += AACG_RESAMPLE_THREADS)
            x[C + e] = k ? (float)(frame - H)[e] : R.fresh ? 0.0f : old[e];
        dp_block_sync();
        /* the frame's outputs (the header's arithmetic): m_lo = q L + c1, of which there are c2 - c1; in the stream's output the first
         * is at q L + c1 - ceil(n0 L / M); i(m_lo + j) - n = base + (r + j M) / L and p = (r + j M) mod L */
        const uint32_t n = R.n0 + 1024u * k, q = n / M, nn = n - q * M;
        const uint32_t c1 = AACG_RESAMPLE_CEIL(nn, L, M), n_f = AACG_RESAMPLE_CEIL(nn + 1024u, L, M) - c1;
        const uint32_t pos0 = q * L + c1 - AACG_RESAMPLE_CEIL(R.n0, L, M);
        const uint32_t a0 = c1 * M / L, r = c1 * M - a0 * L, base = a0 - nn;
        for (uint32_t j = tid; j < n_f; j += AACG_RESAMPLE_THREADS) {
            const uint32_t u = r + j * M, qd = u / L, p = u - qd * L;
            const float* const xs = x + (size_t)(T + base + qd) * C;      /* x[i], channel 0; x[i - t] lies t * C floats in front */
            const dpf4* const hrow = (const dpf4*)(A.table + (size_t)p * T);
            float acc[C] = {};                                            /* (every one is set by its first product below) */
            for (uint32_t t4 = 0; t4 < T; t4 += 4u) {
                const dpf4 hv = hrow[t4 >> 2];
                const float h[4] = {hv.x, hv.y, hv.z, hv.w};
                #pragma unroll
                for (int d = 0; d < 4; d++) {
                    const float* const xt = xs - (size_t)(t4 + (uint32_t)d) * C;
                    #pragma unroll
                    for (int c = 0; c < C; c++) {
                        const float prod = h[d] * xt[c];
                        acc[c] = (t4 == 0u && d == 0) ? prod : acc[c] + prod;
                    }
                }
            }
            const size_t at = (size_t)pos0 + j;                           /* the output's place in the stream's output */
            if (A.row) {
                ELEM* const d = (ELEM*)A.dst + (size_t)s * C * A.row + at;
                #pragma unroll
                for (int c = 0; c < C; c++) {
                    if constexpr (sizeof(ELEM) == 4) d[(size_t)c * A.row] = acc[c];
                    else d[(size_t)c * A.row] = (ELEM)(int16_t)(uint16_t)((uint32_t)dp_pcm16_pair(acc[c] * 0.000030517578125f, 0.0f) & 0xffffu);
                }
            } else {
                ELEM* const d = (ELEM*)A.dst + ((size_t)R.out_first + at) * C;
                if constexpr (sizeof(ELEM) == 4) {
                    #pragma unroll
                    for (int c = 0; c < C; c++) d[c] = acc[c];
                } else if constexpr (C % 2 == 0) {                        /* an even count of int16: whole words, 4-byte aligned */
                    #pragma unroll
                    for (int c = 0; c < C; c += 2) ((int*)d)[c >> 1] = dp_pcm16_pair(acc[c] * 0.000030517578125f, acc[c + 1] * 0.000030517578125f);
                } else {
                    #pragma unroll
                    for (int c = 0; c < C; c++) d[c] = (ELEM)(int16_t)(uint16_t)((uint32_t)dp_pcm16_pair(acc[c] * 0.000030517578125f, 0.0f) & 0xffffu);
                }
            }
        }
        /* planar: this frame's share of the zeros behind the stream's n_out samples, in every channel's row */
        if (A.row) {
            const uint32_t pad = A.row - R.n_out, share = (pad + R.frames - 1u) / R.frames;
            const uint32_t lo = k * share < pad ? k * share : pad, hi = pad - lo < share ? pad : lo + share;
            #pragma unroll
            for (int c = 0; c < C; c++) {
                ELEM* const d = (ELEM*)A.dst + ((size_t)s * C + (size_t)c) * A.row + R.n_out;
                for (uint32_t e = lo + tid; e < hi; e += AACG_RESAMPLE_THREADS) d[e] = (ELEM)0;
            }
        }
        /* the stream's last frame: its last T - 1 samples are the slot's new history */
        if (k + 1u == R.frames) {
            float* const next = A.hist + ((size_t)R.slot * 2u + (R.parity ^ 1u)) * H;
            for (uint32_t e = tid; e < H; e += AACG_RESAMPLE_THREADS) next[e] = x[(size_t)1025u * C + e];
        }
        dp_block_sync();                                                  /* the next frame of this workgroup overwrites the LDS */
    }
}

}  // namespace aacg_pipe
#endif

#endif
