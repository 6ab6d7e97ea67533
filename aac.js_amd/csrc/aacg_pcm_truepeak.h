/*
 * aacg_pcm_truepeak.h — the TRUE PEAK of a resident batch's transform PCM (aacg_pipeline_set_true_peak, include/aacgpu.h): the largest
 * magnitude of the signal oversampled by a polyphase FIR, one float per hop and channel, beside the meter's records.  ONE launch per batch
 * (aacg_pcm_truepeak_*, aacg_engine_truepeak.hip) on the lane's stream behind aacg_pipeline_join and beside the meter's launch; it reads
 * the buffer the transform wrote, as the meter does — the PCM's way out (aacg_pipe_exit.h) does not know it.
 *
 * The rule (include/aacgpu.h states it for callers).  With the polyphase table h[L][T], for input index i and phase p of a channel
 *     acc = h[p][0] * x[i];   acc = acc + h[p][t] * x[i - t]   for t = 1 .. T-1, in that order
 * every product and every sum a float32 operation of its own, never fused (#pragma clang fp contract(off), as resample_body has it),
 * every term computed whatever its coefficient, subnormals kept, x[j] = 0 for j < 0: aacg_pcm_resample.h's rule with M = 1.  x is the
 * meter's input; int16: the sample times 2^-15 (exact).  tp of hop k is the largest |acc| over i in [k hop, (k + 1) hop) and all L
 * phases, a NaN if any of them is one.
 *
 * The maximum is taken on the BITS of |acc| as unsigned integers: for floats that are no NaN that is the order of their values, and
 * every NaN lies above +inf, so a NaN wins wherever one takes part and nothing has to look for it.  A maximum does not depend on order:
 * no result here depends on how the work is split or on which workgroup arrives first.
 *
 * Work.  One workgroup per input frame of the batch (grid-stride over frames), four waves.  It stages the frame's 1024 x C elements
 * into LDS as floats — 16-byte non-temporal loads, int16 converted on the way in — and in front of them the T - 1 samples that precede
 * the frame: from the previous frame in the transform's buffer, or for a stream's first frame from the slot's history (resample_body's
 * layout: sample j of the frame at float (T + j) C + c).  A lane then takes an input sample at a time with all its C channels: four phase
 * rows at once (row min(p, L - 1): a row computed twice changes no maximum), two taps of each row as one 8-byte LDS read at an address
 * that is the same in every lane (a broadcast), 4 C accumulators side by side, each sample read from LDS once per four phases.  The
 * sample's maximum over the phases goes to LDS as bits, y[j][c].
 * The table lies in LDS, 2 KiB at most, copied once per workgroup — NOT through the cache as the resampler's: its table is up to 64 KiB
 * and a lane reads its own row; here every lane reads the same coefficients, the compiler makes scalar loads of that, and sixteen scalar
 * registers of coefficients beside the body's other uniform values overflowed the scalar file (a spill, which the gate refuses).
 * Then the reduction.  Hop boundaries cut the frame into PIECES: with P = n0 + 1024 k the frame's clock modulo nothing (n0 = N mod hop
 * at the stream's first frame), hop h of the stream's batch covers the frame's samples [max(h hop, P), min((h + 1) hop, P + 1024)) - P.
 * A wave takes a piece at a time: its lanes stride over the piece's samples, the wave's maximum is dp_wave_max (on the values as floats
 * with a NaN's place taken by a flag, which that primitive asks for), and the wave's first lane delivers the C channels:
 *   - a piece that is a whole hop is stored, plainly: dst[out_first + h][c];
 *   - a piece of a hop that straddles frames goes to the same place by a vector atomic unsigned maximum (dp_g_atomic_max_u32);
 *   - a piece of the hop that does not end in this batch (h >= n_out) goes by the same atomic to the slot's partial of the OTHER parity.
 * The stream's first frame also delivers the partial the slot carried, to hop 0's place, and then clears it where it lay.
 * What must be zero before the atomics arrive: the batch's records — the host clears them on the lane's stream in front of the launch —
 * and the partial of the parity that is written.  That one is cleared by the launch BEFORE: a batch reads parity `parity` and writes
 * parity ^ 1, the slot's next batch does the opposite, launches are ordered one behind the other by an event, and the state is zeros
 * when the stage is set.  So the partial a batch has read and cleared is the one the next batch finds empty, fresh slot or not (a fresh
 * slot reads nothing and clears all the same).
 *
 * Why atomics, and not a {head, tail} scratch per frame with a combining pass: the pass would be a second launch or a last-workgroup-
 * done counter, which is an atomic too and a fence besides; the maximum of non-negative floats on their bits is exact and commutes, so
 * the atomic gives the same bits with less machinery.  At most two pieces of a frame need one (the hops that cross its ends).
 *
 * State: [slot][parity]{hist[T - 1][C] floats, partial[C] bits}, T x C words, double-buffered as the resampler's history.  The clock is the
 * meter's, on the host, and so are the records: this kernel reads the meter's aacg_loudness_stream records (frame_first, frames,
 * out_first, n_out, n0, slot, parity, fresh), whose parity and fresh flag move exactly as this state's would.
 * Output: packed [stream s][n_out[s]][C] floats, stream s at record out_first[s].
 * LDS: (64 + 1024) x C floats of samples and 1024 x C words of maxima, 8448 bytes a channel, and 2048 for the table, static.
 * Not tuned: the four phases at a time, the workgroup size and the wave per piece (a hop of a few samples makes hundreds of pieces of a
 * frame, each a wave-wide reduction) were decided by reading.
 *
 * Written against devport.h like aacg_pcm_resample.h, and executed lane by lane on the CPU by tests/emu/truepeak_emu.cpp.
 */
#ifndef AACG_PCM_TRUEPEAK_H
#define AACG_PCM_TRUEPEAK_H

#include <stddef.h>
#include <stdint.h>

#include "aacg_pcm_loudness.h"                           /* the meter's records (and, unless AACG_LOUDNESS_HOST_ONLY, devport.h) */
#ifndef AACG_TRUEPEAK_HOST_ONLY                          /* (aacg_pipeline.hip takes the limits and the records alone) */
#include "devport.h"
#endif

/* X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of a body, and the HOST
 * picks the body — each is a kernel entry of its own (aacg_pcm_truepeak_<name>_c<C>, aacg_engine_truepeak.hip). */
#define AACG_TRUEPEAK_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_TRUEPEAK_THREADS 256
#define AACG_TRUEPEAK_MAX_BLOCKS 4096
#define AACG_TRUEPEAK_MAX_TAPS 64
#define AACG_TRUEPEAK_MAX_PHASES 8
#define AACG_TRUEPEAK_MAX_FRAMES (1u << 21)               /* frames of a launch: n0 + 1024 frames stays below 2^32 */
#define AACG_TRUEPEAK_LDS_BYTES(C) ((AACG_TRUEPEAK_MAX_TAPS + 1024 + 1024) * (C) * 4 + AACG_TRUEPEAK_MAX_PHASES * AACG_TRUEPEAK_MAX_TAPS * 4)
#define AACG_TRUEPEAK_STATE(T, C) ((T) * (C))             /* words of a slot's state of one parity: (T - 1) C of history, C of partial */

/* what one launch measures */
typedef struct aacg_truepeak_args {
    const void* src;           /* the transform's packed PCM: [frame][1024][C] elements, 16-byte aligned                       */
    uint32_t*   dst;           /* [sum n_out][C] floats as bits, ZERO before the launch                                        */
    const aacg_loudness_stream* rec;      /* the meter's n_streams records, frame_first ascending from 0, no gaps              */
    const float* table;        /* h[L][T], 16-byte aligned                                                                     */
    float*      state;         /* [slot][2][T x C] words                                                                       */
    uint32_t n_streams, n_frames, hop;
    uint32_t phases, taps;     /* L in 1..8, T a multiple of 4 in 4..64                                                        */
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_TRUEPEAK_BODIES); a body does not read them      */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_truepeak_args;

/* 0 if (L, T) is a table the kernels serve, else which limit it breaks (aacg_truepeak_why) */
static inline int aacg_truepeak_check(uint32_t L, uint32_t T)
{
    if (L < 1u || L > AACG_TRUEPEAK_MAX_PHASES) return 1;
    if (T < 4u || T > AACG_TRUEPEAK_MAX_TAPS || (T & 3u)) return 2;
    return 0;
}
static inline const char* aacg_truepeak_why(int code) { return code == 1 ? "phases is not in 1..8" : code == 2 ? "taps is not a multiple of 4 in 4..64" : ""; }

#ifndef AACG_TRUEPEAK_HOST_ONLY
namespace aacg_pipe {

DP_DEVICE uint32_t truepeak_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
DP_DEVICE float truepeak_float(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
DP_DEVICE uint32_t truepeak_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

/* Workgroup b of `blocks`: frames b, b + blocks, ... of the batch. */
template <typename ELEM, int C>
DP_DEVICE void truepeak_body(const aacg_truepeak_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    float* const x = (float*)dp_lds_fixed<AACG_TRUEPEAK_LDS_BYTES(C)>();
    uint32_t* const y = (uint32_t*)(x + (size_t)(AACG_TRUEPEAK_MAX_TAPS + 1024) * C);
    float* const ht = x + (size_t)(AACG_TRUEPEAK_MAX_TAPS + 2048) * C;      /* the table, h[p][t] at p T + t */
    const uint32_t T = A.taps, L = A.phases, hop = A.hop, tid = (uint32_t)dp_tid(), lane = (uint32_t)dp_lane(), wave = (uint32_t)dp_wave();
    const uint32_t H = (T - 1u) * C, SZ = AACG_TRUEPEAK_STATE(T, C);
    constexpr float SCALE = sizeof(ELEM) == 2 ? 0.000030517578125f : 1.0f;      /* int16: x 2^-15, exact */
    for (uint32_t e = tid; e < L * T; e += AACG_TRUEPEAK_THREADS) ht[e] = A.table[e];      /* (the frame loop's first barrier stands behind this) */
    for (uint32_t f = (uint32_t)dp_block(); f < A.n_frames; f += blocks) {
        /* the frame's stream: the last record that begins at or before it */
        uint32_t s = 0;
        for (uint32_t hi = A.n_streams; hi - s > 1u;) { const uint32_t mid = (s + hi) >> 1; if (A.rec[mid].frame_first <= f) s = mid; else hi = mid; }
        const aacg_loudness_stream R = A.rec[s];
        const uint32_t k = f - R.frame_first;
        const ELEM* const frame = (const ELEM*)A.src + (size_t)f * 1024u * C;
        float* const old = A.state + ((size_t)R.slot * 2u + R.parity) * SZ;
        float* const next = A.state + ((size_t)R.slot * 2u + (R.parity ^ 1u)) * SZ;
        /* the frame into LDS: 16 bytes a lane and turn */
        if constexpr (sizeof(ELEM) == 4) {
            for (uint32_t v = tid; v < 256u * C; v += AACG_TRUEPEAK_THREADS) ((dpi4*)(x + T * C))[v] = dp_load_nt((const dpi4*)frame + v);
        } else {
            for (uint32_t v = tid; v < 128u * C; v += AACG_TRUEPEAK_THREADS) {
                const dpi4 w = dp_load_nt((const dpi4*)frame + v);
                const int q[4] = {w.x, w.y, w.z, w.w};
                dpf4 a, b;
                a.x = (float)(int16_t)(uint16_t)(uint32_t)q[0] * SCALE; a.y = (float)(int16_t)(uint16_t)((uint32_t)q[0] >> 16) * SCALE;      /* exact */
                a.z = (float)(int16_t)(uint16_t)(uint32_t)q[1] * SCALE; a.w = (float)(int16_t)(uint16_t)((uint32_t)q[1] >> 16) * SCALE;
                b.x = (float)(int16_t)(uint16_t)(uint32_t)q[2] * SCALE; b.y = (float)(int16_t)(uint16_t)((uint32_t)q[2] >> 16) * SCALE;
                b.z = (float)(int16_t)(uint16_t)(uint32_t)q[3] * SCALE; b.w = (float)(int16_t)(uint16_t)((uint32_t)q[3] >> 16) * SCALE;
                ((dpf4*)(x + T * C))[2u * v] = a; ((dpf4*)(x + T * C))[2u * v + 1u] = b;
            }
        }
        /* the T - 1 samples in front of it: the previous frame's last, the slot's history, or — a fresh stream — zeros */
        for (uint32_t e = tid; e < H; e += AACG_TRUEPEAK_THREADS)
            x[C + e] = k ? (float)(frame - H)[e] * SCALE : R.fresh ? 0.0f : old[e];
        dp_block_sync();
        /* a sample a lane and turn: the largest |acc| of its L phases, per channel, as bits */
        for (uint32_t j = tid; j < 1024u; j += AACG_TRUEPEAK_THREADS) {
            const float* const xs = x + (size_t)(T + j) * C;             /* x[i], channel 0; x[i - t] lies t * C floats in front */
            uint32_t m[C];
            #pragma unroll
            for (int c = 0; c < C; c++) m[c] = 0u;
            for (uint32_t p0 = 0; p0 < L; p0 += 4u) {
                uint32_t row[4];                                          /* (floats from the table's start: at most 8 x 64) */
                #pragma unroll
                for (uint32_t pp = 0; pp < 4u; pp++) row[pp] = (p0 + pp < L ? p0 + pp : L - 1u) * T;
                float acc[4][C] = {};                                     /* (every one is set by its first product below) */
                #pragma clang loop unroll(disable)
                for (uint32_t t2 = 0; t2 < T; t2 += 2u) {                 /* two taps of four rows: eight coefficients, the same address in every lane */
                    float h[4][2];
                    #pragma unroll
                    for (int pp = 0; pp < 4; pp++) { const dpf2 hv = *(const dpf2*)(ht + row[pp] + t2); h[pp][0] = hv.x; h[pp][1] = hv.y; }
                    #pragma unroll
                    for (int d = 0; d < 2; d++) {
                        const float* const xt = xs - (size_t)(t2 + (uint32_t)d) * C;
                        #pragma unroll
                        for (int c = 0; c < C; c++) {
                            const float xv = xt[c];
                            #pragma unroll
                            for (int pp = 0; pp < 4; pp++) {
                                const float prod = h[pp][d] * xv;
                                acc[pp][c] = (t2 == 0u && d == 0) ? prod : acc[pp][c] + prod;
                            }
                        }
                    }
                }
                #pragma unroll
                for (int pp = 0; pp < 4; pp++) {
                    #pragma unroll
                    for (int c = 0; c < C; c++) m[c] = truepeak_umax(m[c], truepeak_bits(acc[pp][c]) & 0x7fffffffu);
                }
            }
            #pragma unroll
            for (int c = 0; c < C; c++) y[j * C + (uint32_t)c] = m[c];
        }
        /* the stream's last frame: its last T - 1 samples are the slot's new history */
        if (k + 1u == R.frames)
            for (uint32_t e = tid; e < H; e += AACG_TRUEPEAK_THREADS) next[e] = x[(size_t)1025u * C + e];
        dp_block_sync();
        /* the frame's pieces, a wave a piece: hop h of the stream's batch where it meets the frame's samples P .. P + 1023 */
        const uint32_t P = R.n0 + 1024u * k, h_hi = (P + 1023u) / hop;
        for (uint32_t h = P / hop + wave; h <= h_hi; h += AACG_TRUEPEAK_THREADS / 64u) {
            const uint32_t lo = h * hop, end = lo + hop;
            const uint32_t a = lo > P ? lo - P : 0u, b = end < P + 1024u ? end - P : 1024u;
            const bool whole = lo >= P && end <= P + 1024u;
            uint32_t m[C];
            #pragma unroll
            for (int c = 0; c < C; c++) m[c] = 0u;
            for (uint32_t j = a + lane; j < b; j += 64u) {
                #pragma unroll
                for (int c = 0; c < C; c++) m[c] = truepeak_umax(m[c], y[j * C + (uint32_t)c]);
            }
            /* the wave's maximum: the values that are no NaN as floats, and whether there was one */
            float v[2 * C];
            #pragma unroll
            for (int c = 0; c < C; c++) { const bool nan = m[c] > 0x7f800000u; v[c] = truepeak_float(nan ? 0u : m[c]); v[C + c] = nan ? 1.0f : 0.0f; }
            dp_wave_max(v);
            if (lane == 0u) {                                             /* (every lane has the maxima: one delivers the C of them) */
                const bool emits = h < R.n_out;
                uint32_t* const to = emits ? A.dst + ((size_t)R.out_first + h) * C : (uint32_t*)next + H;
                #pragma unroll
                for (int c = 0; c < C; c++) {
                    const uint32_t bits = v[C + c] != 0.0f ? 0x7fc00000u : truepeak_bits(v[c]);
                    if (whole && emits) to[c] = bits; else dp_g_atomic_max_u32(to + c, bits);
                }
            }
        }
        /* the stream's first frame: the partial the slot carried belongs to hop 0, and its place is left empty for the batch after this */
        if (k == 0u && tid < (uint32_t)C) {
            uint32_t* const was = (uint32_t*)old + H + tid;
            const uint32_t carried = R.fresh ? 0u : *was;
            *was = 0u;
            if (carried) dp_g_atomic_max_u32(R.n_out ? A.dst + (size_t)R.out_first * C + tid : (uint32_t*)next + H + tid, carried);
        }
        dp_block_sync();                                                  /* the next frame of this workgroup overwrites the LDS */
    }
}

}  // namespace aacg_pipe
#endif

#endif
