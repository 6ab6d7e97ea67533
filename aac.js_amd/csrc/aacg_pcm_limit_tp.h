/*
 * aacg_pcm_limit_tp.h — the limiter of aacg_pcm_limit.h with a TRUE-PEAK detector in front of its recurrence
 * (aacg_pipeline_set_limiter_true_peak, include/aacgpu.h): the same stage of the way out (aacg_pipe_exit.h: AACG_EXIT_LIMIT), the same
 * buffers, the same records (aacg_limit_stream), and in the place of the one launch TWO on the lane's stream, both inside the stage's
 * ordered launch: the detector (aacg_pcm_limit_tp_detect_*) and the walk (aacg_pcm_limit_tp_*, aacg_engine_limit_tp.hip).
 *
 * The rule (include/aacgpu.h states it for callers).  x is the limiter's input of a slot since its reset, x[j] = 0 for j < 0; with the
 * polyphase table h[L][T], D = T / 2 and z[j] = x[j - D], block k (indices 64 k .. 64 k + 63) has
 *     ps = max |z[j][ch]|                       pt = max |acc_ph[j][ch]|  over j in the block, ph = 0 .. L-1
 *     acc = h[ph][0] * x[j];   acc = acc + h[ph][t] * x[j - t]   for t = 1 .. T-1, in that order (aacg_pcm_truepeak.h's accumulation)
 *     p  = fmaxf(ps, pt)                        every maximum an fmaxf from +0: a NaN is ignored
 * and then aacg_pcm_limit.h's rule with xk := block k of z and this p.  float32, every operation rounded on its own, nothing fused
 * (#pragma clang fp contract(off)), subnormals kept.
 *
 * Work.  Only a0 and th are serial per stream; a block's p is a maximum, free of order and of every other block.
 *   The DETECTOR fills the chip: one workgroup per input frame of the batch (grid-stride over frames), four waves.  It stages the frame's
 * 1024 x C elements into LDS as floats and in front of them the T - 1 samples that precede the frame — from the previous frame in the
 * source buffer, or for a stream's first frame from the slot's history (zeros for a fresh slot) —, the layout of truepeak_body: sample j of
 * the frame at float (T + j) C + c.  A lane takes a sample at a time with all its C channels, four phase rows at once, two taps of each
 * row as one 8-byte LDS read that is the same in every lane; the sample's maximum over phases and channels, and over the C magnitudes of
 * the sample D in front of it (z's), goes to LDS as ONE float, y[j].  Then a wave per block of 64: dp_wave_max, and the wave's first lane
 * stores the block's p into the lane's scratch, peak[frame 16 + block].  The stream's last frame leaves its last T - 1 samples as the
 * slot's new history.  The table lies in LDS, as truepeak_body's does and for its reason.
 *   The WALK is limit_body's with two differences: a lane's sample of block b is z's — the source D samples earlier, and for the first
 * D lanes of a stream's first block the history's last D samples — and p is READ from the scratch, not reduced.  One wave per stream,
 * blocks in groups of eight whose vectors are loaded back to back; no LDS.
 *
 * State.  The plain limiter's buffer, untouched in layout: [slot][parity]{a0, th, two unused, xh[64][C]} — xh is a block of z.  Beside
 * it a SECOND buffer for the history: [slot][parity][(T - 1) C] floats, sample -(T - 1) first, the layout of the true peak's history.
 * Both follow the record's parity and fresh flag: a launch pair reads parity `parity` of both (a fresh slot reads neither) and writes
 * parity ^ 1 of both; the host orders consecutive pairs with the stage's event.
 * Scratch: [frames of the largest batch][16] floats per lane of the pipeline, written by the detector and read by the walk behind it on
 * the same stream.
 * LDS of the detector: (64 + 1024) x C floats of samples, 1024 floats of maxima and 2048 bytes for the table, static.
 * Not tuned: the four phases at a time, the workgroup per frame and the group of eight were decided by reading.
 *
 * Written against devport.h like aacg_pcm_limit.h, and executed lane by lane on the CPU by tests/emu/limiter_tp_emu.cpp.
 */
#ifndef AACG_PCM_LIMIT_TP_H
#define AACG_PCM_LIMIT_TP_H

#include <stddef.h>
#include <stdint.h>

#include "aacg_pcm_limit.h"                              /* the records, the plain state's layout, limit_vec */
#include "aacg_pcm_truepeak.h"                           /* the table's limits (aacg_truepeak_check) */

#define AACG_LIMIT_TP_THREADS 256                        /* the detector's workgroup; the walk's is AACG_LIMIT_THREADS */
#define AACG_LIMIT_TP_MAX_BLOCKS 4096
#define AACG_LIMIT_TP_FRAME_BLOCKS (1024 / AACG_LIMIT_BLOCK)      /* floats of scratch a frame */
#define AACG_LIMIT_TP_LDS_BYTES(C) ((AACG_TRUEPEAK_MAX_TAPS + 1024) * (C) * 4 + 1024 * 4 + AACG_TRUEPEAK_MAX_PHASES * AACG_TRUEPEAK_MAX_TAPS * 4)
#define AACG_LIMIT_TP_HIST(T, C) (((T) - 1) * (C))       /* floats of a slot's history of one parity */

/* what one pair of launches limits */
typedef struct aacg_limit_tp_args {
    aacg_limit_args lim;       /* the plain launch's: source, destination, records, the plain state, counts, settings, which body */
    const float* table;        /* h[L][T], 16-byte aligned                                                                     */
    float*      hist;          /* [slot][2][(T - 1) C] floats                                                                  */
    float*      peak;          /* [n_frames][16] floats: the detector writes every one, the walk reads every one                */
    uint32_t phases, taps;     /* L in 1..8, T a multiple of 4 in 4..64                                                        */
} aacg_limit_tp_args;

#if !defined(AACG_LIMIT_HOST_ONLY) && !defined(AACG_TRUEPEAK_HOST_ONLY)
namespace aacg_pipe {

/* The detector.  Workgroup b of `blocks`: frames b, b + blocks, ... of the batch. */
template <typename ELEM, int C>
DP_DEVICE void limit_tp_detect_body(const aacg_limit_tp_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    float* const x = (float*)dp_lds_fixed<AACG_LIMIT_TP_LDS_BYTES(C)>();
    float* const y = x + (size_t)(AACG_TRUEPEAK_MAX_TAPS + 1024) * C;
    float* const ht = y + 1024;                                           /* the table, h[p][t] at p T + t */
    const uint32_t T = A.taps, L = A.phases, D = T / 2u, tid = (uint32_t)dp_tid(), lane = (uint32_t)dp_lane(), wave = (uint32_t)dp_wave();
    const uint32_t H = AACG_LIMIT_TP_HIST(T, C);
    constexpr float SCALE = sizeof(ELEM) == 2 ? 0.000030517578125f : 1.0f;      /* int16: x 2^-15, exact */
    for (uint32_t e = tid; e < L * T; e += AACG_LIMIT_TP_THREADS) ht[e] = A.table[e];      /* (the frame loop's first barrier stands behind this) */
    for (uint32_t f = (uint32_t)dp_block(); f < A.lim.n_frames; f += blocks) {
        /* the frame's stream: the last record that begins at or before it */
        uint32_t s = 0;
        for (uint32_t hi = A.lim.n_streams; hi - s > 1u;) { const uint32_t mid = (s + hi) >> 1; if (A.lim.rec[mid].frame_first <= f) s = mid; else hi = mid; }
        const aacg_limit_stream R = A.lim.rec[s];
        const uint32_t k = f - R.frame_first;
        const ELEM* const frame = (const ELEM*)A.lim.src + (size_t)f * 1024u * C;
        const float* const old = A.hist + ((size_t)R.slot * 2u + R.parity) * H;
        float* const next = A.hist + ((size_t)R.slot * 2u + (R.parity ^ 1u)) * H;
        /* the frame into LDS: 16 bytes a lane and turn */
        if constexpr (sizeof(ELEM) == 4) {
            for (uint32_t v = tid; v < 256u * C; v += AACG_LIMIT_TP_THREADS) ((dpi4*)(x + T * C))[v] = dp_load_nt((const dpi4*)frame + v);
        } else {
            for (uint32_t v = tid; v < 128u * C; v += AACG_LIMIT_TP_THREADS) {
                const dpi4 q4 = dp_load_nt((const dpi4*)frame + v);
                const int q[4] = {q4.x, q4.y, q4.z, q4.w};
                float lo[4], hi[4];
                #pragma unroll
                for (int i = 0; i < 4; i++) {
                    lo[i] = (float)(int16_t)(uint16_t)(uint32_t)q[i] * SCALE;               /* exact */
                    hi[i] = (float)(int16_t)(uint16_t)((uint32_t)q[i] >> 16) * SCALE;
                }
                dpf4 a, b;
                a.x = lo[0]; a.y = hi[0]; a.z = lo[1]; a.w = hi[1]; b.x = lo[2]; b.y = hi[2]; b.z = lo[3]; b.w = hi[3];
                ((dpf4*)(x + T * C))[2u * v] = a; ((dpf4*)(x + T * C))[2u * v + 1u] = b;
            }
        }
        /* the T - 1 samples in front of it: the previous frame's last, the slot's history, or — a fresh slot — zeros */
        for (uint32_t e = tid; e < H; e += AACG_LIMIT_TP_THREADS)
            x[C + e] = k ? (float)(frame - H)[e] * SCALE : R.fresh ? 0.0f : old[e];
        dp_block_sync();
        /* a sample a lane and turn: the largest of |z| and of |acc| over its L phases and C channels */
        for (uint32_t j = tid; j < 1024u; j += AACG_LIMIT_TP_THREADS) {
            const float* const xs = x + (size_t)(T + j) * C;             /* x[j], channel 0; x[j - t] lies t C floats in front */
            float m = 0.0f;
            #pragma unroll
            for (int c = 0; c < C; c++) m = __builtin_fmaxf(m, __builtin_fabsf((xs - (size_t)D * C)[c]));      /* (a NaN is ignored) */
            for (uint32_t p0 = 0; p0 < L; p0 += 4u) {
                uint32_t row[4];                                          /* (row min(p, L - 1): a row computed twice changes no maximum) */
                #pragma unroll
                for (uint32_t pp = 0; pp < 4u; pp++) row[pp] = (p0 + pp < L ? p0 + pp : L - 1u) * T;
                float acc[4][C] = {};                                     /* (every one is set by its first product below) */
                #pragma clang loop unroll(disable)
                for (uint32_t t2 = 0; t2 < T; t2 += 2u) {                 /* two taps of four rows: the same address in every lane */
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
                    for (int c = 0; c < C; c++) m = __builtin_fmaxf(m, __builtin_fabsf(acc[pp][c]));
                }
            }
            y[j] = m;
        }
        /* the stream's last frame: its last T - 1 samples are the slot's new history */
        if (k + 1u == R.frames)
            for (uint32_t e = tid; e < H; e += AACG_LIMIT_TP_THREADS) next[e] = x[(size_t)1025u * C + e];
        dp_block_sync();
        /* the frame's sixteen blocks, a wave a block */
        for (uint32_t b = wave; b < AACG_LIMIT_TP_FRAME_BLOCKS; b += AACG_LIMIT_TP_THREADS / 64u) {
            float v[1] = {y[b * AACG_LIMIT_BLOCK + lane]};
            dp_wave_max(v);
            if (lane == 0u) A.peak[(size_t)f * AACG_LIMIT_TP_FRAME_BLOCKS + b] = v[0];
        }
        dp_block_sync();                                                  /* the next frame of this workgroup overwrites the LDS */
    }
}

/* The walk.  Wave w of workgroup b of `blocks`: streams b 4 + w, then b 4 + w + blocks 4 ... */
template <typename ELEM, int C>
DP_DEVICE void limit_tp_walk_body(const aacg_limit_tp_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    typedef limit_vec<ELEM, C> V;
    typedef limit_vec<float, C> VF;
    constexpr uint32_t NB = AACG_LIMIT_GROUP, B = AACG_LIMIT_BLOCK, SF = AACG_LIMIT_STATE(C);
    const uint32_t lane = (uint32_t)dp_lane(), T = A.taps, D = T / 2u, H = AACG_LIMIT_TP_HIST(T, C);
    const float w = (float)lane * 0.015625f, c = A.lim.ceiling, r = A.lim.release;
    for (uint32_t s = (uint32_t)dp_block() * AACG_LIMIT_WAVES + (uint32_t)dp_wave(); s < A.lim.n_streams; s += blocks * AACG_LIMIT_WAVES) {
        const aacg_limit_stream R = A.lim.rec[s];
        const float G = R.gain;
        float a0 = G, th = G, xh[C], first[C];                           /* first: this lane's sample of the stream's first block where it lies in front of the batch */
        #pragma unroll
        for (int ch = 0; ch < C; ch++) xh[ch] = first[ch] = 0.0f;
        if (!R.fresh) {                                                   /* a fresh slot's state is the rule's and nothing is read */
            const float* const old = A.lim.state + ((size_t)R.slot * 2u + R.parity) * SF;
            a0 = old[0]; th = old[1];
            const VF h = *((const VF*)(old + AACG_LIMIT_STATE_HEAD) + lane);
            #pragma unroll
            for (int ch = 0; ch < C; ch++) xh[ch] = h.v[ch];
            if (lane < D) {                                               /* z[lane] = x[lane - D]: the history's sample T - 1 - D + lane */
                const float* const was = A.hist + ((size_t)R.slot * 2u + R.parity) * H + (size_t)(T - 1u - D + lane) * C;
                #pragma unroll
                for (int ch = 0; ch < C; ch++) first[ch] = was[ch];
            }
        }
        /* this lane's sample of the stream's block j of z: src[j B - D] (from block 1 on, and in block 0 from lane D on), and where the
         * block that leaves in its place goes: dst[j B] */
        const V* const src = (const V*)A.lim.src + (size_t)R.frame_first * 1024u + lane;
        V* const dst = (V*)A.lim.dst + (size_t)R.frame_first * 1024u + lane;
        const float* const peak = A.peak + (size_t)R.frame_first * AACG_LIMIT_TP_FRAME_BLOCKS;
        const uint32_t n_groups = R.frames * (1024u / B / NB);
        for (uint32_t g = 0; g < n_groups; g++) {
            float x[NB][C], pk[NB];
            V cur[NB];
            #pragma unroll
            for (uint32_t b = 0; b < NB; b++) {
                const ptrdiff_t at = (ptrdiff_t)(((size_t)g * NB + b) * B);
                const bool before = g == 0u && b == 0u && lane < D;      /* (the sample lies in front of the batch: not read here) */
                cur[b] = src[before ? at : at - (ptrdiff_t)D];
                pk[b] = peak[(size_t)g * NB + b];
            }
            #pragma unroll
            for (uint32_t b = 0; b < NB; b++) {
                const bool before = g == 0u && b == 0u && lane < D;
                #pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    float v;
                    if constexpr (sizeof(ELEM) == 4) v = cur[b].v[ch];
                    else v = (float)cur[b].v[ch] * 0.000030517578125f;    /* exact */
                    x[b][ch] = before ? first[ch] : v;
                }
            }
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
        }
        float* const next = A.lim.state + ((size_t)R.slot * 2u + (R.parity ^ 1u)) * SF;
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
