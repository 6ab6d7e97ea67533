/*
 * aacg_pcm_features.h — a resident batch's one-channel PCM framed and transformed to (log-)mel features on the device
 * (aacg_pipeline_set_features, include/aacgpu.h).  ONE launch per batch (aacg_pcm_features_*, aacg_engine_features.hip) on the lane's
 * stream, the LAST stage of the way out: behind the transform, the mix and the resampler, where the copy down or the caller's device
 * memory is written for a pipeline without the stage.
 *
 * The rule (include/aacgpu.h states it for callers).  With basis[R][K], fb[n_mels][B], B = R / 2, feature frame j = 0, 1, ... of a
 * stream slot since its reset covers x[j H - P + k], k = 0 .. K-1, x[n] = 0 for n < 0, and in float32 throughout
 *     lin[r] = fmaf(basis[r][K-1], x[jH-P+K-1], ... fmaf(basis[r][0], x[jH-P], +0) ...)      one k-ordered fused chain from +0
 *     pw[b]  = lin[2b] * lin[2b] + lin[2b+1] * lin[2b+1]                                     each product rounded, then the sum
 *     mel[m] = fmaf(fb[m][B-1], pw[B-1], ... fmaf(fb[m][0], pw[0], +0) ...)                  one b-ordered fused chain from +0
 *     out[m] = log ? log10f(fmaxf(mel[m], floor)) : mel[m]
 * every term computed whatever its coefficient.  x is the stream's PCM as the pipeline would have delivered it; int16: the already
 * rounded sample times 2^-15 (exact).  After N consumed samples a slot has emitted count(N) = max(0, floor((N + P - K) / H) + 1) frames.
 *
 * State.  A stream slot carries its clock N — on the HOST, in 64 bits, which passes the launch what follows from it: how many frames
 * the stream's samples of this batch complete, and where the first of them begins relative to the batch's first sample (off0, in
 * -(K-1) .. 0: a frame not yet emitted ends at or behind the clock, and the one before it was emitted) — and on the device its last
 * K - 1 input samples as floats, [slot][parity][K - 1], double-buffered: a launch reads parity `parity` (or takes zeros if the stream
 * is fresh: after a reset nothing is read, so nothing need be cleared) and writes parity ^ 1, the last K - 1 samples of the old history
 * followed by the batch's.  The host orders consecutive launches and flips the parity, as for the resampler.
 *
 * Work.  One workgroup (sixteen waves) per ITEM: sixteen consecutive feature frames of a stream (grid-stride over the batch's items; a
 * stream that completes no frame is one item all the same, for its history and its padding).  The item's samples — (nf - 1) H + K of
 * them, the history in front where the frames reach back — go into LDS as floats, so that element (k, j) of the frame operand is the
 * staged sample j H + k: no im2col.  The contraction [R x K] . [K x 16] runs on v_mfma_f32_16x16x4_f32 (dp_mfma_16x16x4): tiles of 16
 * rows x 16 frames, ONE accumulator per tile through the whole k chain — which is the rule's chain, k0..k3 inside an instruction and
 * instruction after instruction — and a wave carries two row tiles side by side on one frame operand, so that the second instruction
 * hides the first one's dependent latency.  R and the frame count are padded to the tile in the INDEXING (a row or a frame beyond the
 * end repeats the last one, and its results are dropped); K is a multiple of 4, so no chain has a term more than the rule's.  The
 * accumulator layout (frame on the lane, four consecutive rows in the four registers) puts a bin's two quadrature rows into one lane:
 * the power needs no lane movement and goes to LDS as pw[b][16].  The mel chain is VALU fmaf, a lane per (m, frame), two chains
 * side by side, over exactly B terms.  Both loops take their operands in groups — eight k steps' 24, eight bins' 24 — so that the loads
 * are in flight together: with one load in front of every instruction the kernel waited a memory round trip per step (0.38 ms for
 * 8 750 Whisper frames; DESIGN.md 7a has what the grouping gave).  The order of the terms is the rule's either way.
 *
 * basis and fb come THROUGH THE CACHE, like the resampler's table: read-only, shared by every workgroup of every launch.  Decided by
 * reading, not tuned: the tile shape (16 x 16 x 4 keeps the staged samples at 15 H + K floats; the 32 x 32 form would need 31 H + K),
 * the table placement, and the LDS layout (adjacent frames lie H floats apart, which for H = 160 lands sixteen lanes on two banks).
 * LDS: (15 x 1024 + 1024) x 4 bytes of samples + 513 x 16 x 4 of power = 98368 bytes, static.
 *
 * Writes.  Packed: [stream of the batch][n_out[s]][n_mels], tight, stream s at frame out_first[s].  Planar (row != 0):
 * [stream][n_mels][row], and the padding behind n_out[s] is written with the rule's value for mel = 0 (0, or log10f(floor)), the
 * stream's items each a share of it: every element of the n_streams x n_mels x row block is written exactly once, nothing outside it.
 *
 * Written against devport.h like aacg_pcm_resample.h, and executed lane by lane on the CPU by tests/emu/features_emu.cpp.
 */
#ifndef AACG_PCM_FEATURES_H
#define AACG_PCM_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#ifndef AACG_FEATURES_HOST_ONLY                          /* (aacg_features.cpp and aacg_pipe_exit.h's users take the limits and the records alone) */
#include <math.h>
#include "devport.h"
#endif

#define AACG_FEATURES_THREADS 1024            /* sixteen waves: a workgroup's LDS admits one workgroup per CU, so the waves that hide each other's loads are its own */
#define AACG_FEATURES_CHAINS 2                /* mel chains of a lane side by side: 64 groups of sixteen lanes x 2 cover 128 bands */
#define AACG_FEATURES_MAX_BLOCKS 4096
#define AACG_FEATURES_TILE 16              /* feature frames of an item: the MFMA tile's columns */
#define AACG_FEATURES_MAX_K 1024
#define AACG_FEATURES_MAX_R 1026
#define AACG_FEATURES_MAX_MELS 128
#define AACG_FEATURES_X_FLOATS ((AACG_FEATURES_TILE - 1) * AACG_FEATURES_MAX_K + AACG_FEATURES_MAX_K)
#define AACG_FEATURES_LDS_BYTES ((AACG_FEATURES_X_FLOATS + (AACG_FEATURES_MAX_R / 2) * AACG_FEATURES_TILE) * 4)

/* one stream of a launch; travels up in the lane's staging block behind the resampler's records */
typedef struct aacg_features_stream {
    uint32_t in_first;         /* the stream's first sample in the launch's source, in elements                                */
    uint32_t n_in;             /* its samples in this batch                                                                    */
    uint32_t out_first;        /* packed layout: the stream's first feature frame (the sum of n_out of the streams before it)  */
    uint32_t n_out;            /* feature frames this launch emits for the stream (0: none is completed yet)                   */
    uint32_t item_first;       /* the stream's first item: max(1, ceil(n_out / 16)) items each, ascending from 0, no gaps      */
    int32_t  off0;             /* where its first emitted frame begins, relative to in_first: -(K - 1) .. 0                    */
    uint32_t slot;
    uint32_t flags;            /* bit 0: the history buffer the launch reads (it writes the other); bit 1: fresh, history = 0  */
} aacg_features_stream;

/* what one launch transforms */
typedef struct aacg_features_args {
    const void* src;           /* one channel of PCM, float or int16, the streams' samples at in_first                         */
    float*      dst;           /* packed [sum n_out][n_mels] or planar [n_streams][n_mels][row]                                */
    const aacg_features_stream* rec;      /* n_streams records                                                                 */
    const float* basis;        /* [R][K]                                                                                       */
    const float* fb;           /* [n_mels][R / 2]                                                                              */
    float*      hist;          /* [slot][2][K - 1] floats                                                                      */
    uint32_t n_streams, n_items;
    uint32_t K, H, R, n_mels;
    float    floor;
    uint32_t log;
    uint32_t row;              /* 0: packed; else planar, feature frames per row (>= every n_out)                              */
    uint32_t elem;             /* 4 or 2: which body the host launches; a body does not read it                                */
} aacg_features_args;

/* 0 if (K, H, P, R, n_mels) is a stage the kernels serve, else which limit it breaks (aacg_features_why) */
static inline int aacg_features_check(uint32_t K, uint32_t H, uint32_t P, uint32_t R, uint32_t n_mels)
{
    if (K < 32 || K > AACG_FEATURES_MAX_K || (K & 3u)) return 1;
    if (H < 1 || H > K) return 2;
    if (P >= K) return 3;
    if (R < 2 || R > AACG_FEATURES_MAX_R || (R & 1u)) return 4;
    if (n_mels < 1 || n_mels > AACG_FEATURES_MAX_MELS) return 5;
    return 0;
}
static inline const char* aacg_features_why(int code)
{
    return code == 1 ? "frame_length is not a multiple of 4 in 32..1024" : code == 2 ? "hop is not in 1..frame_length" :
           code == 3 ? "pad_left is not below frame_length" : code == 4 ? "n_rows is not even in 2..1026" :
           code == 5 ? "n_mels is not in 1..128" : "";
}
/* frames a slot has emitted after N consumed samples */
static inline uint64_t aacg_features_count(uint32_t K, uint32_t H, uint32_t P, uint64_t N)
{
    return N + P < K ? 0u : (N + P - K) / H + 1u;
}
#define AACG_FEATURES_ITEMS(n_out) ((n_out) ? ((n_out) + AACG_FEATURES_TILE - 1u) / AACG_FEATURES_TILE : 1u)      /* (a macro: host and device code share it) */
static inline uint32_t aacg_features_items(uint32_t n_out) { return AACG_FEATURES_ITEMS(n_out); }
/* a stream's record from its clock N and what the batch brings: n_out, off0 and the item count; the places are the caller's */
static inline void aacg_features_span(uint32_t K, uint32_t H, uint32_t P, uint64_t N, uint32_t n_in, aacg_features_stream* r)
{
    const uint64_t j0 = aacg_features_count(K, H, P, N);
    r->n_in = n_in;
    r->n_out = (uint32_t)(aacg_features_count(K, H, P, N + n_in) - j0);
    r->off0 = (int32_t)((int64_t)(j0 * H) - (int64_t)P - (int64_t)N);
}

#ifndef AACG_FEATURES_HOST_ONLY
namespace aacg_pipe {

/* Workgroup b of `blocks`: items b, b + blocks, ... of the batch. */
template <typename ELEM>
DP_DEVICE void features_body(const aacg_features_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert(sizeof(ELEM) == 4 || sizeof(ELEM) == 2, "f32 or int16 PCM");
    float* const xs = (float*)dp_lds_fixed<AACG_FEATURES_LDS_BYTES>();
    float* const pw = xs + AACG_FEATURES_X_FLOATS;
    const uint32_t K = A.K, H = A.H, R = A.R, B = A.R >> 1, NM = A.n_mels, tid = (uint32_t)dp_tid(), lane = (uint32_t)dp_lane(), wave = (uint32_t)dp_wave();
    const uint32_t T = AACG_FEATURES_TILE, hist_n = K - 1u;
    const float pad_value = A.log ? log10f(fmaxf(0.0f, A.floor)) : 0.0f;
    for (uint32_t it = (uint32_t)dp_block(); it < A.n_items; it += blocks) {
        /* the item's stream: the last record that begins at or before it */
        uint32_t s = 0;
        for (uint32_t hi = A.n_streams; hi - s > 1u;) { const uint32_t mid = (s + hi) >> 1; if (A.rec[mid].item_first <= it) s = mid; else hi = mid; }
        const aacg_features_stream S = A.rec[s];
        const uint32_t t = it - S.item_first, items = AACG_FEATURES_ITEMS(S.n_out), fresh = S.flags & 2u;
        const uint32_t nf = S.n_out - t * T < T ? S.n_out - t * T : T;      /* (0 for the one item of a stream that emits nothing) */
        const ELEM* const in = (const ELEM*)A.src + S.in_first;
        const float* const old = A.hist + ((size_t)S.slot * 2u + (S.flags & 1u)) * hist_n;
        /* sample p of the stream, counted from the batch's first: the batch's own, the slot's history in front of it, or zero */
        auto sample = [&](int32_t p) -> float {
            if (p >= 0) {
                if ((uint32_t)p >= S.n_in) return 0.0f;                  /* (no record of the host's reaches here) */
                if constexpr (sizeof(ELEM) == 4) return (float)in[p]; else return (float)in[p] * 0.000030517578125f;      /* exact */
            }
            return fresh || p < -(int32_t)hist_n ? 0.0f : old[(int32_t)hist_n + p];
        };
        if (nf) {
            /* the item's samples into LDS: xs[i] = sample a + i */
            const int32_t a = S.off0 + (int32_t)(t * T * H);
            const uint32_t len = (nf - 1u) * H + K;
            for (uint32_t i = tid; i < len; i += AACG_FEATURES_THREADS) xs[i] = sample(a + (int32_t)i);
            dp_block_sync();
            /* rows x frames on the matrix cores: wave w takes the row-tile pairs w, w + 16, ... */
            const uint32_t kk = lane >> 4, c = lane & 15u, jc = c < nf ? c : nf - 1u, row_tiles = (R + 15u) >> 4;
            const float* const xp = xs + (size_t)jc * H + kk;
            for (uint32_t pair = wave; 2u * pair < row_tiles; pair += AACG_FEATURES_THREADS / 64u) {
                const uint32_t r0 = 32u * pair + c, r1 = r0 + 16u;
                const float* const b0 = A.basis + (size_t)(r0 < R ? r0 : R - 1u) * K + kk;
                const float* const b1 = A.basis + (size_t)(r1 < R ? r1 : R - 1u) * K + kk;
                float acc0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                /* eight steps at a time: their 24 operands are loaded first, so that the loads are in flight together and not each in
                 * front of its own instruction; the steps themselves stay in k order on the one accumulator */
                uint32_t k = 0;
                for (; k + 32u <= K; k += 32u) {
                    float u0[8], u1[8], x[8];
                    #pragma unroll
                    for (int i = 0; i < 8; i++) { u0[i] = b0[k + 4u * (uint32_t)i]; u1[i] = b1[k + 4u * (uint32_t)i]; x[i] = xp[k + 4u * (uint32_t)i]; }
                    #pragma unroll
                    for (int i = 0; i < 8; i++) { dp_mfma_16x16x4(u0[i], x[i], acc0); dp_mfma_16x16x4(u1[i], x[i], acc1); }
                }
                for (; k < K; k += 4u) {
                    const float x = xp[k];
                    dp_mfma_16x16x4(b0[k], x, acc0);
                    dp_mfma_16x16x4(b1[k], x, acc1);
                }
                /* this lane: frame c, rows 4 kk .. 4 kk + 3 of either tile — two bins each */
                const uint32_t bin0 = 16u * pair + 2u * kk, bin1 = bin0 + 8u;
                /* (the arithmetic in every lane, only the stores under the condition: each product rounded, then the sum) */
                const float s00 = acc0[0] * acc0[0], s01 = acc0[1] * acc0[1], s02 = acc0[2] * acc0[2], s03 = acc0[3] * acc0[3];
                const float s10 = acc1[0] * acc1[0], s11 = acc1[1] * acc1[1], s12 = acc1[2] * acc1[2], s13 = acc1[3] * acc1[3];
                const float p00 = s00 + s01, p01 = s02 + s03, p10 = s10 + s11, p11 = s12 + s13;
                if (bin0 < B) pw[(size_t)bin0 * T + c] = p00;
                if (bin0 + 1u < B) pw[(size_t)(bin0 + 1u) * T + c] = p01;
                if (bin1 < B) pw[(size_t)bin1 * T + c] = p10;
                if (bin1 + 1u < B) pw[(size_t)(bin1 + 1u) * T + c] = p11;
            }
            dp_block_sync();
            /* the mel chains: lane (m, frame), AACG_FEATURES_CHAINS m side by side (one beyond the end repeats the last and is dropped);
             * eight bins' operands loaded together, the terms in b order */
            const uint32_t j = tid & 15u, mg = tid >> 4, G = AACG_FEATURES_THREADS / 16u;
            for (uint32_t m0 = mg; m0 < NM; m0 += AACG_FEATURES_CHAINS * G) {
                const float* f[AACG_FEATURES_CHAINS];
                float mel[AACG_FEATURES_CHAINS];
                #pragma unroll
                for (int q = 0; q < AACG_FEATURES_CHAINS; q++) { const uint32_t m = m0 + G * (uint32_t)q; f[q] = A.fb + (size_t)(m < NM ? m : NM - 1u) * B; mel[q] = 0.0f; }
                uint32_t b = 0;
                for (; b + 8u <= B; b += 8u) {
                    float p[8], w[AACG_FEATURES_CHAINS][8];
                    #pragma unroll
                    for (int i = 0; i < 8; i++) {
                        p[i] = pw[(size_t)(b + (uint32_t)i) * T + j];
                        #pragma unroll
                        for (int q = 0; q < AACG_FEATURES_CHAINS; q++) w[q][i] = f[q][b + (uint32_t)i];
                    }
                    #pragma unroll
                    for (int i = 0; i < 8; i++) {
                        #pragma unroll
                        for (int q = 0; q < AACG_FEATURES_CHAINS; q++) mel[q] = dp_fma(w[q][i], p[i], mel[q]);
                    }
                }
                for (; b < B; b++) {
                    const float p = pw[(size_t)b * T + j];
                    #pragma unroll
                    for (int q = 0; q < AACG_FEATURES_CHAINS; q++) mel[q] = dp_fma(f[q][b], p, mel[q]);
                }
                #pragma unroll
                for (int q = 0; q < AACG_FEATURES_CHAINS; q++) {
                    const uint32_t m = m0 + G * (uint32_t)q;
                    if (m < NM && j < nf) {
                        const float v = A.log ? log10f(fmaxf(mel[q], A.floor)) : mel[q];
                        const size_t at = (size_t)t * T + j;             /* the frame's place in the stream's output */
                        if (A.row) A.dst[((size_t)s * NM + m) * A.row + at] = v;
                        else A.dst[((size_t)S.out_first + at) * NM + m] = v;
                    }
                }
            }
        }
        /* planar: this item's share of the padding behind the stream's n_out frames, in every row */
        if (A.row) {
            const uint32_t pad = A.row - S.n_out, share = (pad + items - 1u) / items;
            const uint32_t lo = t * share < pad ? t * share : pad, hi = pad - lo < share ? pad : lo + share;
            for (uint32_t m = 0; m < NM; m++) {
                float* const d = A.dst + ((size_t)s * NM + m) * A.row + S.n_out;
                for (uint32_t e = lo + tid; e < hi; e += AACG_FEATURES_THREADS) d[e] = pad_value;
            }
        }
        /* the stream's last item: the last K - 1 samples of (the old history, the batch's samples) are the slot's new history */
        if (t + 1u == items) {
            float* const next = A.hist + ((size_t)S.slot * 2u + ((S.flags & 1u) ^ 1u)) * hist_n;
            for (uint32_t e = tid; e < hist_n; e += AACG_FEATURES_THREADS) next[e] = sample((int32_t)S.n_in - (int32_t)hist_n + (int32_t)e);
        }
        dp_block_sync();                                                  /* the next item of this workgroup overwrites the LDS */
    }
}

}  // namespace aacg_pipe
#endif

#endif
