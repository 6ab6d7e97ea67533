/*
 * aacg_pcm_loudness.h — a loudness TAP on a resident batch's transform PCM (aacg_pipeline_set_loudness, include/aacgpu.h): two biquad
 * sections per channel, the energy and the sample peak of every `hop` samples, a record of two floats per hop and channel.  ONE launch per
 * batch (aacg_pcm_loudness_*, aacg_engine_loudness.hip) on the lane's stream behind aacg_pipeline_join; it reads the buffer the transform
 * wrote and writes beside it — the PCM's way out (aacg_pipe_exit.h) does not know it.
 *
 * The rule (include/aacgpu.h states it for callers).  Per sample x of a channel, for section i = 0 then 1 with v = x into section 0:
 *     y = (b0 v) + z1;   z1 = ((b1 v) - (a1 y)) + z2;   z2 = (b2 v) - (a2 y);   v = y
 * then e = e + (v v) and peak = max(peak, |x|): float32, every operation rounded on its own, nothing fused (#pragma clang fp
 * contract(off) as resample_body has it), subnormals kept.  After every `hop` samples since the slot's reset {e, peak} leaves and both
 * restart at +0.  int16 PCM: x is the sample times 2^-15 (exact).
 *
 * Work.  A CHAIN is one (stream of the batch, channel): its samples are strictly serial, so one lane owns a chain for the whole batch.
 * A workgroup is ONE wave of 64 lanes and takes G = 64 / C streams (lane = g C + c; the 64 - G C lanes left over idle).  Memory is not
 * serial: the group's streams advance together in tiles of 32 samples, and a tile's G x 32 x C elements arrive as 16-byte non-temporal
 * loads spread over the 64 lanes (a stream's frames are contiguous in the lane's packed PCM, so a tile is 8 C or — int16 — 4 C whole
 * vectors), are converted to float and transposed on the way into LDS — x[t][lane] in rows of 65 floats, so that the wave's 64 reads of
 * a sample step are 64 consecutive words and the lanes that write one stream's consecutive vectors meet different banks — and the NEXT
 * tile's loads are issued, all of them unconditionally and back to back, before the lanes walk the current one out of LDS.  Streams of a
 * ragged batch that have no frame left load the batch's first vector in the place of theirs, write nothing, and their lanes wait.
 * The two sections overlap in the instruction stream: eight samples are written out straight wherever no hop ends among them (section 1
 * of sample t does not depend on section 0 of sample t + 1, and nothing stands between them for the scheduler); eight samples with a
 * hop's end among them take a checked step each.
 * LDS: 32 rows of 65 floats, 8320 bytes, static, whatever C.  (A tile of 64 samples makes a lane hold sixteen vectors in flight with
 * their addresses, and the three-channel f32 body then no longer fits the register file without a spill.)
 *
 * State: [slot][parity][C][6] floats — z1, z2 of section 0, z1, z2 of section 1, the partial e, the partial peak — double-buffered like
 * the resampler's history: a chain reads parity `parity` (a fresh slot reads nothing: zeros) and writes parity ^ 1; the host orders
 * consecutive launches with an event and flips the parity.  The 64-bit clock stays on the host, which passes n0 = N mod hop.
 * Output: packed [stream s][n_out[s]][C][2] floats, stream s at record out_first[s]; a lane stores its own eight bytes, at most n_out[s]
 * times whatever the records say.  Not tuned: the tile, the one wave per workgroup and the LDS layout were decided by reading.
 *
 * Written against devport.h like aacg_pcm_resample.h, and executed lane by lane on the CPU by tests/emu/loudness_emu.cpp.
 */
#ifndef AACG_PCM_LOUDNESS_H
#define AACG_PCM_LOUDNESS_H

#include <stddef.h>
#include <stdint.h>

#ifndef AACG_LOUDNESS_HOST_ONLY                          /* (aacg_loudness.cpp and aacg_pipeline.hip take the limits and the records alone) */
#include "devport.h"
#endif

/* X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of a body, and the HOST
 * picks the body — each is a kernel entry of its own (aacg_pcm_loudness_<name>_c<C>, aacg_engine_loudness.hip). */
#define AACG_LOUDNESS_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_LOUDNESS_THREADS 64
#define AACG_LOUDNESS_TILE 32                             /* samples of a tile: 1024 / 32 = 32 tiles a frame */
#define AACG_LOUDNESS_MAX_BLOCKS 4096
#define AACG_LOUDNESS_MAX_HOP (1u << 20)
#define AACG_LOUDNESS_MAX_VECTORS 0xffffffffull           /* 16-byte vectors of a batch's PCM: a lane counts them in 32 bits (64 GiB) */
#define AACG_LOUDNESS_STATE 6                             /* floats of a chain's state */
#define AACG_LOUDNESS_ROW 65                              /* floats between consecutive samples in LDS: 64 chains and one of padding */
#define AACG_LOUDNESS_LDS_BYTES (AACG_LOUDNESS_TILE * AACG_LOUDNESS_ROW * 4)

/* one stream of a launch; travels up in the lane's staging block behind the feature stage's records */
typedef struct aacg_loudness_stream {
    uint32_t frame_first;      /* the stream's first frame in the transform's packed PCM                                       */
    uint32_t frames;           /* >= 1                                                                                         */
    uint32_t out_first;        /* the stream's first record per channel (the sum of n_out of the streams before it)            */
    uint32_t n_out;            /* records per channel this launch emits for the stream                                         */
    uint32_t n0;               /* the slot's clock modulo hop at the stream's first frame                                      */
    uint32_t slot;
    uint32_t parity;           /* the state buffer the stream's chains read; they write parity ^ 1                             */
    uint32_t fresh;            /* nothing consumed since the slot's reset: the state is zeros and is not read                  */
} aacg_loudness_stream;

/* what one launch meters */
typedef struct aacg_loudness_args {
    const void* src;           /* the transform's packed PCM: [frame][1024][C] elements, 16-byte aligned                       */
    float*      dst;           /* [sum n_out][C][2] floats, 8-byte aligned                                                     */
    const aacg_loudness_stream* rec;      /* n_streams records, frame_first ascending from 0, no gaps                          */
    float*      state;         /* [slot][2][C][6] floats                                                                       */
    uint32_t n_streams, n_frames, hop;
    float    coeffs[10];       /* two sections {b0, b1, b2, a1, a2}                                                            */
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_LOUDNESS_BODIES); a body does not read them      */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_loudness_args;

/* records per channel after N samples, and what `samples` more emit at the clock n0 (any value: only n0 mod hop counts) */
static inline uint64_t aacg_loudness_emits(uint32_t hop, uint64_t n0, uint64_t samples) { return (n0 % hop + samples) / hop; }

#ifndef AACG_LOUDNESS_HOST_ONLY
namespace aacg_pipe {

DP_DEVICE float loudness_bits(int v) { float f; __builtin_memcpy(&f, &v, 4); return f; }
/* A value that was loaded from memory has ARRIVED behind this point.  The compiler waits for a load where its value is first used; for
 * the chain's state and its record that is inside the tile loop, where the wait — the counter is in order: for everything — would then
 * stand in every turn, in front of the walk and behind the next tile's loads, which it would bring to a halt.  Nothing on the CPU. */
#ifdef AACG_EMU_BUILD
DP_DEVICE void loudness_settle(float&) {}
DP_DEVICE void loudness_settle(uint32_t&) {}
#else
DP_DEVICE void loudness_settle(float& v) { asm volatile("" : "+v"(v)); }
DP_DEVICE void loudness_settle(uint32_t& v) { asm volatile("" : "+v"(v)); }
#endif

/* a chain in registers: the coefficients of both sections, their state, the hop's energy and peak */
struct loudness_chain {
    float b00, b01, b02, a01, a02, b10, b11, b12, a11, a12;
    float z10, z20, z11, z21, e, pk;
};
DP_DEVICE void loudness_step(loudness_chain& h, float xv)
{
#pragma clang fp contract(off)
    const float y0 = (h.b00 * xv) + h.z10;
    h.z10 = ((h.b01 * xv) - (h.a01 * y0)) + h.z20;
    h.z20 = (h.b02 * xv) - (h.a02 * y0);
    const float y1 = (h.b10 * y0) + h.z11;
    h.z11 = ((h.b11 * y0) - (h.a11 * y1)) + h.z21;
    h.z21 = (h.b12 * y0) - (h.a12 * y1);
    h.e = h.e + (y1 * y1);
    h.pk = __builtin_fmaxf(h.pk, __builtin_fabsf(xv));
}

/* Workgroup b of `blocks`: streams b G .. b G + G - 1 of the batch, then b G + blocks G ..., G = 64 / C. */
template <typename ELEM, int C>
DP_DEVICE void loudness_body(const aacg_loudness_args& A, uint32_t blocks)
{
#pragma clang fp contract(off)
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    constexpr uint32_t TS = AACG_LOUDNESS_TILE, G = 64u / C, EPV = 16u / sizeof(ELEM), VPS = TS * C / EPV, NV = (G * VPS + 63u) / 64u;
    constexpr uint32_t ROW = AACG_LOUDNESS_ROW;
    float* const x = (float*)dp_lds_fixed<AACG_LOUDNESS_LDS_BYTES>();
    const uint32_t lane = (uint32_t)dp_tid(), g = lane / C, c = lane - g * C, hop = A.hop;
    for (uint32_t s0 = (uint32_t)dp_block() * G; s0 < A.n_streams; s0 += blocks * G) {
        const bool mine = g < G && s0 + g < A.n_streams;
        aacg_loudness_stream R = {};
        if (mine) R = A.rec[s0 + g];
        uint32_t K = 0;                                                   /* the group's tiles: its longest stream's, through LDS */
        ((uint32_t*)x)[lane] = lane < G && s0 + lane < A.n_streams ? A.rec[s0 + lane].frames * (1024u / TS) : 0u;
        dp_wave_sync();
        for (uint32_t gs = 0; gs < G; gs++) { const uint32_t n = ((const uint32_t*)x)[gs]; K = n > K ? n : K; }
        dp_wave_sync();                                                   /* (the first tile goes where the counts lay) */
        /* this lane's share of a tile's loads: vector v = i 64 + lane is vector v mod VPS of stream v / VPS of the group — where it
         * begins, and how many tiles that stream has (0: no such stream) */
        uint32_t vfirst[NV], vtiles[NV];                                  /* (in 16-byte vectors from src: below 2^32, AACG_LOUDNESS_MAX_VECTORS) */
        #pragma unroll
        for (uint32_t i = 0; i < NV; i++) {
            const uint32_t v = i * 64u + lane, gs = v / VPS, w = v - gs * VPS;
            const bool has = gs < G && s0 + gs < A.n_streams;
            const uint32_t first = has ? A.rec[s0 + gs].frame_first : 0u;
            vtiles[i] = has ? A.rec[s0 + gs].frames * (1024u / TS) : 0u;
            vfirst[i] = first * (1024u * C / EPV) + w;
        }
        /* the chain: a fresh slot's state is zeros and nothing is read */
        loudness_chain ch;
        ch.b00 = A.coeffs[0]; ch.b01 = A.coeffs[1]; ch.b02 = A.coeffs[2]; ch.a01 = A.coeffs[3]; ch.a02 = A.coeffs[4];
        ch.b10 = A.coeffs[5]; ch.b11 = A.coeffs[6]; ch.b12 = A.coeffs[7]; ch.a11 = A.coeffs[8]; ch.a12 = A.coeffs[9];
        ch.z10 = ch.z20 = ch.z11 = ch.z21 = ch.e = ch.pk = 0.0f;
        if (mine && !R.fresh) {
            const float* const old = A.state + (((size_t)R.slot * 2u + R.parity) * C + c) * AACG_LOUDNESS_STATE;
            ch.z10 = old[0]; ch.z20 = old[1]; ch.z11 = old[2]; ch.z21 = old[3]; ch.e = old[4]; ch.pk = old[5];
        }
        loudness_settle(ch.z10); loudness_settle(ch.z20); loudness_settle(ch.z11); loudness_settle(ch.z21); loudness_settle(ch.e); loudness_settle(ch.pk);
        loudness_settle(R.n_out);
        uint32_t left = hop - R.n0, j = 0;                               /* samples to the hop's end; records written */
        float* const out = A.dst + ((size_t)R.out_first * C + c) * 2u;   /* record j of this chain: out + j C 2 */
        const uint32_t my_tiles = mine ? R.frames * (1024u / TS) : 0u;
        /* tile k of the group into registers.  EVERY lane loads every time, one load behind the other with nothing between them: a
         * vector that is not there (a stream with no tile k, a lane past the group's vectors) reads the batch's first 16 bytes instead */
        dpi4 pre[NV];
        auto fetch = [&](uint32_t k) {
            #pragma unroll
            for (uint32_t i = 0; i < NV; i++) pre[i] = dp_load_nt((const dpi4*)A.src + (k < vtiles[i] ? vfirst[i] + k * VPS : 0u));
        };
        /* ... and from the registers into LDS, as floats, sample t of chain n at x[t ROW + n] */
        auto spill = [&](uint32_t k) {
            #pragma unroll
            for (uint32_t i = 0; i < NV; i++) {
                const uint32_t v = i * 64u + lane, gs = v / VPS, w = v - gs * VPS;
                if (k >= vtiles[i]) continue;
                const int q[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
                #pragma unroll
                for (uint32_t d = 0; d < EPV; d++) {
                    const uint32_t el = w * EPV + d, t = el / C, cc = el - t * C;
                    float f;
                    if constexpr (sizeof(ELEM) == 4) f = loudness_bits(q[d]);
                    else f = (float)(int16_t)(uint16_t)((uint32_t)q[d >> 1] >> (16u * (d & 1u))) * 0.000030517578125f;      /* exact */
                    x[t * ROW + gs * C + cc] = f;
                }
            }
        };
        if (K) fetch(0);
        for (uint32_t k = 0; k < K; k++) {
            if (k) dp_wave_sync();                                        /* every lane has walked tile k - 1 */
            spill(k);
            dp_wave_sync();
            if (k + 1u < K) fetch(k + 1u);                                /* in flight while the lanes walk */
            if (k >= my_tiles) continue;
            const float* const xs = x + lane;
            for (uint32_t t0 = 0; t0 < TS; t0 += 8u) {
                if (left > 8u) {                                          /* no hop ends here: eight samples straight */
                    #pragma unroll
                    for (uint32_t d = 0; d < 8u; d++) loudness_step(ch, xs[(t0 + d) * ROW]);
                    left -= 8u;
                } else {
                    #pragma unroll
                    for (uint32_t d = 0; d < 8u; d++) {
                        loudness_step(ch, xs[(t0 + d) * ROW]);
                        if (--left == 0u) {
                            if (j < R.n_out) { float* const o = out + (size_t)j * C * 2u; o[0] = ch.e; o[1] = ch.pk; }
                            j++; ch.e = 0.0f; ch.pk = 0.0f; left = hop;
                        }
                    }
                }
            }
        }
        if (mine) {
            float* const next = A.state + (((size_t)R.slot * 2u + (R.parity ^ 1u)) * C + c) * AACG_LOUDNESS_STATE;
            next[0] = ch.z10; next[1] = ch.z20; next[2] = ch.z11; next[3] = ch.z21; next[4] = ch.e; next[5] = ch.pk;
        }
        dp_wave_sync();                                                   /* the next group's first tile overwrites this one's last */
    }
}

}  // namespace aacg_pipe
#endif

#endif
