/*
 * aacg_pcm_trim.h — a resident batch's packed PCM cut to each stream's window on the device (aacg_pipeline_set_trim, include/aacgpu.h):
 * the encoder's priming off the front, the padding off the end, and only the kept samples cross the link.  ONE launch per batch
 * (aacg_pcm_trim_*, aacg_engine_trim.hip) on the lane's stream, the LAST PCM stage of the way out: behind the resampler (or the limiter,
 * the mix or the transform, whichever wrote last), where the planar launch or the copy down reads for a pipeline without the stage.
 *
 * The rule (include/aacgpu.h states it for callers).  A stream slot has a window (skip S, keep K) and a position Q, all in samples per
 * channel of what the stage receives, 64-bit, ON THE HOST (aacg_trim_span below is the whole arithmetic).  A batch in which the slot's
 * stream brings n_in samples keeps those with index q in [Q, Q + n_in) n [S, S + K): one contiguous range of n_keep samples, possibly
 * none, copied bit for bit.  The stage has NO device state: a launch sees per stream where the kept range begins in the source and how
 * long it is, and nothing orders it behind the launch of the batch before.
 *
 * Work.  An ITEM is a tile of AACG_TRIM_TILE consecutive kept samples of one stream with all their channels (grid-stride over the batch's
 * items; the stream is found by a search over item_first, like the feature stage's).  A stream that keeps nothing is one item in the
 * planar layout, for its padding, and none in the packed one.
 *
 * Alignment.  The source of a stream begins at (place + skip) x C elements and the packed destination at out_first x C: each is aligned
 * to ONE ELEMENT only (int16 mono with an odd skip: 2 bytes), and the two residues modulo 16 bytes differ from each other.  The body of
 * an item all the same moves as whole, naturally aligned 16-byte vectors ON BOTH SIDES, realigned THROUGH LDS: the workgroup loads the
 * aligned vectors that cover the item's source bytes into LDS as they lie (so the item's first element sits at the source's residue),
 * and a lane then puts a destination vector together from the 16 / E elements at its place in LDS — ds reads of one element each, which
 * need the element's alignment only — and stores it whole.  Through LDS and not in registers because the shift between the two residues
 * is a run-time value per stream: in registers a lane would need its own and its neighbour's source vector (a second load of every
 * vector, or a cross-lane move) and a byte-wise funnel shift by a variable count for either element size, and the planar layout
 * needs a gather with stride C on top, which LDS serves with the same reads.  Decided by reading, NOT TUNED: neither this, nor the tile,
 * nor the workgroup size, nor the LDS reads' bank behaviour (a planar gather reads at a stride of C elements), nor the extent's partial
 * last vector, which ONE lane copies element by element (up to eight in turn), nor the two barriers that a planar item which keeps
 * nothing still passes.
 *
 * Bounds.  No load reaches outside the source's extent (src_elems): the aligned vector that holds an item's first element begins at or
 * behind the source's (16-byte aligned) start, and a vector that would end behind the extent is taken element by element instead.
 * Races.  Two streams that are neighbours in the packed output may share a 16-byte granule, and other workgroups write them in any
 * order: the elements in front of an item's first aligned granule and behind its last whole one are ELEMENT stores, nothing is ever
 * read-modify-written, and no byte outside a stream's own n_keep x C elements is stored.
 *
 * Writes.  Packed: [stream of the batch][n_keep[s]][C], tight, stream s at sample out_first[s].  Planar (row != 0): [stream][C][row]
 * de-interleaved, row a multiple of 1024 so that every row and every tile of it begins 16-byte aligned, and the padding behind
 * n_keep[s] is written as zeros, the stream's items each a share of it: every element of the n_streams x C x row block is written
 * exactly once, and nothing outside it.  LDS: AACG_TRIM_TILE x C x E bytes and two vectors, static — 2080 bytes a channel of float.
 *
 * Written against devport.h like aacg_pcm_resample.h, and executed lane by lane on the CPU by tests/emu/trim_emu.cpp.
 */
#ifndef AACG_PCM_TRIM_H
#define AACG_PCM_TRIM_H

#include <stddef.h>
#include <stdint.h>

#ifndef AACG_TRIM_HOST_ONLY                              /* (aacg_trim.cpp and aacg_pipe_exit.h's users take the limits, the records and the arithmetic alone) */
#include "devport.h"
#endif

/* X(element type, its name in the kernel's name, channels): C and the element size are compile-time constants of a body, and the HOST
 * picks the body — each is a kernel entry of its own (aacg_pcm_trim_<name>_c<C>, aacg_engine_trim.hip). */
#define AACG_TRIM_BODIES(X) \
    X(float, f32, 1) X(float, f32, 2) X(float, f32, 3) X(float, f32, 4) X(float, f32, 5) X(float, f32, 6) X(float, f32, 7) X(float, f32, 8) \
    X(int16_t, i16, 1) X(int16_t, i16, 2) X(int16_t, i16, 3) X(int16_t, i16, 4) X(int16_t, i16, 5) X(int16_t, i16, 6) X(int16_t, i16, 7) X(int16_t, i16, 8)

#define AACG_TRIM_THREADS 256
#define AACG_TRIM_MAX_BLOCKS 4096
#define AACG_TRIM_TILE 512                 /* samples of an item; x E a multiple of 16 bytes, so a planar row's tiles begin aligned */
#define AACG_TRIM_LDS_BYTES(C, E) (AACG_TRIM_TILE * (C) * (E) + 32)
#define AACG_TRIM_LIMIT (1ull << 40)       /* skip and a finite keep are below it */
#define AACG_TRIM_KEEP_ALL UINT64_MAX      /* AACG_TRIM_ALL of include/aacgpu.h */

/* one stream of a launch; travels up in the lane's staging block behind the concealment's records */
typedef struct aacg_trim_stream {
    uint32_t src_first;        /* the stream's first kept sample in the launch's source, in samples per channel                */
    uint32_t n_keep;           /* samples per channel this launch keeps for the stream (0: none)                               */
    uint32_t out_first;        /* packed layout: the stream's first output sample (the sum of n_keep of the streams before it) */
    uint32_t item_first;       /* the stream's first item: ceil(n_keep / tile) items each — planar: at least one —, ascending  */
} aacg_trim_stream;

/* what one launch trims */
typedef struct aacg_trim_args {
    const void* src;           /* packed PCM, [sample][C] elements, 16-byte aligned                                            */
    void*       dst;           /* packed [sum n_keep][C] or planar [n_streams][C][row] elements, 16-byte aligned               */
    const aacg_trim_stream* rec;          /* n_streams records                                                                 */
    uint64_t src_elems;        /* the extent of the source in elements: no load reaches behind it                              */
    uint32_t n_streams, n_items;
    uint32_t row;              /* 0: packed; else planar, elements per row (stride_frames x 1024 >= every n_keep)              */
    uint32_t channels;         /* 1..8   } which body the host launches (AACG_TRIM_BODIES); a body does not read them          */
    uint32_t elem;             /* 4 or 2 }                                                                                    */
} aacg_trim_args;

/* the rule: of the n_in samples a stream brings at position Q, the window (skip, keep) keeps n_keep beginning at the first-th.  keep ==
 * AACG_TRIM_KEEP_ALL: no end.  (Q + n_in does not wrap: Q advances by at most 2^31 a batch from 0) */
static inline void aacg_trim_span(uint64_t Q, uint64_t skip, uint64_t keep, uint32_t n_in, uint32_t* first, uint32_t* n_keep)
{
    const uint64_t end = keep == AACG_TRIM_KEEP_ALL || skip + keep < skip ? UINT64_MAX : skip + keep;
    const uint64_t lo = Q > skip ? Q : skip, top = Q + n_in < Q ? UINT64_MAX : Q + n_in, hi = top < end ? top : end;
    *n_keep = hi > lo ? (uint32_t)(hi - lo) : 0u;
    *first = hi > lo ? (uint32_t)(lo - Q) : 0u;
}
/* 0 if (skip, keep) is a window the stage takes */
static inline int aacg_trim_check(uint64_t skip, uint64_t keep) { return skip >= AACG_TRIM_LIMIT || (keep != AACG_TRIM_KEEP_ALL && keep >= AACG_TRIM_LIMIT); }
#define AACG_TRIM_ITEMS(n_keep, planar) ((n_keep) ? ((n_keep) + AACG_TRIM_TILE - 1u) / AACG_TRIM_TILE : (planar) ? 1u : 0u)      /* (a macro: host and device code share it) */
static inline uint32_t aacg_trim_items(uint32_t n_keep, int planar) { return AACG_TRIM_ITEMS(n_keep, planar); }

#ifndef AACG_TRIM_HOST_ONLY
namespace aacg_pipe {

/* an element as the bits it is: nothing is computed, so a float travels as a word */
template <int E> struct trim_bits;
template <> struct trim_bits<4> { typedef uint32_t type; };
template <> struct trim_bits<2> { typedef uint16_t type; };

/* the 16 / E elements x[0], x[step], x[2 step], ... as one vector, x aligned to an element */
template <typename U>
DP_DEVICE dpi4 trim_gather(const U* x, uint32_t step)
{
    dpi4 w;
    if constexpr (sizeof(U) == 4) {
        w.x = (int)x[0]; w.y = (int)x[step]; w.z = (int)x[2u * step]; w.w = (int)x[3u * step];
    } else {
        w.x = (int)((uint32_t)x[0] | ((uint32_t)x[step] << 16));             w.y = (int)((uint32_t)x[2u * step] | ((uint32_t)x[3u * step] << 16));
        w.z = (int)((uint32_t)x[4u * step] | ((uint32_t)x[5u * step] << 16)); w.w = (int)((uint32_t)x[6u * step] | ((uint32_t)x[7u * step] << 16));
    }
    return w;
}

/* Workgroup b of `blocks`: items b, b + blocks, ... of the batch. */
template <typename ELEM, int C>
DP_DEVICE void trim_body(const aacg_trim_args& A, uint32_t blocks)
{
    static_assert((sizeof(ELEM) == 4 || sizeof(ELEM) == 2) && C >= 1 && C <= 8, "f32 or int16 PCM of 1..8 channels");
    typedef typename trim_bits<(int)sizeof(ELEM)>::type U;
    constexpr uint32_t E = (uint32_t)sizeof(ELEM), V = 16u / E, TILE = AACG_TRIM_TILE;
    unsigned char* const lds = dp_lds_fixed<AACG_TRIM_LDS_BYTES(C, (int)sizeof(ELEM))>();
    const uint32_t tid = (uint32_t)dp_tid();
    const uint64_t src_bytes = A.src_elems * E;
    dpi4 zero; zero.x = zero.y = zero.z = zero.w = 0;
    for (uint32_t it = (uint32_t)dp_block(); it < A.n_items; it += blocks) {
        /* the item's stream: the last record that begins at or before it (a stream without items shares its item_first with the next
         * one, which the search prefers) */
        uint32_t s = 0;
        for (uint32_t hi = A.n_streams; hi - s > 1u;) { const uint32_t mid = (s + hi) >> 1; if (A.rec[mid].item_first <= it) s = mid; else hi = mid; }
        const aacg_trim_stream R = A.rec[s];
        const uint32_t t = it - R.item_first, s0 = t * TILE;
        const uint32_t cnt = R.n_keep - s0 < TILE ? R.n_keep - s0 : TILE;      /* (0 for the one item of a planar stream that keeps nothing) */
        const uint32_t ne = cnt * C;
        /* the item's source bytes into LDS as they lie, in aligned vectors: its first element at the source's residue */
        const uint64_t sb = ((uint64_t)R.src_first + s0) * C * E;
        const uint32_t head = (uint32_t)(sb & 15u);
        if (ne) {
            const uint64_t a0 = sb - head;
            const uint32_t nv = (head + ne * E + 15u) >> 4;
            for (uint32_t v = tid; v < nv; v += AACG_TRIM_THREADS) {
                const uint64_t at = a0 + 16u * (uint64_t)v;
                if (at + 16u <= src_bytes) ((dpi4*)lds)[v] = dp_load_nt((const dpi4*)((const unsigned char*)A.src + at));
                else for (uint64_t b = at; b < src_bytes; b += E) *(U*)(lds + (size_t)(b - a0)) = *(const U*)((const unsigned char*)A.src + b);      /* the extent's last, partial vector */
            }
        }
        dp_block_sync();
        const U* const x = (const U*)(lds + head);       /* x[e]: element e of the item */
        if (!A.row) {
            /* packed: element stores up to the destination's first aligned granule, whole vectors, element stores behind the last */
            U* const d = (U*)A.dst + ((size_t)R.out_first + s0) * C;
            const uint32_t mis = (uint32_t)((uintptr_t)d & 15u), to = ((16u - mis) & 15u) / E;
            const uint32_t h0 = to < ne ? to : ne, nvec = (ne - h0) / V, t0 = h0 + nvec * V;
            for (uint32_t e = tid; e < h0; e += AACG_TRIM_THREADS) d[e] = x[e];
            for (uint32_t v = tid; v < nvec; v += AACG_TRIM_THREADS) dp_store_nt((dpi4*)(d + h0 + v * V), trim_gather<U>(x + h0 + v * V, 1u));
            for (uint32_t e = t0 + tid; e < ne; e += AACG_TRIM_THREADS) d[e] = x[e];
        } else {
            /* planar: every channel's row of the tile, which begins aligned; then this item's share of the zeros behind n_keep */
            const uint32_t items = AACG_TRIM_ITEMS(R.n_keep, 1), nvec = cnt / V;
            const uint32_t p0 = (R.n_keep + V - 1u) & ~(V - 1u), zvec = (A.row - p0) / V, share = (zvec + items - 1u) / items;
            const uint32_t lo = t * share < zvec ? t * share : zvec, hi = zvec - lo < share ? zvec : lo + share;
            for (uint32_t c = 0; c < (uint32_t)C; c++) {
                U* const r = (U*)A.dst + ((size_t)s * C + c) * A.row;
                for (uint32_t v = tid; v < nvec; v += AACG_TRIM_THREADS) dp_store_nt((dpi4*)(r + s0 + v * V), trim_gather<U>(x + (size_t)v * V * C + c, (uint32_t)C));
                for (uint32_t e = nvec * V + tid; e < cnt; e += AACG_TRIM_THREADS) r[s0 + e] = x[(size_t)e * C + c];
                if (t + 1u == items) for (uint32_t e = R.n_keep + tid; e < p0; e += AACG_TRIM_THREADS) r[e] = (U)0;      /* up to the next granule: the item with the row's last samples */
                for (uint32_t v = lo + tid; v < hi; v += AACG_TRIM_THREADS) dp_store_nt((dpi4*)(r + p0 + v * V), zero);
            }
        }
        dp_block_sync();                                                  /* the next item of this workgroup overwrites the LDS */
    }
}

}  // namespace aacg_pipe
#endif

#endif
