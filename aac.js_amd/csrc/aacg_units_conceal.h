/*
 * aacg_units_conceal.h — refused frames concealed on the device: a frame the parser or the refresh refused repeats its stream's last
 * good frame with a fade, by SUBSTITUTING RECORDS in front of the transform.  ONE launch per batch (aacg_units_conceal,
 * aacg_engine_conceal.hip) behind aacg_units_refresh on the same stream and in front of aacg_units_carry_shape
 * (aacg_plan_conceal_refused, include/aacgpu.h, which states the rule; tests/conceal_kit.py states it in numpy).  No run kernel knows
 * of it: what the transform produces is what it would produce for a stream that held the substituted frame.
 *
 * The state.  Per stream slot TWO sides of AACG_CONCEAL_SIDE_BYTES(Cp) bytes:
 *     [aacg_conceal_head: has, r][8 x aacg_conceal_elem: flags, ch[0..1] of G's elements][Cp x (1024 int16 | 120 band words)]
 * A stream's record of the batch (aacg_conceal_stream) says which side the launch READS (bit 0 of `state`) — it always writes the
 * other — and whether the slot is fresh (bit 1: the side it would read counts as empty).
 *
 * One wave per (stream, frame, parser channel block c < Cp): job j of n_streams x longest x Cp, a grid-stride walk.  A wave whose
 * frame the stream does not bring, or whose block no kept element owns, leaves at once.  Everything that decides a wave's path is
 * wave-uniform (the stream's record, the statuses, the state's head).
 *   - A GOOD frame (status OK) looks FORWARD over its stream's later statuses, 64 frames a look, the lanes side by side (dp_any).
 *     One behind it is good: the wave leaves — on a clean feed that is its one look.  None is: it is the stream's last good frame
 *     and writes G — its block into the side the launch writes, the element that owns the block its record (the element's first
 *     block), block 0 the head (has = 1, r = min(frames behind it, hold + 1)).
 *   - A REFUSED frame looks BACK, the lanes over the frames before it, nearest first (dp_wave_first): d = the distance to the
 *     nearest good frame, no further than it matters — `hold` frames, or, for the stream's LAST frame, the whole batch.
 *       d found:      r = d; d <= hold: concealed from that frame's records and blocks, which this launch never writes.
 *       none (f < hold or the last frame): the batch's frames up to this one are all refused; r = r_old + f + 1; concealed from the
 *                     side the launch reads iff that holds a G and r <= hold.
 *     The stream's last frame, with no good frame in the whole batch, also CARRIES the state over: the old G (if any) into the side
 *     the launch writes, with r = min(r_old + frames, hold + 1).
 *     Concealing: the wave's block takes G's 1024 values and 120 words, the words of band types 1..11 with the scalefactor field
 *     lowered by r x fade_steps and kept at 0 or above; the element's first block rewrites the plan unit's flags, ch[0..1] and the
 *     group map derived from them (what the refresh derives); block 0 sets AACG_PARSE_CONCEALED in the frame's result flags.
 * A job moves 2048 + 240 bytes as 16-byte vector loads and stores — two per lane and one for lanes 0..14 — and rewrites the words in
 * registers.  Every learnt stream of a batch has exactly ONE frame that writes the state: its last good frame, or else its last frame.
 *
 * Two hazards:
 *   - READ AND WRITE OF A SLOT'S STATE IN ONE LAUNCH.  Leading refused frames read G while the stream's last good frame replaces it:
 *     two sides, as the resampler's history has them.  The host advances the parity when the batch has been enqueued.  A launch
 *     reads: statuses (never written; the result's flags byte is another byte), records and blocks of GOOD frames (it writes those of
 *     refused frames only) and the side `parity`; it writes the side `parity ^ 1`.  No launch reads a byte it writes, so no order
 *     between its waves is needed and none is assumed.
 *   - ORDER ACROSS LANES.  Batch k + 1's launch runs on another lane's stream and reads the side batch k's wrote: the engine records
 *     an event behind every launch and puts the next launch's stream behind it — behind that lane's own parse and refresh, so the
 *     parses of consecutive batches still run side by side (as the carry's: aacg_shape_carry.h).
 * The same batch twice — plan mode 0's retry of a stale plan — is NOT served: the stage requires a shaped plan, whose set is never stale.
 *
 * Written against devport.h like aacg_shape_carry.h, and executed lane by lane on the CPU by tests/emu/conceal_emu.cpp.
 */
#ifndef AACG_UNITS_CONCEAL_H
#define AACG_UNITS_CONCEAL_H

#include "devport.h"
#include "aacg_pipe_map.h"
#include "aacg_device.h"

#define AACG_CONCEAL_THREADS 256
#define AACG_CONCEAL_WAVES (AACG_CONCEAL_THREADS / 64)
#define AACG_CONCEAL_MAX_BLOCKS 2048

typedef struct aacg_conceal_head { uint32_t has, r, reserved[2]; } aacg_conceal_head;
typedef struct aacg_conceal_elem { uint32_t flags, reserved[3]; aacg_chan_info ch[2]; } aacg_conceal_elem;
#define AACG_CONCEAL_BLOCK_BYTES (2048u + (uint32_t)sizeof(aacg_band_meta))
#define AACG_CONCEAL_ELEMS_AT    ((uint32_t)sizeof(aacg_conceal_head))
#define AACG_CONCEAL_BLOCKS_AT   (AACG_CONCEAL_ELEMS_AT + 8u * (uint32_t)sizeof(aacg_conceal_elem))
#define AACG_CONCEAL_SIDE_BYTES(Cp) (AACG_CONCEAL_BLOCKS_AT + (Cp) * AACG_CONCEAL_BLOCK_BYTES)
static_assert(sizeof(aacg_conceal_head) == 16 && sizeof(aacg_conceal_elem) == 48 && sizeof(aacg_band_meta) == 240 && sizeof(aacg_conceal_stream) == 32,
              "the conceal state is walked in 16-byte vectors");

/* what one launch conceals */
typedef struct aacg_conceal_args {
    aacg_dev_unit*             units;     /* [n_units]: the set's refreshed records                                                 */
    aacg_parse_result*         results;   /* [frames]: status read, flags written (AACG_PARSE_CONCEALED)                             */
    int16_t*                   q;         /* the lane's spectrum blocks, 1024 values each                                           */
    aacg_band_meta*            meta;      /* ... and band-word blocks                                                               */
    const aacg_conceal_stream* tab;       /* [n_streams]                                                                            */
    unsigned char*             state;     /* [n_slots][2][AACG_CONCEAL_SIDE_BYTES(Cp)], 16-byte aligned                              */
    uint32_t n_streams, longest;          /* the batch's streams, the largest frame count among them                                */
    uint32_t Cp, n_slots;                 /* the parser's block stride (1..8); the state's slots                                    */
    uint32_t fade_steps, hold_frames;     /* 0..64, 1..255                                                                          */
} aacg_conceal_args;

namespace aacg_pipe {

DP_DEVICE uint32_t conceal_nch(uint32_t word, uint32_t e) { return (word >> (2u * e)) & 3u; }
DP_DEVICE uint32_t conceal_chan(uint32_t word, uint32_t e)
{
    const uint32_t below = word & ((1u << (2u * e)) - 1u);
    return (uint32_t)__builtin_popcount(below & 0x5555u) + 2u * (uint32_t)__builtin_popcount(below & 0xaaaau);
}
DP_DEVICE uint32_t conceal_status(const aacg_parse_result* results, uint32_t i) { return ((const volatile uint8_t*)(results + i))[0]; }
/* one band word behind r x fade_steps steps of fade: band types 1..11 only, the field kept at 0 or above */
DP_DEVICE uint32_t conceal_fade_word(uint32_t w, uint32_t down)
{
    const uint32_t bt = (w >> AACG_META_BT_SHIFT) & 15u, sf = w & AACG_META_SF_MASK;
    if (bt < 1u || bt > 11u) return w;
    return (w & ~(uint32_t)AACG_META_SF_MASK) | (sf > down ? sf - down : 0u);
}
DP_DEVICE uint32_t conceal_fade_pair(uint32_t v, uint32_t down) { return conceal_fade_word(v & 0xffffu, down) | (conceal_fade_word(v >> 16, down) << 16); }
/* a channel's aacg_chan_info as two 64-bit words (window_sequence: byte 0, group_count: byte 4; group_len: the second word), and the
 * group-of-window map the refresh derives from its grouping (aacg_units_refresh.h) — shifts, no indexed bytes */
DP_DEVICE uint32_t conceal_gmap(dp_u64 lo, dp_u64 hi)
{
    const uint32_t count = (uint32_t)(lo >> 32) & 0xffu;
    uint32_t gmap = 0, w = 0;
    for (uint32_t g = 0; g < 8u; g++) {
        const uint32_t len = g < count ? (uint32_t)(hi >> (8u * g)) & 0xffu : 0u;
        for (uint32_t k = 0; k < len && w < 8u; k++, w++) gmap |= g << (4u * w);
    }
    return gmap;
}

/* Wave dp_wave() of workgroup dp_block() of `blocks`: jobs (block * waves + wave), then blocks * waves on. */
DP_DEVICE void conceal_body(const aacg_conceal_args& A, uint32_t blocks)
{
    const uint32_t lane = (uint32_t)dp_lane(), per = A.longest * A.Cp, total = A.n_streams * per, hold = A.hold_frames;
    const size_t side_bytes = AACG_CONCEAL_SIDE_BYTES(A.Cp);
    for (uint32_t j = (uint32_t)dp_block() * AACG_CONCEAL_WAVES + (uint32_t)dp_wave(); j < total; j += blocks * AACG_CONCEAL_WAVES) {
        const uint32_t s = j / per, rem = j - s * per, f = rem / A.Cp, c = rem - f * A.Cp;
        const aacg_conceal_stream t = A.tab[s];
        const uint32_t kept = (t.frame_units >> 8) & 0xffu, F = t.frames;
        if (!kept || f >= F || t.slot >= A.n_slots) continue;
        /* the kept element that owns block c, and which of its channels the block is */
        uint32_t e = kept, k = 0;
        for (uint32_t x = 0; x < kept && x < 8u; x++) {
            const uint32_t at = conceal_chan(t.nch, x), n = conceal_nch(t.nch, x);
            if (c >= at && c < at + n) { e = x; k = c - at; }
        }
        if (e == kept) continue;
        const uint32_t i = t.frame_first + f, ui = t.unit_first + f * kept + e;
        unsigned char* const rd = A.state + ((size_t)t.slot * 2u + (t.state & 1u)) * side_bytes;
        unsigned char* const wr = A.state + ((size_t)t.slot * 2u + ((t.state & 1u) ^ 1u)) * side_bytes;
        const bool good = conceal_status(A.results, i) == AACG_PARSE_OK;

        const unsigned char *src_q = nullptr, *src_m = nullptr;      /* where the block comes from */
        const aacg_conceal_elem* src_el = nullptr;                   /* ... and the element's record, from the state */
        const aacg_dev_unit* src_u = nullptr;                        /* ... or from a good frame of the batch */
        bool to_state = false, to_frame = false;
        uint32_t head_has = 0, head_r = 0, r = 0;
        if (good) {
            bool later = false;
            for (uint32_t base = f + 1u; base < F && !later; base += 64u) {
                const uint32_t g = base + lane;
                later = dp_any(g < F && conceal_status(A.results, t.frame_first + g) == AACG_PARSE_OK);
            }
            if (later) continue;
            src_u = A.units + ui;
            to_state = true; head_has = 1u; head_r = F - 1u - f < hold + 1u ? F - 1u - f : hold + 1u;
        } else {
            const bool last = f + 1u == F;
            const uint32_t reach = last || f < hold ? f : hold;      /* how far back a good frame matters */
            uint32_t d = 0;
            for (uint32_t base = 1u; base <= reach && !d; base += 64u) {
                const uint32_t dist = base + lane;
                const uint32_t l = dp_wave_first(dist <= reach && conceal_status(A.results, i - dist) == AACG_PARSE_OK);
                if (l < 64u) d = base + l;
            }
            if (d) {
                if (d > hold) continue;
                r = d; src_u = A.units + (ui - d * kept); to_frame = true;
            } else {
                if (reach < f) continue;                             /* more than `hold` refused frames in front of it */
                uint32_t has_old = 0, r_old = 0;
                if (!(t.state & 2u)) {                               /* (a fresh slot's side is not read) */
                    const aacg_conceal_head h = *(const aacg_conceal_head*)rd;
                    has_old = (uint32_t)dp_uniform((int)(h.has != 0u));
                    r_old = has_old ? (uint32_t)dp_uniform((int)h.r) : 0u;
                }
                r = r_old + f + 1u;
                to_frame = has_old && r <= hold;
                if (last) { to_state = true; head_has = has_old; head_r = has_old ? (r_old + F < hold + 1u ? r_old + F : hold + 1u) : 0u; }
                if (!to_frame && !to_state) continue;
                if (has_old) { src_q = rd + AACG_CONCEAL_BLOCKS_AT + (size_t)c * AACG_CONCEAL_BLOCK_BYTES; src_m = src_q + 2048; src_el = (const aacg_conceal_elem*)(rd + AACG_CONCEAL_ELEMS_AT) + e; }
            }
        }
        if (src_u) {
            src_q = (const unsigned char*)(A.q + ((size_t)src_u->d.coef_offset + k) * 1024u);
            src_m = (const unsigned char*)(A.meta + ((size_t)src_u->d.meta_offset + k));
        }
        if (to_state && c == 0u && lane == 0u) { aacg_conceal_head h = {head_has, head_r, {0u, 0u}}; *(aacg_conceal_head*)wr = h; }
        if (!src_q) continue;                                        /* no G anywhere: the head says so, nothing else moves */
        /* the block in registers: 128 vectors of spectrum, two a lane, and 15 of band words */
        const dpi4 q0 = ((const dpi4*)src_q)[lane], q1 = ((const dpi4*)src_q)[64u + lane];
        dpi4 m = {0, 0, 0, 0};
        if (lane < 15u) m = ((const dpi4*)src_m)[lane];
        /* the element's record, by the element's first block: flags and ch[0..1] as four 64-bit words */
        uint32_t el_flags = 0;
        dp_u64 c0lo = 0, c0hi = 0, c1lo = 0, c1hi = 0;
        if (k == 0u && lane == 0u) {
            const dp_u64* const w = (const dp_u64*)(src_u ? (const void*)&src_u->d.ch[0] : (const void*)&src_el->ch[0]);
            el_flags = src_u ? (uint32_t)src_u->d.flags : src_el->flags;
            c0lo = w[0]; c0hi = w[1]; c1lo = w[2]; c1hi = w[3];
        }
        if (to_state) {
            unsigned char* const dq = wr + AACG_CONCEAL_BLOCKS_AT + (size_t)c * AACG_CONCEAL_BLOCK_BYTES;
            ((dpi4*)dq)[lane] = q0; ((dpi4*)dq)[64u + lane] = q1;
            if (lane < 15u) ((dpi4*)(dq + 2048))[lane] = m;
            if (k == 0u && lane == 0u) {
                aacg_conceal_elem* el = (aacg_conceal_elem*)(wr + AACG_CONCEAL_ELEMS_AT) + e;
                dp_u64* const w = (dp_u64*)&el->ch[0];
                el->flags = el_flags; el->reserved[0] = el->reserved[1] = el->reserved[2] = 0u;
                w[0] = c0lo; w[1] = c0hi; w[2] = c1lo; w[3] = c1hi;
            }
        }
        if (to_frame) {
            aacg_dev_unit* const u = A.units + ui;
            const uint32_t down = r * A.fade_steps;
            dpi4 mf;
            mf.x = (int)conceal_fade_pair((uint32_t)m.x, down); mf.y = (int)conceal_fade_pair((uint32_t)m.y, down);
            mf.z = (int)conceal_fade_pair((uint32_t)m.z, down); mf.w = (int)conceal_fade_pair((uint32_t)m.w, down);
            unsigned char* const dq = (unsigned char*)(A.q + ((size_t)u->d.coef_offset + k) * 1024u);
            ((dpi4*)dq)[lane] = q0; ((dpi4*)dq)[64u + lane] = q1;
            if (lane < 15u) ((dpi4*)(A.meta + ((size_t)u->d.meta_offset + k)))[lane] = mf;
            if (k == 0u && lane == 0u) {
                dp_u64* const w = (dp_u64*)&u->d.ch[0];
                const uint32_t n_ch = u->d.n_ch;
                u->d.flags = (uint8_t)el_flags;
                w[0] = c0lo; w[1] = c0hi; w[2] = c1lo; w[3] = c1hi;
                u->gmap[0] = n_ch > 0u && (c0lo & 0xffu) == AACG_EIGHT_SHORT_SEQUENCE ? conceal_gmap(c0lo, c0hi) : 0u;
                u->gmap[1] = n_ch > 1u && (c1lo & 0xffu) == AACG_EIGHT_SHORT_SEQUENCE ? conceal_gmap(c1lo, c1hi) : 0u;
            }
            if (c == 0u && lane == 0u) ((volatile uint8_t*)(A.results + i))[__builtin_offsetof(aacg_parse_result, flags)] |= AACG_PARSE_CONCEALED;
        }
    }
}

}  // namespace aacg_pipe

#endif
