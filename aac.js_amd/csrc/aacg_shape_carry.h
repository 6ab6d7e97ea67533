/*
 * aacg_shape_carry.h — each channel's window shape carried from frame to frame on the device: the first half of a frame is windowed
 * with the PREVIOUS frame's shape (aacg_chan_info.window_shape_prev, which the run kernels honour: unit_view.shape_prev), and on the
 * resident route nobody on the host ever sees a frame's shape.  ONE small launch per batch (aacg_units_carry_shape,
 * aacg_engine_carry.hip) behind aacg_units_refresh on the same stream, when the refreshed shapes are final
 * (aacg_plan_carry_window_shape, include/aacgpu.h).
 *
 * The rule.  The engine holds W[slot][c] in {0, 1} for every stream slot and output channel c < max_channels, 0 at create and after
 * aacg_reset_stream.  Take a stream's frames of the batch in order, f = 0 .. n - 1; for each plan unit of frame f and each of its
 * channels k < n_ch, with c = unit.channel + k:
 *     unit.ch[k].window_shape_prev = f == 0 ? W[slot][c] : shape(f - 1, c),          and after the batch  W[slot][c] = shape(n - 1, c),
 * where shape(f, c) is ch[k].window_shape of the REFRESHED record: a frame the refresh made silent has shape 0 and the frame behind
 * it starts from sine.  A channel without a unit in the batch keeps its W.  No other byte of a unit record changes.
 *
 * One lane per plan unit, no walk: a resident plan lists a stream's frames one behind the other and a frame's units next to each
 * other, so the unit of the same (stream, channel) one frame earlier is `kept` records back (aacg_refresh_map.frame_units bits
 * 8..15, or 0 = all of bits 0..7) and the one a frame later `kept` records on; a lane looks whether they are there (same stream,
 * channel and channel count).  A lane without predecessor reads W, a lane without successor writes it.  A lane writes only its own
 * window_shape_prev bytes and reads only window_shape bytes of others, which this launch never writes.  Plain vector loads and
 * stores and byte writes into the record; no LDS, no wave layout: one lane's work is a dozen loads and two byte stores.
 *
 * Two hazards:
 *   - THE SAME BATCH TWICE.  In plan mode 0 aacg_pipeline_submit_ragged refreshes a batch a second time when aacg_decode_pipelined
 *     answers AACG_ERR_STALE_PLAN; a second carry must not start from the end state the first one wrote.  A W entry is therefore
 *     one 32-bit word (before | after << 1 | batch serial << 2): the state the batch that wrote it STARTED from, the state it left,
 *     and which batch that was.  A launch with the entry's own serial starts again from `before`, any other from `after`; a launch
 *     writes (what it started from, its last frame's shape, its serial).  So a launch is idempotent per serial, and the stream's
 *     first and last lane, which both read the entry while the last one writes it, derive the same start whichever comes first.
 *     The engine gives a carry the serial of its predecessor as long as no launch has taken the records in between; the host
 *     writes entries with serial 0 (create, reset, aacg_set_window_shape), which no launch carries.
 *   - ORDER ACROSS LANES.  Batch k + 1's carry runs on another lane's stream and must read what batch k's wrote: the engine records
 *     an event behind every carry launch and puts the next carry's stream behind it — a wait placed behind that lane's own parse and
 *     refresh, so that the parses of consecutive batches still run side by side (the transforms of consecutive batches are ordered
 *     through the cross-launch cells anyway).
 *
 * Written against devport.h like aacg_pipe_map.h and aacg_plan_shape.h, and executed lane by lane on the CPU by tests/emu/carry_emu.cpp.
 */
#ifndef AACG_SHAPE_CARRY_H
#define AACG_SHAPE_CARRY_H

#include "aacg_pipe_map.h"
#include "aacg_device.h"

#define AACG_CARRY_THREADS 256
#define AACG_CARRY_MAX_BLOCKS 1024

/* a W entry (the host writes and reads entries too: aacg_set / aacg_get_window_shape) */
#define AACG_CARRY_SERIAL_MAX 0x3fffffffu
#if defined(__HIPCC__) && !defined(AACG_EMU_BUILD)
#define AACG_CARRY_HD __host__ __device__ __forceinline__
#else
#define AACG_CARRY_HD static inline
#endif
AACG_CARRY_HD uint32_t aacg_carry_word(uint32_t before, uint32_t after, uint32_t serial) { return (before & 1u) | ((after & 1u) << 1) | (serial << 2); }
AACG_CARRY_HD uint32_t aacg_carry_now(uint32_t word) { return (word >> 1) & 1u; }                       /* what the host reads: the state after the batch that wrote it */

/* what one launch carries */
typedef struct aacg_carry_args {
    aacg_dev_unit*          units;     /* [n_units]: the set's refreshed records                                                    */
    const aacg_refresh_map* map;       /* [n_units]: the map they were refreshed through (frame_units: the units of a frame)          */
    uint32_t*               W;         /* [n_slots x C] entries                                                                     */
    uint32_t n_units;
    uint32_t n_slots, C;               /* the engine's max_streams, max_channels                                                    */
    uint32_t serial;                   /* 1 .. AACG_CARRY_SERIAL_MAX                                                                */
} aacg_carry_args;

namespace aacg_pipe {

DP_DEVICE bool carry_same(const aacg_unit_desc& a, uint32_t stream, uint32_t chan, uint32_t nch) { return a.stream == stream && a.channel == chan && a.n_ch == nch; }

/* Workgroup b of `blocks`: units b * AACG_CARRY_THREADS + lane, then `blocks` workgroups on. */
DP_DEVICE void carry_body(const aacg_carry_args& A, uint32_t blocks)
{
    for (uint32_t i = (uint32_t)dp_block() * AACG_CARRY_THREADS + (uint32_t)dp_tid(); i < A.n_units; i += blocks * AACG_CARRY_THREADS) {
        const uint32_t fu = A.map[i].frame_units, kept = (fu >> 8) & 0xffu ? (fu >> 8) & 0xffu : fu & 0xffu;
        aacg_dev_unit* u = A.units + i;
        const uint32_t stream = u->d.stream, chan = u->d.channel, nch = u->d.n_ch;
        if (!kept || stream >= A.n_slots) continue;
        const bool has_pred = i >= kept && carry_same(A.units[i - kept].d, stream, chan, nch);
        const bool has_succ = i + kept < A.n_units && carry_same(A.units[i + kept].d, stream, chan, nch);
        for (uint32_t k = 0; k < 2; k++) {
            if (k >= nch || chan + k >= A.C) continue;
            unsigned* w = (unsigned*)A.W + (size_t)stream * A.C + chan + k;
            uint32_t start = 0;
            if (!has_pred || !has_succ) {
                const uint32_t word = dp_g_load_u32(w);
                start = (word >> 2) == A.serial ? word & 1u : aacg_carry_now(word);
            }
            u->d.ch[k].window_shape_prev = has_pred ? A.units[i - kept].d.ch[k].window_shape : (uint8_t)start;
            if (!has_succ) dp_g_store_u32(w, aacg_carry_word(start, u->d.ch[k].window_shape, A.serial));
        }
    }
}

}  // namespace aacg_pipe

#include <string>

/* ---- the host's part (aacg_shape.cpp; the engine calls it) -------------------------------------------------------------------- */
/* Is this listing one the kernel can carry through: every stream's units in one stretch, frame behind frame (units that share
 * pcm_offset), every frame of a stream the same elements (channel, n_ch) in the same order, at most 8 of them?  false with a text. */
bool aacg_carry_listing_ok(const aacg_unit_desc* units, size_t n_units, std::string* why);

#endif
