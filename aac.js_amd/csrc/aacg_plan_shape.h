/*
 * aacg_plan_shape.h — a resident batch's plan shaped on the device: everything of a plan that depends on the batch's shape (which
 * stream slots bring how many frames of which element layout) written by ONE launch (aacg_plan_shape, aacg_engine_shape.hip) from
 * a per-stream table of O(streams) bytes, into buffers made once (aacg_plan_create_shaped, include/aacgpu.h).
 *
 * What the host planner makes for such a batch — aacg_pipe::plan_list's unit records through aacg_plan_build (aacg_plan.cpp) — is
 * a pure function of the shape and of the engine's overlap-buffer rotation per channel.  shape_body writes the same bytes:
 *   - the refresh map (what aacg_pipe::map_body writes),
 *   - the unit records' planner part (aacg_dev_unit; aacg_units_refresh merges the parser's part behind it),
 *   - the rendezvous cut of the run table (aacg_run) and its link records (aacg_rv_link), in the XCD-aware block order and with the
 *     per-wave words of aacg_plan_fill_run_waves.
 * The host planner orders chains by (slot, channel) while a batch lists slots in any order: the host puts each stream's first
 * run and first link in that order into the table (aacg_shape_plan, aacg_shape.cpp: prefix sums over the streams sorted by slot),
 * so the kernel sorts nothing.
 *
 * Written against devport.h like aacg_parse.h and aacg_pipe_map.h, and executed lane by lane on the CPU by tests/emu/shape_emu.cpp.
 */
#ifndef AACG_PLAN_SHAPE_H
#define AACG_PLAN_SHAPE_H

#include "aacg_pipe_map.h"
#include "aacg_device.h"

#define AACG_SHAPE_THREADS 64

/* aacg_shape_stream (include/aacgpu.h): one stream of a batch, as the device shapes it.  Chain e of the stream is element e < kept
 * at channel nch[0] + ... + nch[e - 1]; its frame f is plan unit unit_first + f * kept + e; it has ceil(frames / 16) runs and one
 * link fewer; run j holds frames 16 j ... and is run run_first + e * runs + j of the plan in generation order, its link towards
 * run j + 1 is link_first + e * (runs - 1) + j. */
static_assert(sizeof(aacg_shape_stream) == 48 && AACG_OV_BUFFERS <= 16 && AACG_RUN_W == 16, "aacg_shape_stream: 4 bits of rotation per channel, runs of 16");

/* what one launch shapes */
typedef struct aacg_shape_args {
    const aacg_shape_stream* tab;
    uint32_t n_streams;
    uint32_t U, C, Cp;         /* the parser's elements per frame; the PCM's channels (the engine's max_channels); the parser's block stride */
    uint32_t n_runs;           /* runs of the whole plan (the block order is a function of it)                                   */
    uint32_t unit0_coef;       /* plan unit 0's coefficient / band-word block and channels: what a wave without work loads       */
    uint32_t unit0_nch;
    uint32_t reserved;
    aacg_refresh_map* map;     /* [n_units]                                                                                      */
    aacg_dev_unit*    units;   /* [n_units]                                                                                      */
    aacg_run*         runs;    /* [n_runs], block order                                                                          */
    aacg_rv_link*     links;   /* [n_runs], same order                                                                           */
} aacg_shape_args;

namespace aacg_pipe {

/* the block of generation index i among R runs: column x = block % 8 holds (R - 1 - x) / 8 + 1 consecutive generation indices
 * (aacg_plan_build: runs_rv[s * 8 + x] = gen_rv[i++]) */
DP_DEVICE uint32_t shape_block_of(uint32_t i, uint32_t R)
{
    const uint32_t q = R >> 3, r = R & 7u, big = r * (q + 1u);
    const uint32_t x = i < big ? i / (q + 1u) : r + (i - big) / q;       /* (i >= big implies q > 0: i < R = big + (8 - r) q) */
    const uint32_t first = x * q + (x < r ? x : r);
    return (i - first) * 8u + x;
}

/* element e's channels and first channel from the table's word of 2-bit counts (no indexed arrays: they would live in scratch) */
DP_DEVICE uint32_t shape_nch(uint32_t word, uint32_t e) { return (word >> (2u * e)) & 3u; }
DP_DEVICE uint32_t shape_chan(uint32_t word, uint32_t e)
{
    const uint32_t below = word & ((1u << (2u * e)) - 1u);
    return (uint32_t)__builtin_popcount(below & 0x5555u) + 2u * (uint32_t)__builtin_popcount(below & 0xaaaau);
}

/* Workgroup b of `blocks` shapes streams b, b + blocks, ...: the stream's map entries and unit records, one lane per unit; its run
 * and link records, one lane per (run, wave). */
DP_DEVICE void shape_body(const aacg_shape_args& A, uint32_t blocks)
{
    for (uint32_t s = (uint32_t)dp_block(); s < A.n_streams; s += blocks) {
        const aacg_shape_stream t = A.tab[s];
        const uint32_t kept = (t.frame_units >> 8) & 0xffu;
        if (!kept) continue;
        const uint32_t F = t.frames;
        const uint32_t n = F * kept;
        for (uint32_t j = (uint32_t)dp_tid(); j < n; j += AACG_SHAPE_THREADS) {
            const uint32_t f = j / kept, e = j - f * kept, i = t.frame_first + f;
            const uint32_t chan = shape_chan(t.nch, e), nch = shape_nch(t.nch, e);
            aacg_refresh_map m;
            m.parsed_index = i * A.U + e;
            m.frame_units = t.frame_units;
            A.map[t.unit_first + j] = m;
            aacg_dev_unit u;
            memset(&u, 0, sizeof u);
            u.d.stream = t.slot; u.d.pcm_offset = i * 1024u * A.C; u.d.channel = (uint16_t)chan; u.d.n_out_ch = (uint16_t)A.C;
            u.d.n_ch = (uint8_t)nch;
            u.d.coef_offset = u.d.meta_offset = i * A.Cp + chan;
            for (uint32_t c = 0; c < 2; c++) if (c < nch) { u.d.ch[c].group_count = 1; u.d.ch[c].group_len[0] = 1; }
            A.units[t.unit_first + j] = u;
        }
        const uint32_t nr = (F + AACG_RUN_W - 1u) / AACG_RUN_W, cells = kept * nr * AACG_RUN_W;
        for (uint32_t idx = (uint32_t)dp_tid(); idx < cells; idx += AACG_SHAPE_THREADS) {
            const uint32_t w = idx % AACG_RUN_W, rj = idx / AACG_RUN_W, e = rj / nr, j = rj - e * nr;
            const uint32_t chan = shape_chan(t.nch, e), nch = shape_nch(t.nch, e);
            const uint32_t first = j * AACG_RUN_W, n_units = F - first < AACG_RUN_W ? F - first : AACG_RUN_W;
            const uint32_t unit0 = t.unit_first + first * kept + e;                  /* the run's first frame's unit */
            const uint32_t b = shape_block_of(t.run_first + e * nr + j, A.n_runs);
            aacg_run* r = A.runs + b;
            const bool work = w < n_units;
            r->unit[w] = work ? (int32_t)(unit0 + w * kept) : -1;
            r->wave_unit[w] = work ? (int32_t)(unit0 + w * kept) : 0;
            r->wave_coef[w] = r->wave_meta[w] = work ? (t.frame_first + first + w) * A.Cp + chan : A.unit0_coef;
            if (w) continue;
            const bool more = j + 1u < nr;
            uint32_t wave_nch = 0;
            for (uint32_t k = 0; k < AACG_RUN_W; k++) wave_nch |= ((k < n_units ? nch : A.unit0_nch) & 3u) << (2 * k);
            r->pred_unit = -1; r->n_units = (int32_t)n_units; r->is_last = more ? 0 : 1; r->wave_nch = wave_nch;
            for (uint32_t c = 0; c < 2; c++) {
                const uint32_t chn = chan + (c < nch ? c : 0u);
                r->ov0[c] = (int32_t)(((t.slot * A.C + chn) * (uint32_t)AACG_OV_BUFFERS) * 1024u);
                r->rot[c] = (int32_t)((t.rot >> (4 * chn)) & 15u);
            }
            const uint32_t link0 = t.link_first + e * (nr - 1u);
            aacg_rv_link lk;
            lk.link_in = j ? (int32_t)(link0 + j - 1u) : -1;
            lk.link_out = more ? (int32_t)(link0 + j) : -1;
            lk.succ_unit = more ? (int32_t)(unit0 + AACG_RUN_W * kept) : -1;
            lk.reserved = 0;
            A.links[b] = lk;
        }
    }
}

/* The table's caller part for a batch (lay[s], slots[s], frames_of[s] as aacg_pipe::plan_list takes them): everything but
 * run_first, link_first and rot, which aacg_shape_plan adds.  Returns the number of plan units. */
inline uint32_t shape_table(const aacg_pipe_layout* lay, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, aacg_shape_stream* table)
{
    uint32_t first = 0, n_units = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        const aacg_pipe_layout& L = lay[s];
        aacg_shape_stream t;
        memset(&t, 0, sizeof t);
        t.frame_first = first; t.frames = frames_of[s]; t.unit_first = n_units; t.frame_units = (uint32_t)L.n | ((uint32_t)L.kept << 8);
        t.slot = slots[s];
        for (uint32_t e = 0; e < 8 && e < L.n; e++) t.nch |= ((uint32_t)L.nch[e] & 3u) << (2 * e);
        table[s] = t;
        first += frames_of[s];
        n_units += frames_of[s] * L.kept;
    }
    return n_units;
}

}  // namespace aacg_pipe

#include <string>
#include "aacg_host.h"

/* ---- the host's part (aacg_shape.cpp, plain C++: the engine calls it, tests/emu/shape_emu.cpp links it) ------------------------------- */
/* what a shaped plan's buffers hold at most */
struct aacg_shape_limits {
    uint32_t max_streams;      /* streams of a batch                                                                     */
    uint32_t max_frames;       /* frames of one stream in a batch                                                        */
    uint32_t max_elems;        /* elements of a frame that are decoded (kept), at most                                   */
    size_t   max_units, max_runs, max_links;
};
/* the most units, runs and links a batch within (max_streams, max_frames, max_elems) can have on an engine of `channels` channels:
 * max_streams x min(max_elems, channels) chains of ceil(max_frames / 16) runs, one link fewer per chain */
aacg_shape_limits aacg_shape_capacity(uint32_t max_streams, uint32_t max_frames, uint32_t max_elems, uint32_t channels);

/* what launch_run and the engine's bookkeeping take from aacg_plan_host for a kept plan, for one shape */
struct aacg_shape_info {
    uint32_t n_units = 0, n_runs = 0, n_links = 0;
    bool     zero_fill = false;    /* some kept layout does not cover all output channels */
    bool     wide_frames = false, long_chains = false;
    size_t   pcm_floats = 0;
    uint32_t unit0_coef = 0, unit0_nch = 0;
    std::vector<aacg_chain> chains;    /* by (slot, channel): what a launch advances (parity_advance); first_run / n_runs: the rendezvous cut's */
};
/* Completes a batch's table (run_first, link_first, rot from `parity`: [slots x channels], the engine's) and derives the shape's
 * figures.  The table's caller part is checked against the limits and for consistency (prefix sums, layouts that fit the channels,
 * every slot once, slot < n_slots) — the kernel trusts it: AACG_ERR_CAPACITY / AACG_ERR_INVALID_ARG with a text, and then neither
 * the table nor *out has been touched. */
int aacg_shape_plan(aacg_shape_stream* table, uint32_t n_streams, uint32_t n_slots, uint32_t channels, uint32_t Cp, const uint8_t* parity,
                    const aacg_shape_limits& lim, aacg_shape_info* out, std::string* err);
/* The sequence rule of shaped launches: a launch continues its predecessor through the cross-launch cells only if the two were
 * shaped from identical tables — the same slots in the same order with the same counts and layouts; the rotation words, which
 * move on with every launch, apart. */
bool aacg_shape_same(const aacg_shape_stream* a, size_t na, const aacg_shape_stream* b, size_t nb);

#endif
