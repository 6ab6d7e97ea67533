/*
 * aacg_units_refresh.h — a plan's unit records rewritten on the device from what aacg_parse_device produced: the body of
 * aacg_units_refresh (aacg_engine_refresh.hip; aacg_plan_refresh_from_parse / _ex, include/aacgpu.h).  One lane per plan unit
 * copies what the parser found per frame — window sequence and shape, max_sfb, grouping, flags — from the parser's record into
 * the plan's device record, keeps the planner's part (stream, PCM offset, channel layout, block offsets), derives the
 * group-of-window map, and turns a frame the parser refused into a silent one (ONLY_LONG, max_sfb 0), counting it.
 *
 * The rule, for plan unit i.  Without a map src = i and want = 0; with one src = map[i].parsed_index, want = frame_units & 0xff
 * and listed = (frame_units >> 8) & 0xff, or want where that is 0.  frame = src / max_units, e = src % max_units.
 *     matches(a, p):  n_ch, channel, coef_offset and meta_offset equal, and not (refuse_pns and p has AACG_UNIT_HAS_PNS).
 *     want == 0:      the UNIT is accepted iff results[frame].status is OK, e < results[frame].n_units and matches(units[i], parsed[src]);
 *     want > 0:       the FRAME is accepted iff its status is OK, its n_units == want and matches(units[i - e + k], parsed[src - e + k])
 *                     for every k < listed; a refused frame whose status was OK gets AACG_PARSE_LAYOUT.
 * An accepted unit takes the parser's flags, both ch entries (AACG_CHAN_TNS_PRESENT cleared unless keep_tns), tns_offset with
 * keep_tns and 0 without, and gmap[c] for its EIGHT_SHORT channels c < n_ch; a refused one flags 0, tns_offset 0, gmap 0 and
 * both ch entries zero but group_count = group_len[0] = 1.  *refused grows by one per refused unit (no map) or frame (map).
 * No other byte of a record changes.
 *
 * Written against devport.h like aacg_pipe_map.h, aacg_plan_shape.h and aacg_shape_carry.h, and executed lane by lane on the CPU
 * by tests/emu/refresh_emu.cpp (tests/test_units_refresh_emu.py states the rule in numpy and compares byte for byte).
 */
#ifndef AACG_UNITS_REFRESH_H
#define AACG_UNITS_REFRESH_H

#include "devport.h"
#include "aacg_device.h"

#define AACG_REFRESH_THREADS 256

/* what one launch refreshes */
typedef struct aacg_refresh_args {
    aacg_dev_unit*          units;     /* [n_units]: the set's records, the planner's part valid                                   */
    const aacg_unit_desc*   parsed;    /* [frames x max_units]: the parser's records                                               */
    aacg_parse_result*      results;   /* [frames]; written (OK -> LAYOUT) with a map only                                         */
    const aacg_refresh_map* map;       /* [n_units], or null: plan unit i <- parsed record i, refusal per unit                     */
    uint32_t n_units, max_units;
    int refuse_pns, keep_tns;
    uint32_t* refused;                 /* the caller's counter                                                                     */
} aacg_refresh_args;

namespace aacg_pipe {

DP_DEVICE bool unit_matches(const aacg_unit_desc& have, const aacg_unit_desc& p, int refuse_pns)
{
    /* (the blocks: the plan's run tables carry copies of the offsets, aacg_run.wave_coef — a frame the parser put elsewhere is not
     * the frame the plan was made for) */
    return p.n_ch == have.n_ch && p.channel == have.channel && p.coef_offset == have.coef_offset && p.meta_offset == have.meta_offset &&
           !(refuse_pns && (p.flags & AACG_UNIT_HAS_PNS));              /* AACG_PNS_REFERENCE engines do not decode noise bands */
}

/* Lane dp_tid() of workgroup dp_block(), `threads` lanes a workgroup: unit dp_block() * threads + dp_tid(). */
DP_DEVICE void refresh_body(const aacg_refresh_args& A, uint32_t threads)
{
    aacg_dev_unit* const units = A.units;
    const aacg_unit_desc* const parsed = A.parsed;
    aacg_parse_result* const results = A.results;
    const aacg_refresh_map* const map = A.map;
    const uint32_t max_units = A.max_units;
    const int refuse_pns = A.refuse_pns, keep_tns = A.keep_tns;
    const uint32_t i = (uint32_t)dp_block() * threads + (uint32_t)dp_tid();
    if (i >= A.n_units) return;
    aacg_dev_unit u = units[i];
    /* frame_units: elements the frame must have | elements of them the plan lists << 8 (0: all; aacgpu.h) */
    const uint32_t src = map ? map[i].parsed_index : i, want = map ? (map[i].frame_units & 0xffu) : 0u;
    const uint32_t listed = map && (map[i].frame_units >> 8) ? ((map[i].frame_units >> 8) & 0xffu) : want;
    const aacg_unit_desc p = parsed[src];
    const aacg_parse_result r = results[src / max_units];
    const uint32_t e = src % max_units;
    bool ok = r.status == AACG_PARSE_OK && e < r.n_units && unit_matches(u.d, p, refuse_pns);
    if (want) {
        /* with a map a frame is taken or refused as a whole: every lane of the frame looks at all of its elements (the plan lists
         * them next to each other, in the frame's order) and comes to the same answer; the first one reports it */
        ok = r.status == AACG_PARSE_OK && r.n_units == want;
        /* THE SIBLING READS.  A lane reads, from records and results that OTHER lanes of this launch rewrite at the same time and
         * in no order (a frame's lanes may even sit in two workgroups): n_ch, channel, coef_offset and meta_offset of
         * units[i - e + k].d — its frame's other plan records — and results[frame].status, which the frame's first lane may be
         * turning into LAYOUT.  No order is needed:
         *   - those four fields are the planner's part.  A lane writes its record back whole (units[i] = u below), but these
         *     four with the very values it loaded: whether a sibling sees them before or after that store, it sees equal
         *     values.  What a lane changes in its record (flags, ch, tns_offset, gmap) no sibling reads.
         *   - results[].status only ever goes from OK to LAYOUT in a launch, and only for a frame that is being refused.  A lane
         *     that sees OK comes to the refusal by the same element comparison the first lane made; a lane that already sees
         *     LAYOUT refuses because the status is not OK.  Either way the frame is refused by all of its lanes, and only the
         *     first one (e == 0), which decides on the status IT loaded, counts it and writes the result.  n_units is not written. */
        for (uint32_t k = 0; k < listed && ok; k++) ok = unit_matches(units[i - e + k].d, parsed[src - e + k], refuse_pns);
        if (!ok && e == 0 && r.status == AACG_PARSE_OK) results[src / max_units].status = AACG_PARSE_LAYOUT;
    }
    /* A refused frame's record (and the slots e >= n_units) is unspecified: nothing is taken from it.  Its unit keeps
     * the offsets the planner validated — a silent unit still loads its blocks (quant_load reads unconditionally). */
    u.d.tns_offset = 0;                                  /* (keep_tns: an accepted frame's comes from the parser, below) */
    u.gmap[0] = u.gmap[1] = 0;
    if (ok) {
        u.d.flags = p.flags;
        for (int c = 0; c < 2; c++) {
            u.d.ch[c] = p.ch[c];
            /* no TNS records on this path — unless the plan's launches bring them (keep_tns: aacg_decode_pipelined_stages on an
             * AACG_TNS_SPEC engine): then the flag stays, and the records are indexed as the parser indexed its side info */
            if (!keep_tns) u.d.ch[c].flags &= (uint8_t)~AACG_CHAN_TNS_PRESENT;
            if (c < p.n_ch && p.ch[c].window_sequence == AACG_EIGHT_SHORT_SEQUENCE) {
                uint32_t gmap = 0;
                int w = 0;
                for (int g = 0; g < p.ch[c].group_count; g++)
                    for (int k = 0; k < p.ch[c].group_len[g] && w < 8; k++, w++) gmap |= (uint32_t)g << (4 * w);
                u.gmap[c] = gmap;
            }
        }
        if (keep_tns) u.d.tns_offset = p.tns_offset;
    } else {
        u.d.flags = 0;
        for (int c = 0; c < 2; c++) {
            aacg_chan_info z = {};
            z.group_count = 1; z.group_len[0] = 1;                              /* ONLY_LONG, sine, nothing coded */
            u.d.ch[c] = z;
        }
        if (!want || e == 0) dp_g_atomic_add_u32(A.refused, 1u);    /* with a map: refused FRAMES (every element of one is refused together or for its own sake; the first counts) */
    }
    units[i] = u;
}

}  // namespace aacg_pipe

#endif
