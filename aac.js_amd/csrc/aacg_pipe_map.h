/*
 * aacg_pipe_map.h — a resident batch's refresh map (aacg_refresh_map, include/aacgpu.h), listed on the host by the planner and
 * expanded on the device by aacg_pipe_map (aacg_pipeline.hip) from a per-stream table of O(streams) bytes.
 *
 * A batch of the resident route (aacg_pipeline_submit_ragged) brings frames_of[s] consecutive frames of stream s; they are
 * parsed frames first_s .. first_s + frames_of[s] - 1 (first_s: the prefix sum of the counts), the parser puts frame i's element
 * e at record i * U + e, and the kept plan lists, frame by frame, the first `kept` elements of the stream's layout.  The plan's
 * unit records depend on the batch's shape only (they are uploaded once, when the plan is made); the map — where each plan unit
 * finds its parsed record — is rewritten for every batch into the lane's own buffer on the lane's stream, so that a new shape
 * costs no device allocation and no synchronous copy on the submit path.
 *
 * Written against devport.h like aacg_parse.h, and executed lane by lane on the CPU by tests/emu/map_emu.cpp.
 */
#ifndef AACG_PIPE_MAP_H
#define AACG_PIPE_MAP_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/aacgpu.h"

#if defined(AACG_EMU_BUILD)
#include "devport_emu.h"
#else
#include "devport.h"
#endif

#define AACG_PIPE_MAP_THREADS 64

/* one stream of a batch, as the device expands it (16 bytes; the table travels behind the frame table in the lane's staging) */
typedef struct aacg_pipe_stream {
    uint32_t frame_first;      /* first_s: the stream's first frame in the batch's packed order                           */
    uint32_t frames;           /* frames_of[s]                                                                             */
    uint32_t unit_first;       /* the stream's first unit in the plan: the sum of frames * kept over the streams before it  */
    uint32_t frame_units;      /* bits 0..7: the layout's elements (n); bits 8..15: how many of them are decoded (kept);
                                  kept = 0: the stream has no layout yet and no unit in the plan                         */
} aacg_pipe_stream;

/* a stream's element layout: channels of every SCE / LFE / CPE of a frame in order; kept = how many of them fit the channels */
struct aacg_pipe_layout { uint8_t n = 0, kept = 0; uint8_t nch[8] = {}; };

namespace aacg_pipe {

/* Workgroup b of `blocks` expands streams b, b + blocks, ...: plan unit unit_first + f * kept + e <- parsed record
 * (frame_first + f) * U + e, every unit of the stream with the layout's word. */
DP_DEVICE void map_body(const aacg_pipe_stream* tab, uint32_t n_streams, uint32_t U, aacg_refresh_map* map, uint32_t blocks)
{
    for (uint32_t s = (uint32_t)dp_block(); s < n_streams; s += blocks) {
        const aacg_pipe_stream t = tab[s];
        const uint32_t kept = (t.frame_units >> 8) & 0xffu;
        if (!kept) continue;
        const uint32_t n = t.frames * kept;
        for (uint32_t j = (uint32_t)dp_tid(); j < n; j += AACG_PIPE_MAP_THREADS) {
            const uint32_t f = j / kept, e = j - f * kept;
            aacg_refresh_map m;
            m.parsed_index = (t.frame_first + f) * U + e;
            m.frame_units = t.frame_units;
            map[t.unit_first + j] = m;
        }
    }
}

/* The host planner: for a batch of n_streams streams (lay[s]: stream s's layout; slots[s]: its slot; frames_of[s]: its frames),
 * the plan's unit records (units), the refresh map they are refreshed through (map) and the device's per-stream table (table),
 * each only where the pointer is not null.  Frame f of stream s is parsed frame i = first_s + f; the parser (max_units U,
 * max_channels Cp) puts its element e at record i * U + e and its running channel c at block i * Cp + c; its PCM lies at
 * i * 1024 * C.  Returns the number of plan units. */
inline uint32_t plan_list(const aacg_pipe_layout* lay, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams,
                          uint32_t C, uint32_t Cp, uint32_t U, std::vector<aacg_unit_desc>* units, std::vector<aacg_refresh_map>* map,
                          aacg_pipe_stream* table)
{
    uint32_t first = 0, n_units = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        const aacg_pipe_layout& L = lay[s];
        const uint32_t F = frames_of[s], word = (uint32_t)L.n | ((uint32_t)L.kept << 8);
        if (table) table[s] = aacg_pipe_stream{first, F, n_units, word};
        for (uint32_t f = 0; (units || map) && f < F; f++) {
            const uint32_t i = first + f;
            uint32_t chan = 0;
            for (uint32_t e = 0; e < L.kept; e++) {
                if (units) {
                    aacg_unit_desc d;
                    memset(&d, 0, sizeof d);
                    d.stream = slots[s]; d.pcm_offset = i * 1024u * C; d.channel = (uint16_t)chan; d.n_out_ch = (uint16_t)C; d.n_ch = L.nch[e];
                    d.coef_offset = d.meta_offset = i * Cp + chan;
                    for (uint32_t c = 0; c < d.n_ch; c++) { d.ch[c].group_count = 1; d.ch[c].group_len[0] = 1; }
                    units->push_back(d);
                }
                if (map) map->push_back(aacg_refresh_map{i * U + e, word});
                chan += L.nch[e];
            }
        }
        first += F;
        n_units += F * L.kept;
    }
    return n_units;
}

}  // namespace aacg_pipe

#endif
