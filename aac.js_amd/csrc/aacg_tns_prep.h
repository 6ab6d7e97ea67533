/*
 * aacg_tns_prep.h — a batch's TNS records made on the device (aacg_tns_records, aacg_engine_tnsprep.hip): what aacg_tns_prepare
 * (aacg_plan.cpp, tns.js:111-152) makes of an aacg_tns_info on the host — per filter slot the sample range, the direction and the
 * direct-form coefficients of the step-up recursion — from the device parser's outputs, without a visit to the host, BYTE FOR BYTE
 * what the host function writes.
 *
 * One lane per record, and a record per parser channel block: the record of (frame, channel block) lies at the index the parsed
 * unit's tns_offset + c names (aacg_parse.h: the frame's first block plus the running channel), so the run kernels index it as they
 * index host-made records.  A lane writes its whole record: zeros first (order 0 in every slot), then the slots of the filters if an
 * accepted frame's unit owns the block and its channel has AACG_CHAN_TNS_PRESENT.  A refused frame's parser records are never read.
 * Global memory only, no LDS; the recursion is unrolled over the orders so that the coefficients stay in registers.
 *
 * Written against devport.h like aacg_plan_shape.h, and executed lane by lane on the CPU by tests/emu/tnsprep_emu.cpp.
 */
#ifndef AACG_TNS_PREP_H
#define AACG_TNS_PREP_H

#include <stdint.h>

#include "../../include/aacgpu.h"
#ifdef AACG_EMU_BUILD
#include "devport_emu.h"
#else
#include "devport.h"
#endif
#include "aacg_device.h"
#include "aacg_tns_bands.h"

#define AACG_TNSPREP_THREADS 64

/* what one launch prepares: the parser's outputs of one batch (aacg_parse_device) and where the records go */
typedef struct aacg_tnsprep_args {
    const aacg_unit_desc*    units;      /* [n_frames * max_units]                                                       */
    const aacg_parse_result* results;    /* [n_frames]                                                                   */
    const aacg_tns_info*     info;       /* [n_frames * parse_channels]                                                  */
    aacg_dev_tns*            recs;       /* [n_frames * parse_channels]                                                  */
    uint32_t n_frames, max_units, parse_channels, reserved;
    aacg_tns_bands bands;                /* of the engine's sample index: read from the kernel arguments                 */
} aacg_tnsprep_args;

namespace aacg_tnsprep {

static_assert(sizeof(aacg_dev_tns) == 512 && AACG_TNS_MAX_ORDER == 12, "aacg_dev_tns: 128 words a record, twelve coefficients a slot");

/* tns.js:128-140 with its Float32Array stores: lpc <- the direct form of the first `order` reflection coefficients.  The product
 * of two floats is exact in double (24 + 24 bits of significand in 53), so a fused multiply-add and a multiply followed by an
 * addition round the same sum once and agree; the recursion is compiled without contraction all the same, like the other sites
 * that must match the host bit for bit.  Unrolled over all twelve orders: no indexed array, no scratch. */
DP_DEVICE void step_up(const float (&coef)[AACG_TNS_MAX_ORDER], int order, float (&lpc)[AACG_TNS_MAX_ORDER])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < AACG_TNS_MAX_ORDER; i++) {
        if (i < order) {
            const float r = -coef[i];
            lpc[i] = r;
#pragma unroll
            for (int j = 0; j < ((i + 1) >> 1); j++) {
                const float fj = lpc[j], b = lpc[i - 1 - j];
                lpc[j] = (float)((double)fj + (double)r * (double)b);
                lpc[i - 1 - j] = (float)((double)b + (double)r * (double)fj);
            }
        }
    }
}

/* Lane t of workgroup b of `blocks` makes records b * 64 + t, + blocks * 64, ... */
DP_DEVICE void tns_records_body(const aacg_tnsprep_args& A, uint32_t blocks)
{
    const uint32_t n = A.n_frames * A.parse_channels;
    for (uint32_t idx = (uint32_t)dp_block() * AACG_TNSPREP_THREADS + (uint32_t)dp_tid(); idx < n; idx += blocks * AACG_TNSPREP_THREADS) {
        aacg_dev_tns* out = A.recs + idx;
        uint32_t* words = (uint32_t*)(void*)out;
        for (uint32_t k = 0; k < sizeof(aacg_dev_tns) / 4u; k++) words[k] = 0u;
        const uint32_t frame = idx / A.parse_channels;
        const aacg_parse_result res = A.results[frame];
        if (res.status != AACG_PARSE_OK) continue;
        /* the unit that owns this block, if its channel carries TNS side info: units[frame][e], e below the frame's count */
        const uint32_t n_units = res.n_units < A.max_units ? res.n_units : A.max_units;
        const aacg_chan_info* ci = nullptr;
        for (uint32_t e = 0; e < n_units; e++) {
            const aacg_unit_desc* u = A.units + (size_t)frame * A.max_units + e;
            for (uint32_t c = 0; c < 2; c++)
                if (c < u->n_ch && (u->ch[c].flags & AACG_CHAN_TNS_PRESENT) && u->tns_offset + c == idx) ci = &u->ch[c];
        }
        if (!ci) continue;
        const aacg_tns_info* in = A.info + idx;
        const bool is_short = ci->window_sequence == AACG_EIGHT_SHORT_SEQUENCE;
        const uint16_t* swb = is_short ? A.bands.swb_short : A.bands.swb_long;
        const int swb_count = (int)(is_short ? A.bands.n_short : A.bands.n_long);
        const int max_bands = (int)(is_short ? A.bands.tns_short : A.bands.tns_long), max_sfb = ci->max_sfb;
        const int mmm = max_bands < max_sfb ? max_bands : max_sfb;               /* <= 51 / 14: inside swb_long[64] / swb_short[16] */
        const int n_win = is_short ? 8 : 1;
        for (int w = 0; w < n_win; w++) {
            int bottom = swb_count;                                              /* tns.js:112 */
            int nf = in->n_filt[w];
            if (nf > (is_short ? 1 : 3)) nf = 0;                                 /* more filters than the syntax has: the window's slots stay empty */
            for (int f = 0; f < nf; f++) {
                const int slot = is_short ? w : f;
                const aacg_tns_filter* tf = &in->filt[slot];
                const int top = bottom;                                          /* tns.js:121-123: an order-0 filter moves bottom too */
                bottom = top - (int)tf->length;
                if (bottom < 0) bottom = 0;
                const int order = tf->order;
                /* AAC-LC limits (aacg_tns_prepare): 12 for long windows, 3 bits for short ones; the parser refuses a frame beyond
                 * them (AACG_PARSE_TNS_ORDER) — whatever is read here, nothing is indexed past twelve: the slot stays empty */
                if (order == 0 || order > (is_short ? 8 : AACG_TNS_MAX_ORDER)) continue;
                float coef[AACG_TNS_MAX_ORDER], lpc[AACG_TNS_MAX_ORDER];
#pragma unroll
                for (int i = 0; i < AACG_TNS_MAX_ORDER; i++) { coef[i] = i < order ? tf->coef[i] : 0.0f; lpc[i] = 0.0f; }
                step_up(coef, order, lpc);
                int start = swb[bottom < mmm ? bottom : mmm];                    /* tns.js:142-152 */
                const int end = swb[top < mmm ? top : mmm];
                const int size = end - start;
                if (size <= 0) continue;
                int inc = 1;
                if (tf->direction) { inc = -1; start = end - 1; }
                out->start[slot] = start + w * 128;
                out->size[slot] = size;
                out->inc[slot] = inc;
                out->order[slot] = order;
#pragma unroll
                for (int i = 0; i < AACG_TNS_MAX_ORDER; i++) if (i < order) out->lpc[slot][i] = lpc[i];
            }
        }
    }
}

}  // namespace aacg_tnsprep

#endif
