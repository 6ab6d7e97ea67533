/*
 * aacg_tns_bands.h — the band limits of the TNS tool for one sample index: the scalefactor-band offsets a filter region is cut
 * from and TNS_MAX_BANDS (tns.js:65-66).  ONE definition for the two makers of aacg_dev_tns records: aacg_tns_prepare on the host
 * (aacg_plan.cpp) takes its limits from it, and aacg_tns_records (aacg_tns_prep.h) gets it with its kernel arguments.  Plain C++,
 * no HIP.
 */
#ifndef AACG_TNS_BANDS_H
#define AACG_TNS_BANDS_H

#include <stdint.h>

typedef struct aacg_tns_bands {
    uint16_t swb_long[64];     /* SWB_OFFSET_1024[sample_index], [n_long] = 1024 (tables.js:34-155)                    */
    uint16_t swb_short[16];    /* SWB_OFFSET_128[sample_index], [n_short] = 128                                         */
    uint32_t n_long, n_short;  /* swbCount of either window length                                                      */
    uint32_t tns_long;         /* TNS_MAX_BANDS_1024[sample_index]                                                      */
    uint32_t tns_short;        /* TNS_MAX_BANDS_128[sample_index]: tns.js:106 intends min(maxBands, maxSFB); the short-window
                                  table is the documented deviation of SPEC mode                                        */
} aacg_tns_bands;

int aacg_swb_offsets(int sample_index, int is_long, int* dst);      /* aacg_tables.cpp */

/* 0, or -1 for a sample index without tables (> 11; the TNS tables know a thirteenth the band tables do not) */
static inline int aacg_tns_bands_make(int sample_index, aacg_tns_bands* b)
{
    /* TNS_MAX_BANDS_1024 / _128 (tns.js:65-66; ISO/IEC 14496-3 Table 4.138) by sampleIndex */
    static const uint8_t kTnsMaxBandsLong[13]  = {31, 31, 34, 40, 42, 51, 46, 46, 42, 42, 42, 39, 39};
    static const uint8_t kTnsMaxBandsShort[13] = {9, 9, 10, 14, 14, 14, 14, 14, 14, 14, 14, 14, 14};
    int off[64];
    *b = aacg_tns_bands();
    if (sample_index < 0 || sample_index > 11) return -1;
    b->n_long = (uint32_t)aacg_swb_offsets(sample_index, 1, off);
    for (uint32_t i = 0; i <= b->n_long && i < 64; i++) b->swb_long[i] = (uint16_t)off[i];
    b->n_short = (uint32_t)aacg_swb_offsets(sample_index, 0, off);
    for (uint32_t i = 0; i <= b->n_short && i < 16; i++) b->swb_short[i] = (uint16_t)off[i];
    b->tns_long = kTnsMaxBandsLong[sample_index];
    b->tns_short = kTnsMaxBandsShort[sample_index];
    return 0;
}

#endif
