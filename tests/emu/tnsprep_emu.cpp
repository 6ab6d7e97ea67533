/*
 * tnsprep_emu.cpp — the TNS records kernel's source (aac.js_amd/csrc/aacg_tns_prep.h: tns_records_body) and the matrices kernel
 * behind it (aacg_kernels.h: tns_matrices_body) run lane by lane on the CPU (tests/emu/devport_emu.h), next to what the host
 * makes of the same parser outputs (aacg_tns_prepare, aacg_plan.cpp; tns_matrix_row), for tests/test_tns_records_emu.py, which
 * compiles it into a library of its own.  Neither body has a point where lanes meet, so the lanes run one after the other, on
 * purpose: no thread per lane, and so not through emu_launch.h like the other drivers here.
 * TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_kernels.h"
#include "../../aac.js_amd/csrc/aacg_tns_prep.h"
#include "../../aac.js_amd/csrc/aacg_host.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* sizes of the records the test lays out */
void emu_tnsprep_sizes(uint32_t out[6])
{
    out[0] = sizeof(aacg_dev_tns); out[1] = sizeof(aacg_tns_info); out[2] = sizeof(aacg_unit_desc); out[3] = sizeof(aacg_parse_result);
    out[4] = AACG_TNS_M_DOUBLES; out[5] = sizeof(aacg_tnsprep_args);
}
/* where the matrices start behind n records, and the whole buffer (aacg_tns_records_bytes) */
uint64_t emu_tnsprep_layout(uint32_t n, uint64_t* total) { *total = aacg_tns_buffer_bytes(n); return aacg_tns_record_bytes(n); }

/* The two launches of aacg_tns_records_from_parse on a buffer of aacg_tns_buffer_bytes(n_frames * parse_channels) bytes, over
 * whatever it holds (the caller poisons it): `blocks` workgroups of AACG_TNSPREP_THREADS lanes, then the matrices' launch as
 * aacg_tns_matrices_launch sizes it.  Returns 0, or -1 for a sample index without tables. */
int emu_tns_records(int sample_index, const aacg_unit_desc* units, const aacg_parse_result* results, const aacg_tns_info* info,
                    uint32_t n_frames, uint32_t max_units, uint32_t parse_channels, uint32_t blocks, void* buffer)
{
    aacg_tnsprep_args A;
    std::memset(&A, 0, sizeof A);
    if (aacg_tns_bands_make(sample_index, &A.bands)) return -1;
    const uint32_t n = n_frames * parse_channels;
    A.units = units; A.results = results; A.info = info; A.recs = (aacg_dev_tns*)buffer;
    A.n_frames = n_frames; A.max_units = max_units; A.parse_channels = parse_channels;
    emu_wave wave;
    emu_block blk;
    std::memset(&wave, 0, sizeof wave);
    std::memset(&blk, 0, sizeof blk);
    for (uint32_t b = 0; b < blocks; b++)
        for (int t = 0; t < AACG_TNSPREP_THREADS; t++) {
            blk.block_id = (int)b;
            g_emu = emu_lane_ctx{t & 63, t >> 6, &wave, &blk};
            aacg_tnsprep::tns_records_body(A, blocks);
        }
    double* M = (double*)((char*)buffer + aacg_tns_record_bytes(n));
    for (uint32_t b = 0; b < (n + AACG_WG_WAVES - 1) / AACG_WG_WAVES; b++)
        for (int t = 0; t < AACG_WG_THREADS; t++) {
            blk.block_id = (int)b;
            g_emu = emu_lane_ctx{t & 63, t >> 6, &wave, &blk};
            tns_matrices_body(A.recs, M, n);
        }
    return 0;
}

/* The host's records of the same outputs, as aacg_plan_build makes them: aacg_tns_prepare for every channel with
 * AACG_CHAN_TNS_PRESENT of every unit of every frame that parsed, at tns_offset + c; every other record zero.  The matrices from
 * tns_matrix_row, row by row, for every record.  `buffer` is laid out like the device's.  Returns the number of channels
 * aacg_tns_prepare refused (their records are what it left). */
int emu_tns_host(int sample_index, const aacg_unit_desc* units, const aacg_parse_result* results, const aacg_tns_info* info,
                 uint32_t n_frames, uint32_t max_units, uint32_t parse_channels, void* buffer)
{
    const uint32_t n = n_frames * parse_channels;
    aacg_dev_tns* recs = (aacg_dev_tns*)buffer;
    std::memset(buffer, 0, aacg_tns_buffer_bytes(n));
    int refused = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        if (results[f].status != AACG_PARSE_OK) continue;
        for (uint32_t e = 0; e < results[f].n_units && e < max_units; e++) {
            const aacg_unit_desc& u = units[(size_t)f * max_units + e];
            for (uint32_t c = 0; c < u.n_ch && c < 2; c++) {
                if (!(u.ch[c].flags & AACG_CHAN_TNS_PRESENT)) continue;
                const uint32_t ti = u.tns_offset + c;
                if (ti >= n) std::abort();                          /* the test's own records are wrong */
                if (aacg_tns_prepare(sample_index, &u.ch[c], &info[ti], &recs[ti])) refused++;
            }
        }
    }
    double* M = (double*)((char*)buffer + aacg_tns_record_bytes(n));
    for (uint32_t k = 0; k < n; k++)
        for (int f = 0; f < 3; f++) {
            float lpc[AACG_TNS_MAX_ORDER];
            for (int i = 0; i < AACG_TNS_MAX_ORDER; i++) lpc[i] = i < recs[k].order[f] ? recs[k].lpc[f][i] : 0.0f;
            for (int r = 0; r < AACG_TNS_MAX_ORDER; r++) {
                double row[AACG_TNS_MAX_ORDER];
                tns_matrix_row(lpc, r, row);
                std::memcpy(M + (size_t)k * AACG_TNS_M_DOUBLES + (size_t)(f * AACG_TNS_MAX_ORDER + r) * AACG_TNS_MAX_ORDER, row, sizeof row);
            }
        }
    return refused;
}

}  // extern "C"
