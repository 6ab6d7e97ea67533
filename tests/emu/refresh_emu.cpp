/*
 * refresh_emu.cpp — the unit refresh kernel's source (aac.js_amd/csrc/aacg_units_refresh.h: refresh_body) run lane by lane on CPU
 * threads (tests/emu/devport_emu.h) over plan records, parser records, results and a refresh map that the test made, for
 * tests/test_units_refresh_emu.py, which compiles it into a library of its own and states the rule in numpy.  The lanes of a
 * workgroup are concurrent threads: a lane's reads of its frame siblings' records and of the frame's result really overlap the
 * siblings' writes.  With -DREFRESH_EMU_MAIN the same driver is a program: the map cases over heap blocks of exactly the arrays'
 * sizes, for a build with -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_units_refresh.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* sizeof(aacg_dev_unit), sizeof(aacg_refresh_map), sizeof(aacg_parse_result), AACG_REFRESH_THREADS: what the test lays its arrays out by */
void emu_refresh_sizes(uint32_t out[4])
{
    out[0] = (uint32_t)sizeof(aacg_dev_unit); out[1] = (uint32_t)sizeof(aacg_refresh_map); out[2] = (uint32_t)sizeof(aacg_parse_result); out[3] = AACG_REFRESH_THREADS;
}

/* One launch as aacg_refresh_launch makes it: ceil(n_units / AACG_REFRESH_THREADS) workgroups of AACG_REFRESH_THREADS lanes, run in
 * the order given by `reverse` (workgroups of a launch run in any order). */
void emu_refresh(aacg_dev_unit* units, const aacg_unit_desc* parsed, aacg_parse_result* results, const aacg_refresh_map* map, uint32_t n_units,
                 uint32_t max_units, int refuse_pns, int keep_tns, uint32_t* refused, int reverse)
{
    const aacg_refresh_args A = {units, parsed, results, map, n_units, max_units, refuse_pns, keep_tns, refused};
    const uint32_t blocks = (n_units + AACG_REFRESH_THREADS - 1u) / AACG_REFRESH_THREADS;
    emu_launch((int)blocks, AACG_REFRESH_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::refresh_body(A, AACG_REFRESH_THREADS); });
}

}  // extern "C"

#ifdef REFRESH_EMU_MAIN
/* A map case over heap blocks of exactly n_units records, n_frames * max_units parsed records and n_frames results: frames of
 * `want` elements (nch[e] channels each) of which the plan lists `listed`, frame after frame; every parsed channel EIGHT_SHORT with
 * the group lengths `groups`.  fault[f]: 0 none, 1 + k: element k's blocks moved in the plan, -1: parse error, -2: one element too
 * few, -3: one too many (the listed ones match).  Checked here: which frames went silent, the statuses, the counter, and the group
 * map of the accepted ones. */
static int one_case(const char* name, uint32_t n_frames, uint32_t max_units, const std::vector<uint32_t>& nch, uint32_t listed, const std::vector<int>& fault,
                    const std::vector<uint8_t>& groups, uint32_t want_gmap, int reverse)
{
    const uint32_t want = (uint32_t)nch.size(), n_units = n_frames * listed;
    uint32_t Cp = 0;
    for (uint32_t c : nch) Cp += c;
    aacg_dev_unit* units = (aacg_dev_unit*)malloc(sizeof(aacg_dev_unit) * n_units);
    aacg_unit_desc* parsed = (aacg_unit_desc*)malloc(sizeof(aacg_unit_desc) * n_frames * max_units);
    aacg_parse_result* results = (aacg_parse_result*)malloc(sizeof(aacg_parse_result) * n_frames);
    aacg_refresh_map* map = (aacg_refresh_map*)malloc(sizeof(aacg_refresh_map) * n_units);
    uint32_t* refused = (uint32_t*)malloc(sizeof(uint32_t));
    if (!units || !parsed || !results || !map || !refused) return 2;
    std::memset(units, 0xA5, sizeof(aacg_dev_unit) * n_units);
    std::memset(parsed, 0xff, sizeof(aacg_unit_desc) * n_frames * max_units);
    std::memset(results, 0, sizeof(aacg_parse_result) * n_frames);
    *refused = 0;
    uint32_t expect_refused = 0;
    for (uint32_t f = 0; f < n_frames; f++) {
        const int ft = fault[f];
        results[f].status = ft == -1 ? AACG_PARSE_SCALEFACTOR : AACG_PARSE_OK;
        results[f].n_units = (uint8_t)(ft == -2 ? want - 1 : ft == -3 ? want + 1 : want);
        expect_refused += ft != 0;
        uint32_t chan = 0;
        for (uint32_t e = 0; e < want; e++) {
            aacg_unit_desc& p = parsed[f * max_units + e];
            if (ft != -1) {
                std::memset(&p, 0, sizeof p);
                p.n_ch = (uint8_t)nch[e]; p.channel = (uint16_t)chan; p.coef_offset = p.meta_offset = f * Cp + chan;
                p.flags = AACG_UNIT_COMMON_WINDOW; p.tns_offset = 7;
                for (int c = 0; c < 2; c++) {
                    p.ch[c].window_sequence = AACG_EIGHT_SHORT_SEQUENCE; p.ch[c].flags = AACG_CHAN_TNS_PRESENT;
                    p.ch[c].group_count = (uint8_t)groups.size();
                    for (size_t g = 0; g < groups.size(); g++) p.ch[c].group_len[g] = groups[g];
                }
            }
            if (e < listed) {
                aacg_dev_unit& u = units[f * listed + e];
                u.d.stream = 0; u.d.pcm_offset = f * 1024 * Cp; u.d.n_out_ch = (uint16_t)Cp;
                u.d.n_ch = (uint8_t)nch[e]; u.d.channel = (uint16_t)chan; u.d.coef_offset = u.d.meta_offset = f * Cp + chan + (ft == 1 + (int)e ? 1000u : 0u);
                map[f * listed + e] = aacg_refresh_map{f * max_units + e, want | (listed << 8)};
            }
            chan += nch[e];
        }
    }
    emu_refresh(units, parsed, results, map, n_units, max_units, 1, 0, refused, reverse);
    int bad = *refused != expect_refused;
    for (uint32_t f = 0; f < n_frames; f++) {
        const int ft = fault[f];
        bad |= results[f].status != (ft == -1 ? AACG_PARSE_SCALEFACTOR : ft ? AACG_PARSE_LAYOUT : AACG_PARSE_OK);
        for (uint32_t e = 0; e < listed; e++) {
            const aacg_dev_unit& u = units[f * listed + e];
            bad |= u.d.tns_offset != 0 || (u.d.ch[0].flags | u.d.ch[1].flags) != 0;
            if (ft) bad |= u.d.flags != 0 || u.gmap[0] != 0 || u.gmap[1] != 0 || u.d.ch[0].window_sequence != 0 || u.d.ch[0].group_count != 1 || u.d.ch[1].group_len[0] != 1;
            else bad |= u.d.flags != AACG_UNIT_COMMON_WINDOW || u.gmap[0] != want_gmap || u.gmap[1] != (nch[e] == 2 ? want_gmap : 0u) || u.d.ch[1].window_sequence != AACG_EIGHT_SHORT_SEQUENCE;
        }
    }
    free(units); free(parsed); free(results); free(map); free(refused);
    if (bad) std::fprintf(stderr, "refresh_emu: %s%s: the records, the results or the counter are not the rule's\n", name, reverse ? " (workgroups in reverse)" : "");
    return bad;
}

int main()
{
    int bad = 0;
    for (int reverse = 0; reverse < 2; reverse++) {
        /* five elements in eight channels, 52 frames = 260 units: frame 51's first lane is lane 255 of workgroup 0, its others are in workgroup 1 */
        std::vector<int> fault(52, 0);
        fault[0] = 1; fault[1] = 3; fault[2] = 5; fault[7] = -1; fault[9] = -2; fault[11] = -3; fault[50] = 3; fault[51] = 5;
        bad |= one_case("five elements, [3, 4, 1]", 52, 8, {1, 2, 2, 2, 1}, 5, fault, {3, 4, 1}, 0x21111000u, reverse);
        fault[51] = 1; fault[50] = 0;
        bad |= one_case("five elements, eight groups", 52, 8, {1, 2, 2, 2, 1}, 5, fault, {1, 1, 1, 1, 1, 1, 1, 1}, 0x76543210u, reverse);
        /* group lengths that sum past eight: the walk stops at the eighth window (a shift by 32 or more is what the bound keeps out) */
        bad |= one_case("group lengths beyond eight windows", 52, 8, {1, 2, 2, 2, 1}, 5, fault, {3, 4, 5, 2}, 0x21111000u, reverse);
        bad |= one_case("eight groups of two", 3, 8, {2}, 1, {0, 0, 0}, {2, 2, 2, 2, 2, 2, 2, 2}, 0x33221100u, reverse);
        /* SCE + CPE + CPE, two of three listed: the last frame's lanes must not look behind the records */
        std::vector<int> f2(130, 0);
        f2[0] = 2; f2[5] = -2; f2[64] = 1; f2[127] = -1; f2[129] = 2;
        bad |= one_case("two of three listed", 130, 3, {1, 2, 2}, 2, f2, {2, 6}, 0x11111100u, reverse);
    }
    std::printf(bad ? "refresh_emu: FAILED\n" : "refresh_emu: ok\n");
    return bad;
}
#endif
