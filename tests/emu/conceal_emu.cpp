/*
 * conceal_emu.cpp — the conceal stage's source (aac.js_amd/csrc/aacg_units_conceal.h: conceal_body) run lane by lane on CPU threads
 * (tests/emu/devport_emu.h) over unit records, results, spectrum and band-word blocks, a per-stream table and a state block that the
 * test made, for tests/test_units_conceal_emu.py, which compiles it into a library of its own and walks the rule in numpy
 * (tests/conceal_kit.py).
 * With -DCONCEAL_EMU_MAIN the same driver is a program: two batches of three streams over exactly sized heap blocks, for a build with
 * -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_units_conceal.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its arrays out by: sizeof(aacg_dev_unit), sizeof(aacg_conceal_stream), the workgroup's threads, the head's,
 * an element's and a block's bytes, and a side's bytes at 1, 2 and 8 parser channels */
void emu_conceal_sizes(uint32_t out[9])
{
    out[0] = (uint32_t)sizeof(aacg_dev_unit); out[1] = (uint32_t)sizeof(aacg_conceal_stream); out[2] = AACG_CONCEAL_THREADS;
    out[3] = (uint32_t)sizeof(aacg_conceal_head); out[4] = (uint32_t)sizeof(aacg_conceal_elem); out[5] = AACG_CONCEAL_BLOCK_BYTES;
    out[6] = AACG_CONCEAL_SIDE_BYTES(1u); out[7] = AACG_CONCEAL_SIDE_BYTES(2u); out[8] = AACG_CONCEAL_SIDE_BYTES(8u);
}

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order). */
void emu_conceal(aacg_dev_unit* units, aacg_parse_result* results, int16_t* q, aacg_band_meta* meta, const aacg_conceal_stream* tab, uint32_t n_streams,
                 uint32_t longest, uint32_t Cp, unsigned char* state, uint32_t n_slots, uint32_t fade_steps, uint32_t hold_frames, uint32_t blocks, int reverse)
{
    aacg_conceal_args A;
    std::memset(&A, 0, sizeof A);
    A.units = units; A.results = results; A.q = q; A.meta = meta; A.tab = tab; A.state = state; A.n_streams = n_streams; A.longest = longest;
    A.Cp = Cp; A.n_slots = n_slots; A.fade_steps = fade_steps; A.hold_frames = hold_frames;
    /* workgroups of AACG_CONCEAL_THREADS lanes, as hipLaunchKernelGGL(aacg_units_conceal, blocks, AACG_CONCEAL_THREADS) runs them */
    emu_launch((int)blocks, AACG_CONCEAL_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::conceal_body(A, blocks); });
}

}  // extern "C"

#ifdef CONCEAL_EMU_MAIN
/* Three streams on slots 2, 0, 1 of three: a CPE stream of 3 frames, an SCE + CPE + LFE stream of 2 and an SCE stream of 1, Cp = 8,
 * over heap blocks of exactly the buffers' sizes (the last stream's blocks end the spectrum and band-word buffers).  Batch 1: the
 * first stream's middle frame refused.  Batch 2: every frame refused, so that every stream reads the side batch 1 wrote and carries it
 * over.  Checked here: which frames come back concealed, that a concealed block holds its source's values, and the heads. */
struct batch_mem {
    aacg_dev_unit* units; aacg_parse_result* res; int16_t* q; aacg_band_meta* meta; aacg_conceal_stream* tab; uint32_t n_units, n_frames;
};
static const uint32_t kFrames[3] = {3, 2, 1}, kSlots[3] = {2, 0, 1}, kN[3] = {1, 3, 1}, kNch[3] = {2u, 1u | (2u << 2) | (1u << 4), 1u};

static bool make(batch_mem& B, uint32_t Cp, uint32_t salt, const uint32_t parity[3], const uint32_t fresh[3])
{
    B.n_units = 0; B.n_frames = 0;
    for (int s = 0; s < 3; s++) { B.n_units += kFrames[s] * kN[s]; B.n_frames += kFrames[s]; }
    B.units = (aacg_dev_unit*)calloc(B.n_units, sizeof(aacg_dev_unit));
    B.res = (aacg_parse_result*)calloc(B.n_frames, sizeof(aacg_parse_result));
    /* (the last frame is the SCE stream's: one block of its Cp is used, and the buffers end behind it) */
    const size_t blocks = (size_t)(B.n_frames - 1) * Cp + 1;
    B.q = (int16_t*)aligned_alloc(16, blocks * 2048);
    B.meta = (aacg_band_meta*)aligned_alloc(16, blocks * sizeof(aacg_band_meta));
    B.tab = (aacg_conceal_stream*)calloc(3, sizeof(aacg_conceal_stream));
    if (!B.units || !B.res || !B.q || !B.meta || !B.tab) return false;
    for (size_t i = 0; i < blocks * 1024; i++) B.q[i] = (int16_t)((i * 31u + salt) % 201u) - 100;
    for (size_t i = 0; i < blocks * 120; i++) ((uint16_t*)B.meta)[i] = (uint16_t)((((i + salt) % 16u) << 12) | ((i * 7u + salt) % 300u));
    uint32_t first = 0, unit = 0;
    for (int s = 0; s < 3; s++) {
        aacg_conceal_stream t = {first, kFrames[s], unit, kN[s] | (kN[s] << 8), kSlots[s], kNch[s], parity[s] | (fresh[s] << 1), 0u};
        B.tab[s] = t;
        for (uint32_t f = 0; f < kFrames[s]; f++) {
            uint32_t chan = 0;
            for (uint32_t e = 0; e < kN[s]; e++) {
                aacg_dev_unit& u = B.units[unit++];
                const uint32_t nch = (kNch[s] >> (2 * e)) & 3u;
                u.d.stream = kSlots[s]; u.d.channel = (uint16_t)chan; u.d.n_ch = (uint8_t)nch; u.d.coef_offset = u.d.meta_offset = (first + f) * Cp + chan;
                u.d.flags = (uint8_t)(salt & 3u);
                for (uint32_t c = 0; c < 2; c++) {
                    u.d.ch[c].window_sequence = (uint8_t)((f + e + c + salt) & 3u); u.d.ch[c].max_sfb = (uint8_t)(10 + f);
                    u.d.ch[c].group_count = u.d.ch[c].window_sequence == AACG_EIGHT_SHORT_SEQUENCE ? 3 : 1;
                    u.d.ch[c].group_len[0] = u.d.ch[c].group_count == 3 ? 2 : 1; u.d.ch[c].group_len[1] = u.d.ch[c].group_count == 3 ? 5 : 0; u.d.ch[c].group_len[2] = u.d.ch[c].group_count == 3 ? 1 : 0;
                }
                chan += nch;
            }
        }
        first += kFrames[s];
    }
    return true;
}
static void drop(batch_mem& B) { free(B.units); free(B.res); free(B.q); free(B.meta); free(B.tab); }

int main()
{
    const uint32_t Cp = 8, fade = 2, hold = 2;
    const size_t side = AACG_CONCEAL_SIDE_BYTES(Cp);
    unsigned char* state = (unsigned char*)aligned_alloc(16, 3 * 2 * side);
    if (!state) return 2;
    std::memset(state, 0xA5, 3 * 2 * side);
    int bad = 0;
    batch_mem B;
    const uint32_t p0[3] = {0, 1, 0}, fresh1[3] = {1, 1, 1};
    if (!make(B, Cp, 5, p0, fresh1)) return 2;
    B.res[1].status = AACG_PARSE_INSUFFICIENT_DATA;
    const int16_t want = B.q[(size_t)0 * Cp * 1024 + 1024 + 17];                 /* frame 0, channel 1 */
    emu_conceal(B.units, B.res, B.q, B.meta, B.tab, 3, 3, Cp, state, 3, fade, hold, 5, 1);
    bad |= B.res[1].flags != AACG_PARSE_CONCEALED || B.res[0].flags || B.res[2].flags || B.res[3].flags || B.res[5].flags;
    bad |= B.q[(size_t)1 * Cp * 1024 + 1024 + 17] != want;
    for (int s = 0; s < 3; s++) {
        const aacg_conceal_head* h = (const aacg_conceal_head*)(state + ((size_t)kSlots[s] * 2 + (p0[s] ^ 1u)) * side);
        bad |= h->has != 1u || h->r != 0u;
    }
    drop(B);
    const uint32_t p1[3] = {1, 0, 1}, fresh0[3] = {0, 0, 0};
    if (!make(B, Cp, 9, p1, fresh0)) return 2;
    for (uint32_t i = 0; i < B.n_frames; i++) B.res[i].status = AACG_PARSE_SCALEFACTOR;
    emu_conceal(B.units, B.res, B.q, B.meta, B.tab, 3, 3, Cp, state, 3, fade, hold, 2, 0);
    /* hold = 2: the first two frames of every stream repeat the frame batch 1 left; the CPE stream's third is silent */
    bad |= B.res[0].flags != AACG_PARSE_CONCEALED || B.res[1].flags != AACG_PARSE_CONCEALED || B.res[2].flags != 0;
    bad |= B.res[3].flags != AACG_PARSE_CONCEALED || B.res[4].flags != AACG_PARSE_CONCEALED || B.res[5].flags != AACG_PARSE_CONCEALED;
    for (int s = 0; s < 3; s++) {
        const aacg_conceal_head* h = (const aacg_conceal_head*)(state + ((size_t)kSlots[s] * 2 + (p1[s] ^ 1u)) * side);
        bad |= h->has != 1u || h->r != (kFrames[s] < hold + 1u ? kFrames[s] : hold + 1u);
    }
    drop(B);
    free(state);
    std::printf(bad ? "conceal_emu: FAILED\n" : "conceal_emu: ok\n");
    return bad;
}
#endif
