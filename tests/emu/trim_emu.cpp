/*
 * trim_emu.cpp — the PCM trim kernel's source (aac.js_amd/csrc/aacg_pcm_trim.h: trim_body, the body the host's switch would launch) run
 * lane by lane on CPU threads (tests/emu/devport_emu.h) over a packed PCM buffer and per-stream records that the test made, for
 * tests/test_pcm_trim_emu.py, which compiles it into a library of its own and slices in numpy.  With -DTRIM_EMU_MAIN the same driver is a
 * program: int16 and f32 cases of 1, 2, 3 and 8 channels, both layouts, over exactly sized heap blocks, for a build with
 * -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_trim.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, bytes of a stream's record, the samples of an item */
void emu_trim_sizes(uint32_t out[3]) { out[0] = AACG_TRIM_THREADS; out[1] = (uint32_t)sizeof(aacg_trim_stream); out[2] = AACG_TRIM_TILE; }

/* the rule and the item count as the host's part computes them */
void emu_trim_span(uint64_t Q, uint64_t skip, uint64_t keep, uint32_t n_in, uint32_t out[2]) { aacg_trim_span(Q, skip, keep, n_in, &out[0], &out[1]); }
uint32_t emu_trim_items(uint32_t n_keep, int planar) { return aacg_trim_items(n_keep, planar); }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order).  Returns 0 if no
 * body serves the launch. */
int emu_trim(const void* src, void* dst, const void* rec, uint64_t src_elems, uint32_t n_streams, uint32_t n_items, uint32_t row, uint32_t channels, uint32_t elem,
             uint32_t blocks, int reverse)
{
    if (!n_items || !n_streams || (row & 1023u)) return 0;
    aacg_trim_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_trim_stream*)rec; A.src_elems = src_elems;
    A.n_streams = n_streams; A.n_items = n_items; A.row = row; A.channels = channels; A.elem = elem;
    int ran = 0;
    /* the body the host's switch picks (aacg_trim_launch), in workgroups of AACG_TRIM_THREADS lanes with the body's static LDS */
#define EMU_TRIM_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { ran = 1; emu_launch((int)blocks, AACG_TRIM_THREADS, AACG_TRIM_LDS_BYTES(C, (int)sizeof(T)), reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::trim_body<T, C>(A, blocks); }); }
    AACG_TRIM_BODIES(EMU_TRIM_RUN)
    return ran;
}

}  // extern "C"

#ifdef TRIM_EMU_MAIN
/* one case: four streams of n_in samples each, one behind the other in a source of exactly their size; they keep [skip, skip + n_keep)
 * with odd skips and ragged counts — one keeps nothing, one keeps up to the source's last element — into a destination of exactly the
 * output's size */
template <typename T>
static int one_case(uint32_t C, int planar, uint32_t blocks, int reverse)
{
    const uint32_t S = 4, n_in = 1301, skip[S] = {1, 640, 0, 777}, keep[S] = {2 * AACG_TRIM_TILE + 5, 0, 9, n_in - 777};
    aacg_trim_stream* rec = (aacg_trim_stream*)malloc(S * sizeof(aacg_trim_stream));
    uint32_t total = 0, items = 0, longest = 0;
    for (uint32_t s = 0; s < S; s++) {
        rec[s] = {s * n_in + skip[s], keep[s], total, items};
        total += keep[s]; items += aacg_trim_items(keep[s], planar);
        if (keep[s] > longest) longest = keep[s];
    }
    const uint32_t row = planar ? ((longest + 1023u) / 1024u) * 1024u : 0u;
    const size_t n_src = (size_t)S * n_in * C, n_dst = planar ? (size_t)S * C * row : (size_t)total * C;
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, n_src * sizeof(T))) return 2;
    T* src = (T*)mem;
    T* dst = (T*)malloc(n_dst * sizeof(T));               /* (16-byte aligned as malloc makes it; exactly sized, ragged as the output is) */
    if (!src || !dst || !rec) return 2;
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int16_t)(uint16_t)(i * 7u + 1u);
    std::memset(dst, 0x7f, n_dst * sizeof(T));
    const int ran = emu_trim(src, dst, rec, n_src, S, items, row, C, (uint32_t)sizeof(T), blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t j = 0; j < (planar ? row : keep[s]); j++)
            for (uint32_t c = 0; c < C; c++) {
                const T got = planar ? dst[((size_t)s * C + c) * row + j] : dst[((size_t)rec[s].out_first + j) * C + c];
                const T want = j < keep[s] ? src[((size_t)rec[s].src_first + j) * C + c] : (T)0;
                wrong += std::memcmp(&got, &want, sizeof(T)) != 0;
            }
    free(src); free(dst); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "trim_emu: %u channels of %zu bytes, %s, %u workgroups%s: %zu elements differ\n", C, sizeof(T), planar ? "planar" : "packed", blocks,
                                    reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    for (uint32_t C : {1u, 2u, 3u, 8u}) {
        bad |= one_case<int16_t>(C, 0, 1, 0);
        bad |= one_case<int16_t>(C, 1, 3, 1);
        bad |= one_case<float>(C, 0, 5, 1);
        bad |= one_case<float>(C, 1, 2, 0);
    }
    std::printf(bad ? "trim_emu: FAILED\n" : "trim_emu: ok\n");
    return bad;
}
#endif
