/*
 * carry_emu.cpp — the window-shape carry kernel's source (aac.js_amd/csrc/aacg_shape_carry.h: carry_body) run lane by lane on CPU
 * threads (tests/emu/devport_emu.h) over unit records, a refresh map and the engine's per-channel entries that the test made, for
 * tests/test_shape_carry_emu.py, which compiles it into a library of its own and walks the rule in numpy.  TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_shape_carry.h"

thread_local emu_lane_ctx g_emu;

namespace {

struct lane_arg { emu_lane_ctx ctx; const aacg_carry_args* A; uint32_t blocks; };

void* lane_main(void* p)
{
    lane_arg* a = (lane_arg*)p;
    g_emu = a->ctx;
    aacg_pipe::carry_body(*a->A, a->blocks);
    return nullptr;
}

/* one workgroup of AACG_CARRY_THREADS lanes, as hipLaunchKernelGGL(aacg_units_carry_shape, blocks, AACG_CARRY_THREADS) runs it */
void run_block(const aacg_carry_args& A, uint32_t blocks, int block)
{
    const int threads = AACG_CARRY_THREADS, waves = threads / 64;
    std::vector<emu_wave> wv((size_t)waves);
    std::vector<lane_arg> args((size_t)threads);
    std::vector<pthread_t> tid((size_t)threads);
    emu_block blk;
    blk.lds = nullptr; blk.lds_bytes = 0; blk.block_id = block;
    pthread_barrier_init(&blk.bar, nullptr, (unsigned)threads);
    for (int w = 0; w < waves; w++) pthread_barrier_init(&wv[(size_t)w].bar, nullptr, 64);
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 64 * 1024);
    for (int t = 0; t < threads; t++) {
        args[(size_t)t] = lane_arg{emu_lane_ctx{t & 63, t >> 6, &wv[(size_t)(t >> 6)], &blk}, &A, blocks};
        pthread_create(&tid[(size_t)t], &attr, lane_main, &args[(size_t)t]);
    }
    for (int t = 0; t < threads; t++) pthread_join(tid[(size_t)t], nullptr);
    for (int w = 0; w < waves; w++) pthread_barrier_destroy(&wv[(size_t)w].bar);
    pthread_barrier_destroy(&blk.bar);
    pthread_attr_destroy(&attr);
}

}  // namespace

extern "C" {

/* sizeof(aacg_dev_unit), sizeof(aacg_refresh_map), AACG_CARRY_THREADS: what the test lays its arrays out by */
void emu_carry_sizes(uint32_t out[3]) { out[0] = (uint32_t)sizeof(aacg_dev_unit); out[1] = (uint32_t)sizeof(aacg_refresh_map); out[2] = AACG_CARRY_THREADS; }

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order), over
 * units[n_units] / map[n_units] and the entries W[n_slots x C], with the batch serial `serial`. */
void emu_carry(aacg_dev_unit* units, const aacg_refresh_map* map, uint32_t n_units, uint32_t* W, uint32_t n_slots, uint32_t C, uint32_t serial,
               uint32_t blocks, int reverse)
{
    aacg_carry_args A;
    A.units = units; A.map = map; A.W = W; A.n_units = n_units; A.n_slots = n_slots; A.C = C; A.serial = serial;
    for (uint32_t b = 0; b < blocks; b++) run_block(A, blocks, (int)(reverse ? blocks - 1 - b : b));
}

uint32_t emu_carry_entry(uint32_t before, uint32_t after, uint32_t serial) { return aacg_carry_word(before, after, serial); }
uint32_t emu_carry_now(uint32_t word) { return aacg_carry_now(word); }

}  // extern "C"
