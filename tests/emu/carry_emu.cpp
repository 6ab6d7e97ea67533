/*
 * carry_emu.cpp — the window-shape carry kernel's source (aac.js_amd/csrc/aacg_shape_carry.h: carry_body) run lane by lane on CPU
 * threads (tests/emu/devport_emu.h) over unit records, a refresh map and the engine's per-channel entries that the test made, for
 * tests/test_shape_carry_emu.py, which compiles it into a library of its own and walks the rule in numpy.  TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_shape_carry.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

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
    /* workgroups of AACG_CARRY_THREADS lanes, as hipLaunchKernelGGL(aacg_units_carry_shape, blocks, AACG_CARRY_THREADS) runs them */
    emu_launch((int)blocks, AACG_CARRY_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::carry_body(A, blocks); });
}

uint32_t emu_carry_entry(uint32_t before, uint32_t after, uint32_t serial) { return aacg_carry_word(before, after, serial); }
uint32_t emu_carry_now(uint32_t word) { return aacg_carry_now(word); }

}  // extern "C"
