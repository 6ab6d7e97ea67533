/*
 * map_emu.cpp — the resident batch's refresh-map kernel source (aac.js_amd/csrc/aacg_pipe_map.h: map_body) run lane by lane on
 * CPU threads (tests/emu/devport_emu.h), next to the host planner's own listing of the same map (aacg_pipe::plan_list), for
 * tests/test_pipe_map_emu.py, which compiles it into a library of its own.  TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_pipe_map.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* A batch of n_streams streams: layouts (n[s], kept[s], nch[8 s .. 8 s + 7]), slots, frames_of; channels C, parser block stride Cp,
 * elements per frame U.  host_map / dev_map: room for max_units entries each (dev_map is written over whatever it holds: the
 * caller poisons it); units (optional): room for max_units unit records.  Returns the plan's unit count (the host planner's),
 * or -1 if it exceeds max_units. */
int emu_pipe_map(const uint8_t* n, const uint8_t* kept, const uint8_t* nch, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams,
                 uint32_t C, uint32_t Cp, uint32_t U, uint32_t blocks, uint32_t max_units,
                 aacg_refresh_map* host_map, aacg_refresh_map* dev_map, aacg_unit_desc* units, aacg_pipe_stream* table)
{
    std::vector<aacg_pipe_layout> lay(n_streams);
    for (uint32_t s = 0; s < n_streams; s++) { lay[s].n = n[s]; lay[s].kept = kept[s]; std::memcpy(lay[s].nch, nch + 8 * s, 8); }
    std::vector<aacg_unit_desc> u;
    std::vector<aacg_refresh_map> m;
    const uint32_t n_units = aacg_pipe::plan_list(lay.data(), slots, frames_of, n_streams, C, Cp, U, &u, &m, table);
    if (n_units > max_units || u.size() != n_units || m.size() != n_units) return -1;
    std::memcpy(host_map, m.data(), m.size() * sizeof(aacg_refresh_map));
    if (units) std::memcpy(units, u.data(), u.size() * sizeof(aacg_unit_desc));
    /* workgroups of AACG_PIPE_MAP_THREADS lanes (one wave), as hipLaunchKernelGGL(aacg_pipe_map, blocks, 64) runs them */
    emu_launch((int)blocks, AACG_PIPE_MAP_THREADS, 0, EMU_BLOCKS_FORWARD, [&] { aacg_pipe::map_body(table, n_streams, U, dev_map, blocks); });
    return (int)n_units;
}

}  // extern "C"
