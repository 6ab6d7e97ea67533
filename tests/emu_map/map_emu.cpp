/*
 * map_emu.cpp — the resident batch's refresh-map kernel source (aac.js_amd/csrc/aacg_pipe_map.h: map_body) run lane by lane on
 * CPU threads (tests/emu/devport_emu.h), next to the host planner's own listing of the same map (aacg_pipe::plan_list), for
 * tests/test_pipe_map_emu.py, which compiles it into a library of its own.  TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_pipe_map.h"

thread_local emu_lane_ctx g_emu;

namespace {

struct lane_arg { emu_lane_ctx ctx; const aacg_pipe_stream* tab; uint32_t n_streams, U, blocks; aacg_refresh_map* map; };

void* lane_main(void* p)
{
    lane_arg* a = (lane_arg*)p;
    g_emu = a->ctx;
    aacg_pipe::map_body(a->tab, a->n_streams, a->U, a->map, a->blocks);
    return nullptr;
}

/* one workgroup of AACG_PIPE_MAP_THREADS lanes (one wave), as hipLaunchKernelGGL(aacg_pipe_map, blocks, 64) runs it */
void run_block(const aacg_pipe_stream* tab, uint32_t n_streams, uint32_t U, aacg_refresh_map* map, uint32_t blocks, int block)
{
    const int threads = AACG_PIPE_MAP_THREADS, waves = threads / 64;
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
        args[(size_t)t] = lane_arg{emu_lane_ctx{t & 63, t >> 6, &wv[(size_t)(t >> 6)], &blk}, tab, n_streams, U, blocks, map};
        pthread_create(&tid[(size_t)t], &attr, lane_main, &args[(size_t)t]);
    }
    for (int t = 0; t < threads; t++) pthread_join(tid[(size_t)t], nullptr);
    for (int w = 0; w < waves; w++) pthread_barrier_destroy(&wv[(size_t)w].bar);
    pthread_barrier_destroy(&blk.bar);
    pthread_attr_destroy(&attr);
}

}  // namespace

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
    for (uint32_t b = 0; b < blocks; b++) run_block(table, n_streams, U, dev_map, blocks, (int)b);
    return (int)n_units;
}

}  // extern "C"
