/*
 * shape_emu.cpp — the shaping kernel's source (aac.js_amd/csrc/aacg_plan_shape.h: shape_body) run lane by lane on CPU threads
 * (tests/emu/devport_emu.h), next to what the host planner makes of the same batch (aacg_pipe::plan_list's units through
 * aacg_plan_build, with the same rotation state), and the engine's own per-shape arithmetic (aacg_shape.cpp), for
 * tests/test_plan_shape_emu.py, which compiles it into a library of its own.  TESTS ONLY.
 */
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_plan_shape.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

namespace {

std::string g_err;

}  // namespace

extern "C" {

const char* emu_shape_error(void) { return g_err.c_str(); }

/* sizes of the records the test compares byte for byte */
void emu_shape_sizes(uint32_t out[5])
{
    out[0] = sizeof(aacg_dev_unit); out[1] = sizeof(aacg_run); out[2] = sizeof(aacg_rv_link); out[3] = sizeof(aacg_refresh_map); out[4] = sizeof(aacg_shape_stream);
}

void emu_shape_capacity(uint32_t max_streams, uint32_t max_frames, uint32_t max_elems, uint32_t channels, uint64_t out[4])
{
    const aacg_shape_limits lim = aacg_shape_capacity(max_streams, max_frames, max_elems, channels);
    out[0] = lim.max_units; out[1] = lim.max_runs; out[2] = lim.max_links; out[3] = lim.max_elems;
}

int emu_shape_same(const aacg_shape_stream* a, uint32_t na, const aacg_shape_stream* b, uint32_t nb) { return aacg_shape_same(a, na, b, nb) ? 1 : 0; }

/* A batch of n_streams streams — layouts (n[s], kept[s], nch[8 s .. 8 s + 7]), slots, frames_of — on an engine of n_slots slots x C
 * channels whose rotation state is parity[n_slots * C]; parser block stride Cp, elements per frame U; the shaped plan's limits
 * (lim_streams, lim_frames, lim_elems).
 *   host_*: what aacg_plan_build makes of aacg_pipe::plan_list's units (room for cap[0] units / cap[1] runs each);
 *   dev_*:  what shape_body writes, over whatever the buffers hold (the caller poisons them);
 *   table:  the completed per-stream table; figures[0..7] the host planner's n_units, n_runs, n_links, zero_fill, wide_frames,
 *           long_chains, pcm_floats, n_chains, figures[8..15] the same from aacg_shape_plan; chains_host / chains_dev: five
 *           words per chain (stream, channel, n_ch, parity[0], parity[1]).
 * Returns 0; the error of aacg_shape_plan (< 0: nothing was run, nothing written); 1 if the host planner failed; 2 if the
 * buffers are too small. */
int emu_plan_shape(const uint8_t* n, const uint8_t* kept, const uint8_t* nch, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams,
                   uint32_t n_slots, uint32_t C, uint32_t Cp, uint32_t U, const uint8_t* parity, uint32_t blocks,
                   uint32_t lim_streams, uint32_t lim_frames, uint32_t lim_elems, const uint64_t cap[2],
                   aacg_dev_unit* host_units, aacg_run* host_runs, aacg_rv_link* host_links, aacg_refresh_map* host_map,
                   aacg_dev_unit* dev_units, aacg_run* dev_runs, aacg_rv_link* dev_links, aacg_refresh_map* dev_map,
                   aacg_shape_stream* table, uint64_t figures[16], uint32_t* chains_host, uint32_t* chains_dev)
{
    std::vector<aacg_pipe_layout> lay(n_streams);
    for (uint32_t s = 0; s < n_streams; s++) { lay[s].n = n[s]; lay[s].kept = kept[s]; std::memcpy(lay[s].nch, nch + 8 * s, 8); }
    /* the engine's side first: a shape it refuses is not run */
    const aacg_shape_limits lim = aacg_shape_capacity(lim_streams, lim_frames, lim_elems, C);
    std::vector<aacg_shape_stream> tab(n_streams);
    aacg_pipe::shape_table(lay.data(), slots, frames_of, n_streams, tab.data());
    aacg_shape_info info;
    const int src = aacg_shape_plan(tab.data(), n_streams, n_slots, C, Cp, parity, lim, &info, &g_err);
    if (src) return src;
    std::memcpy(table, tab.data(), tab.size() * sizeof(aacg_shape_stream));
    /* the host planner */
    std::vector<aacg_unit_desc> u;
    std::vector<aacg_refresh_map> m;
    const uint32_t n_units = aacg_pipe::plan_list(lay.data(), slots, frames_of, n_streams, C, Cp, U, &u, &m, nullptr);
    aacg_plan_host h;
    if (n_units && aacg_plan_build(u.data(), n_units, 3, (int)n_slots, (int)C, parity, &h, &g_err)) return 1;
    if (h.units.size() > cap[0] || h.runs_rv.size() > cap[1] || info.n_units > cap[0] || info.n_runs > cap[1]) return 2;
    std::memcpy(host_units, h.units.data(), h.units.size() * sizeof(aacg_dev_unit));
    std::memcpy(host_runs, h.runs_rv.data(), h.runs_rv.size() * sizeof(aacg_run));
    std::memcpy(host_links, h.links_rv.data(), h.links_rv.size() * sizeof(aacg_rv_link));
    std::memcpy(host_map, m.data(), m.size() * sizeof(aacg_refresh_map));
    const uint64_t fh[8] = {h.units.size(), h.runs_rv.size(), h.n_links_rv, h.zero_fill, h.wide_frames, h.long_chains, h.pcm_floats, h.chains.size()};
    const uint64_t fd[8] = {info.n_units, info.n_runs, info.n_links, info.zero_fill, info.wide_frames, info.long_chains, info.pcm_floats, info.chains.size()};
    std::memcpy(figures, fh, sizeof fh);
    std::memcpy(figures + 8, fd, sizeof fd);
    for (size_t k = 0; k < h.chains.size(); k++) { const aacg_chain& c = h.chains[k]; const uint32_t w[5] = {c.stream, c.channel, c.n_ch, c.parity[0], c.parity[1]}; std::memcpy(chains_host + 5 * k, w, sizeof w); }
    for (size_t k = 0; k < info.chains.size(); k++) { const aacg_chain& c = info.chains[k]; const uint32_t w[5] = {c.stream, c.channel, c.n_ch, c.parity[0], c.parity[1]}; std::memcpy(chains_dev + 5 * k, w, sizeof w); }
    /* the kernel */
    aacg_shape_args A;
    std::memset(&A, 0, sizeof A);
    A.tab = table; A.n_streams = n_streams; A.U = U; A.C = C; A.Cp = Cp; A.n_runs = info.n_runs; A.unit0_coef = info.unit0_coef; A.unit0_nch = info.unit0_nch;
    A.map = dev_map; A.units = dev_units; A.runs = dev_runs; A.links = dev_links;
    /* workgroups of AACG_SHAPE_THREADS lanes (one wave), as hipLaunchKernelGGL(aacg_plan_shape, blocks, 64) runs them */
    emu_launch((int)blocks, AACG_SHAPE_THREADS, 0, EMU_BLOCKS_FORWARD, [&] { aacg_pipe::shape_body(A, blocks); });
    return 0;
}

}  // extern "C"
