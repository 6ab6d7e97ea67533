/*
 * walk_emu.cpp — the span walk's kernel source (aacg_parse.h: walk_body) run lane by lane on CPU threads, for
 * tests/test_parse_walk_emu.py, which compiles it (with tests/emu/devport_emu.h) into a library of its own.  TESTS ONLY.
 * Same arguments and outputs as aacg_parse_walk; the lane order is the launcher's: spans sorted by length, longest first, the
 * sorted 64-span pieces one per workgroup of one wave.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../aac.js_amd/csrc/aacg_parse.h"
#include "../../aac.js_amd/csrc/aacg_host.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

namespace {

std::string g_err;

}  // namespace

extern "C" {

const char* emu_walk_last_error() { return g_err.c_str(); }

int emu_walk(int sample_index, const aacg_code_entry* entries, const uint32_t* counts, const uint8_t* bytes, size_t n_bytes,
             const aacg_parse_frame* spans, uint32_t n_spans, uint32_t max_frames, uint32_t options,
             aacg_parse_frame* frames, aacg_walk_result* results)
{
    static aacg_parse_tables tab;
    int rc = aacg_parse_build_tables(sample_index, entries, counts, &tab, &g_err);
    if (rc) return rc;
    for (uint32_t s = 0; s < n_spans; s++)
        if ((size_t)spans[s].byte_offset + spans[s].byte_length > n_bytes) { g_err = "span outside the buffer"; return AACG_ERR_INVALID_ARG; }
    std::vector<uint32_t> padded((n_bytes + 15) / 16 * 4 + AACG_PARSE_PAD_BYTES / 4 + 4, 0u);
    std::memcpy(padded.data(), bytes, n_bytes);
    std::memset(frames, 0, (size_t)n_spans * max_frames * sizeof *frames);
    aacg_walk_params W;
    std::memset(&W, 0, sizeof W);
    W.P.bytes = padded.data(); W.P.frames = spans; W.P.tab = &tab; W.P.n_frames = n_spans; W.P.options = options;
    W.P.wg_threads = 64;
    W.blocks = frames; W.results = results; W.max_frames = max_frames;
    const uint32_t n_wg = (n_spans + 63) / 64;
    std::vector<uint32_t> sorted(n_spans), order((size_t)n_wg * 64, 0xffffffffu);
    for (uint32_t i = 0; i < n_spans; i++) sorted[i] = i;
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return spans[a].byte_length > spans[b].byte_length; });
    for (uint32_t pos = 0; pos < n_spans; pos++) order[pos] = sorted[pos];
    W.P.order = n_spans > 64 ? order.data() : nullptr;
    const size_t lds_bytes = AACG_PARSE_LDS_FIXED(tab.lut_words, 64);
    emu_launch((int)n_wg, (int)W.P.wg_threads, lds_bytes, EMU_BLOCKS_FORWARD, [&] { aacg_parse::walk_body(W); });
    return AACG_OK;
}

}  // extern "C"
