/*
 * exit_trim_emu.cpp — the resident route's way out as data (aac.js_amd/csrc/aacg_pipe_exit.h) with the fields and the seventh stage the
 * trim added, behind a flat C interface, for tests/test_pipe_exit_trim.py, which compiles it into a library of its own.
 * tests/emu/exit_emu.cpp, tests/emu/exit_features_emu.cpp and tests/emu/exit_limit_emu.cpp stay the drivers of the fields that were there
 * before.  Host code only: nothing is emulated.  TESTS ONLY.
 */
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pipe_exit.h"

extern "C" {

/* pipe: C, O, resampled, elem, max_streams, max_frames, lane_elems, n_mels, ft_lane_elems, limited, trimmed;
 * batch: n, n_streams, longest, dest, stride_frames, rs_most, rs_total, ft_most, ft_total, tr_most, tr_total */
static aacg_exit_pipe pipe_of(const uint64_t* v)
{
    aacg_exit_pipe P = {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]};
    P.n_mels = (uint32_t)v[7]; P.ft_lane_elems = v[8]; P.limited = (uint32_t)v[9]; P.trimmed = (uint32_t)v[10];
    return P;
}
static aacg_exit_batch batch_of(const uint64_t* v)
{
    aacg_exit_batch B = {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]};
    B.ft_most = (uint32_t)v[7]; B.ft_total = v[8]; B.tr_most = (uint32_t)v[9]; B.tr_total = v[10];
    return B;
}

/* out: n_stages, row, xform_bytes, out_bytes, device_need, collect_copy, ft_row, then (what, src, dst, tail, bytes) for each of the seven
 * stage entries, used or not: 42 words */
void emu_exit_plan(const uint64_t* pipe, const uint64_t* batch, uint64_t* out)
{
    const aacg_exit_plan X = aacg_pipe::exit_plan(pipe_of(pipe), batch_of(batch));
    out[0] = X.n_stages; out[1] = X.row; out[2] = X.xform_bytes; out[3] = X.out_bytes; out[4] = X.device_need; out[5] = X.collect_copy; out[6] = X.ft_row;
    for (int i = 0; i < 7; i++) {
        const aacg_exit_stage& S = X.stage[i];
        uint64_t* o = out + 7 + 5 * i;
        o[0] = S.what; o[1] = S.src; o[2] = S.dst; o[3] = S.tail; o[4] = S.bytes;
    }
}

uint64_t emu_exit_host_capacity(const uint64_t* pipe) { return aacg_pipe::exit_host_capacity(pipe_of(pipe)); }

/* A device batch's pure refusals, as tests/emu/exit_emu.cpp's */
int emu_exit_check(const uint64_t* pipe, const uint64_t* batch, uint64_t d_pcm, uint64_t d_pcm_bytes, int32_t layout, uint32_t planar_items,
                   int* late, char* text, uint32_t cap)
{
    const aacg_exit_pipe P = pipe_of(pipe);
    aacg_exit_batch B = batch_of(batch);
    B.dest = aacg_pipe::exit_dest_device(layout);
    const aacg_pcm_device_out out = {(void*)(uintptr_t)d_pcm, (size_t)d_pcm_bytes, layout, B.stride_frames};
    const aacg_exit_refusal no = aacg_pipe::exit_check(P, B, aacg_pipe::exit_plan(P, B), out, planar_items);
    *late = no.late ? 1 : 0;
    std::strncpy(text, no.text.c_str(), cap);
    if (cap) text[cap - 1] = 0;
    return no.code;
}

}  // extern "C"
