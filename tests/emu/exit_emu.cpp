/*
 * exit_emu.cpp — the resident route's way out as data (aac.js_amd/csrc/aacg_pipe_exit.h: exit_plan, exit_check, the capacities) behind a
 * flat C interface, for tests/test_pipe_exit_plan.py, which compiles it into a library of its own.  Host code only: nothing is emulated.
 * TESTS ONLY.
 */
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pipe_exit.h"

extern "C" {

/* pipe: C, O, resampled, elem, max_streams, max_frames, lane_elems; batch: n, n_streams, longest, dest, stride_frames, rs_most, rs_total */
static aacg_exit_pipe pipe_of(const uint64_t* v) { return {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]}; }
static aacg_exit_batch batch_of(const uint64_t* v) { return {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5], v[6]}; }

/* out: n_stages, row, xform_bytes, out_bytes, device_need, collect_copy, then (what, src, dst, tail, bytes) for each of the four stage
 * entries, used or not: 26 words */
void emu_exit_plan(const uint64_t* pipe, const uint64_t* batch, uint64_t* out)
{
    const aacg_exit_plan X = aacg_pipe::exit_plan(pipe_of(pipe), batch_of(batch));
    out[0] = X.n_stages; out[1] = X.row; out[2] = X.xform_bytes; out[3] = X.out_bytes; out[4] = X.device_need; out[5] = X.collect_copy;
    for (int i = 0; i < 4; i++) {
        const aacg_exit_stage& S = X.stage[i];
        uint64_t* o = out + 6 + 5 * i;
        o[0] = S.what; o[1] = S.src; o[2] = S.dst; o[3] = S.tail; o[4] = S.bytes;
    }
}

uint64_t emu_exit_host_capacity(const uint64_t* pipe) { return aacg_pipe::exit_host_capacity(pipe_of(pipe)); }
uint64_t emu_exit_resample_most(uint32_t max_streams, uint32_t max_frames, uint32_t L, uint32_t M) { return aacg_pipe::exit_resample_most(max_streams, max_frames, L, M); }

/* A device batch's pure refusals: the plan is made as the pipeline makes it (the destination from the layout), then checked.  Returns
 * the code; *late and the text (cut to cap) as exit_check gives them */
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
