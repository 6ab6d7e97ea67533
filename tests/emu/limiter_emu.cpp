/*
 * limiter_emu.cpp — the limiter's source (aac.js_amd/csrc/aacg_pcm_limit.h: limit_body, the body the host's switch would launch) run
 * lane by lane on CPU threads (tests/emu/devport_emu.h, tests/emu/devport_limit_emu.h) over packed PCM buffers, per-stream records and a
 * state block that the test made, for tests/test_pcm_limiter_emu.py, which compiles it into a library of its own and applies the rule
 * in numpy float32.  TESTS ONLY.
 */
#include <cstdint>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_limit.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, streams of one, bytes of a stream's record, floats in front of a
 * state buffer's held block, samples of a block */
void emu_limit_sizes(uint32_t out[5])
{
    out[0] = AACG_LIMIT_THREADS; out[1] = AACG_LIMIT_WAVES; out[2] = (uint32_t)sizeof(aacg_limit_stream); out[3] = AACG_LIMIT_STATE_HEAD; out[4] = AACG_LIMIT_BLOCK;
}

/* One launch of `blocks` workgroups, run in the order given by `reverse` (workgroups of a launch run in any order).  Returns 0 if no
 * body serves the launch. */
int emu_limit(const void* src, void* dst, const void* rec, uint32_t n_streams, float* state, float ceiling, float release,
              uint32_t channels, uint32_t elem, uint32_t blocks, int reverse)
{
    if (!n_streams || !blocks || !aacg_limit_config_ok(ceiling, release)) return 0;
    aacg_limit_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_limit_stream*)rec; A.state = state; A.n_streams = n_streams; A.n_frames = 0;
    for (uint32_t k = 0; k < n_streams; k++) A.n_frames += A.rec[k].frames;
    A.ceiling = ceiling; A.release = release; A.channels = channels; A.elem = elem;
    int ran = 0;
    /* the body the host's switch picks (aacg_limit_launch), in workgroups of four waves, no LDS */
#define EMU_LIMIT_RUN(T, NAME, C) \
    if (elem == sizeof(T) && channels == C) { ran = 1; emu_launch((int)blocks, AACG_LIMIT_THREADS, 0, reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD, [&] { aacg_pipe::limit_body<T, C>(A, blocks); }); }
    AACG_LIMIT_BODIES(EMU_LIMIT_RUN)
    return ran;
}

}  // extern "C"
