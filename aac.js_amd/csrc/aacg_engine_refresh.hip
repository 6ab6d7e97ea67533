/*
 * aacg_engine_refresh.hip — a plan's unit records rewritten on the device from what aacg_parse_device produced
 * (aacg_plan_refresh_from_parse, include/aacgpu.h).  The run tables of a plan only depend on which streams bring
 * how many frames of which element layout; consecutive batches of the same streams share them.  What changes from
 * batch to batch is what the parser found per frame — window sequence and shape, max_sfb, grouping, flags — and that
 * never has to visit the host: one lane per unit copies it from the parser's record into the plan's device record,
 * keeps the planner's part (stream, PCM offset, channel layout), derives the group-of-window map, and turns a frame
 * the parser refused into a silent one (ONLY_LONG, max_sfb 0), counting it.
 *
 * Round 6: plan unit i need not be parsed record i.  With a map (aacg_refresh_map, include/aacgpu.h) a plan lists only the
 * elements its streams really have — streams of different element layouts in one batch (SCE + CPE + CPE + LFE beside plain
 * stereo; decoder.js:233-247 walks whatever elements a frame brings) — and says for each where the parser put it and how many
 * elements its frame must have; a frame with another count is not the frame the plan was made for and goes silent as a whole.
 */
#include <hip/hip_runtime.h>

#include "aacg_units_refresh.h"

/* (the body: aacg_units_refresh.h, which tests/emu/refresh_emu.cpp runs lane by lane on the CPU) */
extern "C" __global__ __launch_bounds__(AACG_REFRESH_THREADS)
void aacg_units_refresh(aacg_dev_unit* units, const aacg_unit_desc* parsed, aacg_parse_result* results, const aacg_refresh_map* map,
                        uint32_t n_units, uint32_t max_units, int refuse_pns, int keep_tns, uint32_t* refused)
{
    const aacg_refresh_args A = {units, parsed, results, map, n_units, max_units, refuse_pns, keep_tns, refused};
    aacg_pipe::refresh_body(A, blockDim.x);
}

void aacg_refresh_launch(aacg_dev_unit* units, const aacg_unit_desc* parsed, aacg_parse_result* results, const aacg_refresh_map* map, uint32_t n_units,
                         uint32_t max_units, int refuse_pns, int keep_tns, uint32_t* refused, hipStream_t s)
{
    hipLaunchKernelGGL(aacg_units_refresh, dim3((n_units + AACG_REFRESH_THREADS - 1u) / AACG_REFRESH_THREADS), dim3(AACG_REFRESH_THREADS), 0, s, units, parsed, results, map, n_units, max_units, refuse_pns, keep_tns, refused);
}
