/*
 * half_emu.cpp — the lane emulator (tests/emu/emu_lib.cpp, unchanged) with its rendezvous run kernels of f32 PCM on the
 * eight-wave run body (imdct_run_body<..., NW = AACG_HALF_WAVES>, the body behind aacg_imdct_run_quant_rv), for
 * tests/test_half_runs_emu.py and tests/test_schedules_emu.py: compiled (with tests/emu/devport_emu.h) into a library of its
 * own, libaacg_emu_half.so (tests/emu/Makefile).  TESTS ONLY.
 * The emulator launches every run kernel with sixteen waves; here waves 0..7 run the eight-wave body, each taking two frames of
 * the run, and waves 8..15 take part in its one workgroup barrier and leave, so the body sees eight working waves and touches
 * no LDS beyond AACG_HALF_LDS_BYTES.  Every other kernel is the emulator's own.
 * Built as the profiling build (AACG_PROFILE): emu_half_set_ablate sets the work-skipping switches (AACG_ABL) the eight-wave
 * body then sees, so that its profiling paths are emulated too; 0, the default, is the library that ships.
 */
#define AACG_PROFILE
#define AACG_EMU_SCHEDULER              /* devport_emu.h: emu_lib.cpp, included below, has the schedule controller */
#include "../../aac.js_amd/csrc/aacg_kernels.h"

namespace half_emu {

int g_ablate = 0;

template <int KIND, int OUT = AACG_OUTPUT_F32, bool DD = false, bool EX = false, bool CPL = false, bool RV = false, bool NTL = false>
void run_body(const aacg_kparams& P, const aacg_rv_args* V = nullptr)
{
    if constexpr (RV && !DD && !EX && !CPL && OUT == AACG_OUTPUT_F32) {
        if (dp_wave() >= AACG_HALF_WAVES) { dp_block_sync_lds(); return; }
        aacg_kparams Q = P;
        Q.ablate = g_ablate;
        imdct_run_body<KIND, OUT, false, false, false, true, NTL, false, AACG_HALF_WAVES>(Q, V);
    } else {
        imdct_run_body<KIND, OUT, DD, EX, CPL, RV, NTL>(P, V);
    }
}

}  // namespace half_emu

#define imdct_run_body half_emu::run_body
#include "emu_lib.cpp"

extern "C" void emu_half_set_ablate(int bits) { half_emu::g_ablate = bits; }
