/*
 * aacg_engine_rv.hip — the run kernels for plans whose chains are longer than a run, WITHOUT a recomputed frame: the
 * runs of a chain hand their tails over through a rendezvous cell in global memory (aacg_rv_args; AACG_RK_RV).
 * Their own translation unit and code object, like the other variants.  MI355X (gfx950) only.
 */
#include <hip/hip_runtime.h>

#include "aacg_kernels.h"
#include "aacg_routes.h"

/* the headline kernel runs 16 frames on eight waves, two workgroups per CU (AACG_HALF_WAVES, aacg_device.h); the _nt ones are for
 * batches of multichannel frames: non-temporal loads of the spectra (aacg_engine_nt.hip says why) */
AACG_RUN_KERNEL_UNIT(rv, AACG_RUN_KERNELS_RV)
