/*
 * aacg_engine_i16.hip — the run kernels for AACG_OUTPUT_I16 engines: the same bodies with the epilogue's stores
 * narrowed to int16 (round to nearest, saturating).  Their own translation unit, like the other variants, so that
 * the float32 kernels' code objects do not move.  MI355X (gfx950) only.
 */
#include <hip/hip_runtime.h>

#include "aacg_kernels.h"
#include "aacg_routes.h"

/* also for batches of multichannel frames: non-temporal loads of the spectra (_nt, aacg_engine_nt.hip says why); and for chains
 * that meet in rendezvous cells — between the runs of a launch and between consecutive launches (_rv, aacg_engine_rv.hip) */
AACG_RUN_KERNEL_UNIT(i16, AACG_RUN_KERNELS_I16)
