/*
 * aacg_engine_exrun.hip — the run kernels with the optional stages inside (AACG_RK_EX): noise bands
 * (AACG_PNS_SPEC) and TNS filters (AACG_TNS_SPEC) applied between dequantisation and IMDCT, in the wave's own slot.
 * Batches that carry TNS records or noise bands, produce f32 PCM, have no coupling elements and no chain longer than a
 * run's double-duty variant is needed for (with the filters in both copies of its front end that variant spilled 800
 * bytes per lane) run here in ONE launch; everything else with optional stages takes the staged route
 * (aacg_engine_spectral.hip).  A code object of its own,
 * so that the plain kernels of aacg_engine.hip never move.  MI355X (gfx950) only.
 */
#include <hip/hip_runtime.h>

#include "aacg_kernels.h"
#include "aacg_routes.h"

/* the _rv ones with chains that meet in rendezvous cells (aacg_engine_rv.hip): chains longer than a run without a staged route, and
 * launches through the pipeline that overlap */
AACG_RUN_KERNEL_UNIT(exrun, AACG_RUN_KERNELS_EXRUN)

static_assert(AACG_LDS_BYTES_QUANT_EX <= 160 * 1024, "the TNS exchange areas must fit beside the slots");
