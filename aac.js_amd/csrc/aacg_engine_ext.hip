/*
 * aacg_engine_ext.hip — the run kernel's variants (see aacg_engine.hip): separate translation unit, separate
 * code object.  MI355X (gfx950) only.
 */
#include <hip/hip_runtime.h>

#include "aacg_kernels.h"
#include "aacg_routes.h"

/* Variants of aacg_imdct_run_quant / _f32:
 *   _dd : plans with full later runs (chains longer than 16 frames), whose first wave does double duty;
 * (the optional TNS / PNS stages are a kernel of their own, aacg_engine_spectral.hip) */
AACG_RUN_KERNEL_UNIT(ext, AACG_RUN_KERNELS_EXT)
