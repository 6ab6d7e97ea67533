/*
 * aacg_run_kernels.h — the registry of run kernels: every instantiation of imdct_run_body (aacg_kernels.h) is ONE row here.
 *
 * A kernel's key is its set of switches (AACG_RK_*); its symbol is "aacg_imdct_run_" + the row's suffix, which must be what
 * aacg_run_kernel_name composes from the key (tests/test_routes.py).  Each translation unit that defines run kernels expands
 * its own list with AACG_RUN_KERNEL_UNIT: the kernels, then its table of them for the engine (aacg_find_run_kernel).  The units
 * are separate code objects so that adding one variant never moves another's code.  tests/emu/emu_lib.cpp expands every row
 * into the lane emulator's switch, and tests/test_kernel_resources.py reads the rows for each kernel's resource budget.  A new
 * variant is one row here (and a recipe in tests/test_route_matrix.py that reaches it).
 *
 * A row:  X(suffix, key, waves, args)
 *   waves  AACG_WG_WAVES (16 waves, one workgroup per CU) or AACG_HALF_WAVES (the eight-wave body: two workgroups per CU,
 *          bounded to 128 VGPRs)
 *   args   the kernel's signature:
 *          P    (const aacg_kparams P)
 *          PV   (const aacg_kparams P, const aacg_rv_args V): the rendezvous kernels
 *          PRE  the rendezvous kernels whose early pointers are preloaded: six leading pointer arguments (run table, tables,
 *               links, units, spectra, band words) that arrive in SGPRs with the wave (-amdgpu-kernarg-preload-count), then the
 *               two argument records.  By-value struct arguments are not preloaded, so the pointers a wave needs for its first
 *               loads travel once more as leading scalar arguments — the table loads and the run record's batch go out with
 *               the wave's first instructions, one dependent round trip earlier (0.2 us per launch on the headline route).
 */
#ifndef AACG_RUN_KERNELS_H
#define AACG_RUN_KERNELS_H

#include "aacg_device.h"

/* template switches of imdct_run_body = key of a run kernel */
enum {
    AACG_RK_QUANT = 1,      /* KIND = AACG_INPUT_QUANT_I16 (else f32 spectra) */
    AACG_RK_I16   = 2,      /* OUT = AACG_OUTPUT_I16 */
    AACG_RK_DD    = 4,      /* double duty: the first wave of a full later run recomputes the frame before it */
    AACG_RK_EX    = 8,      /* the optional stages (AACG_TNS_SPEC, AACG_PNS_SPEC) inside the run */
    AACG_RK_CPL   = 16,     /* independent coupling applied where the target's PCM is formed */
    AACG_RK_RV    = 32,     /* rendezvous cells between the runs of a chain (and, pipelined, between launches); takes aacg_rv_args */
    AACG_RK_NT    = 64      /* non-temporal loads of the spectra: batches of multichannel frames */
};

/* aacg_engine.hip */
#define AACG_RUN_KERNELS_PLAIN(X) \
    X(quant,            AACG_RK_QUANT,                                       AACG_WG_WAVES,   P) \
    X(f32,              0,                                                   AACG_WG_WAVES,   P)
/* aacg_engine_rv.hip; the headline kernel first */
#define AACG_RUN_KERNELS_RV(X) \
    X(quant_rv,         AACG_RK_QUANT | AACG_RK_RV,                          AACG_HALF_WAVES, PRE) \
    X(f32_rv,           AACG_RK_RV,                                          AACG_WG_WAVES,   PRE) \
    X(quant_rv_nt,      AACG_RK_QUANT | AACG_RK_RV | AACG_RK_NT,             AACG_WG_WAVES,   PRE) \
    X(f32_rv_nt,        AACG_RK_RV | AACG_RK_NT,                             AACG_WG_WAVES,   PRE)
/* aacg_engine_nt.hip */
#define AACG_RUN_KERNELS_NT(X) \
    X(quant_nt,         AACG_RK_QUANT | AACG_RK_NT,                          AACG_WG_WAVES,   P) \
    X(f32_nt,           AACG_RK_NT,                                          AACG_WG_WAVES,   P)
/* aacg_engine_ext.hip */
#define AACG_RUN_KERNELS_EXT(X) \
    X(quant_dd,         AACG_RK_QUANT | AACG_RK_DD,                          AACG_WG_WAVES,   P) \
    X(f32_dd,           AACG_RK_DD,                                          AACG_WG_WAVES,   P)
/* aacg_engine_i16.hip */
#define AACG_RUN_KERNELS_I16(X) \
    X(quant_i16,        AACG_RK_QUANT | AACG_RK_I16,                         AACG_WG_WAVES,   P) \
    X(f32_i16,          AACG_RK_I16,                                         AACG_WG_WAVES,   P) \
    X(quant_dd_i16,     AACG_RK_QUANT | AACG_RK_DD | AACG_RK_I16,            AACG_WG_WAVES,   P) \
    X(f32_dd_i16,       AACG_RK_DD | AACG_RK_I16,                            AACG_WG_WAVES,   P) \
    X(quant_i16_nt,     AACG_RK_QUANT | AACG_RK_I16 | AACG_RK_NT,            AACG_WG_WAVES,   P) \
    X(f32_i16_nt,       AACG_RK_I16 | AACG_RK_NT,                            AACG_WG_WAVES,   P) \
    X(quant_rv_i16,     AACG_RK_QUANT | AACG_RK_RV | AACG_RK_I16,            AACG_WG_WAVES,   PV) \
    X(f32_rv_i16,       AACG_RK_RV | AACG_RK_I16,                            AACG_WG_WAVES,   PV) \
    X(quant_rv_i16_nt,  AACG_RK_QUANT | AACG_RK_RV | AACG_RK_I16 | AACG_RK_NT, AACG_WG_WAVES, PV) \
    X(f32_rv_i16_nt,    AACG_RK_RV | AACG_RK_I16 | AACG_RK_NT,               AACG_WG_WAVES,   PV)
/* aacg_engine_exrun.hip */
#define AACG_RUN_KERNELS_EXRUN(X) \
    X(quant_ex,         AACG_RK_QUANT | AACG_RK_EX,                          AACG_WG_WAVES,   P) \
    X(f32_ex,           AACG_RK_EX,                                          AACG_WG_WAVES,   P) \
    X(quant_ex_rv,      AACG_RK_QUANT | AACG_RK_EX | AACG_RK_RV,             AACG_WG_WAVES,   PV) \
    X(f32_ex_rv,        AACG_RK_EX | AACG_RK_RV,                             AACG_WG_WAVES,   PV)
/* aacg_engine_couple.hip */
#define AACG_RUN_KERNELS_COUPLE(X) \
    X(quant_cpl,        AACG_RK_QUANT | AACG_RK_CPL,                         AACG_WG_WAVES,   P) \
    X(f32_cpl,          AACG_RK_CPL,                                         AACG_WG_WAVES,   P) \
    X(quant_cpl_nt,     AACG_RK_QUANT | AACG_RK_CPL | AACG_RK_NT,            AACG_WG_WAVES,   P) \
    X(f32_cpl_nt,       AACG_RK_CPL | AACG_RK_NT,                            AACG_WG_WAVES,   P)

/* every list with the name of the table its unit exports (aacg_run_kernels_<set>, aacg_run_kernels_<set>_n) */
#define AACG_RUN_KERNEL_SETS(X) \
    X(plain, AACG_RUN_KERNELS_PLAIN) X(rv, AACG_RUN_KERNELS_RV) X(nt, AACG_RUN_KERNELS_NT) X(ext, AACG_RUN_KERNELS_EXT) \
    X(i16, AACG_RUN_KERNELS_I16) X(exrun, AACG_RUN_KERNELS_EXRUN) X(couple, AACG_RUN_KERNELS_COUPLE)

/* the key as imdct_run_body's leading template arguments <KIND, OUT, DD, EX, CPL, RV, NTL> (PRE and NW follow them) */
#define AACG_RUN_BODY_ARGS(key) \
    (((key) & AACG_RK_QUANT) ? AACG_INPUT_QUANT_I16 : AACG_INPUT_SPEC_F32), (((key) & AACG_RK_I16) ? AACG_OUTPUT_I16 : AACG_OUTPUT_F32), \
    (((key) & AACG_RK_DD) != 0), (((key) & AACG_RK_EX) != 0), (((key) & AACG_RK_CPL) != 0), (((key) & AACG_RK_RV) != 0), (((key) & AACG_RK_NT) != 0)

struct aacg_run_kernel {
    unsigned    key;        /* AACG_RK_* */
    const char* name;       /* the symbol a rocprofv3 kernel trace shows */
    const void* fn;         /* host stub, for hipLaunchKernel */
    bool        preloaded;  /* the PRE signature */
    unsigned    threads;    /* workgroup size it is launched with */
};

#define AACG_RUN_KERNEL_EXTERN(set, ROWS) extern const aacg_run_kernel aacg_run_kernels_##set[]; extern const int aacg_run_kernels_##set##_n;
AACG_RUN_KERNEL_SETS(AACG_RUN_KERNEL_EXTERN)
#undef AACG_RUN_KERNEL_EXTERN

/* In a translation unit of run kernels: its kernels, then its table. */
#define AACG_RUN_KERNEL_UNIT(set, ROWS) \
    ROWS(AACG_RUN_KERNEL) \
    const aacg_run_kernel aacg_run_kernels_##set[] = { ROWS(AACG_RUN_KERNEL_ENTRY) }; \
    const int aacg_run_kernels_##set##_n = sizeof aacg_run_kernels_##set / sizeof aacg_run_kernels_##set[0];

#define AACG_RUN_KERNEL(suffix, key, waves, args) AACG_RUN_KERNEL_##args(aacg_imdct_run_##suffix, key, waves, AACG_RUN_BOUNDS_##waves)
#define AACG_RUN_KERNEL_ENTRY(suffix, key, waves, args) \
    {key, "aacg_imdct_run_" #suffix, (const void*)aacg_imdct_run_##suffix, AACG_RUN_PRELOADED_##args, (waves) * 64},

/* 1024 threads = 16 waves, one workgroup per CU: 4 waves per SIMD -> 128 VGPRs per lane.  Eight waves: bounded so that the kernel
 * keeps to 128 VGPRs all the same — four waves per SIMD, two workgroups per CU with its 80 KiB of LDS. */
#define AACG_RUN_BOUNDS_AACG_WG_WAVES   __launch_bounds__(AACG_WG_THREADS)
#define AACG_RUN_BOUNDS_AACG_HALF_WAVES __launch_bounds__(AACG_HALF_WAVES * 64, 4)

#define AACG_RUN_PRELOADED_P   false
#define AACG_RUN_PRELOADED_PV  false
#define AACG_RUN_PRELOADED_PRE true

#define AACG_RUN_KERNEL_P(name, key, waves, bounds) \
    static_assert(!((key) & AACG_RK_RV), #name ": a rendezvous kernel takes aacg_rv_args"); \
    extern "C" __global__ bounds void name(const aacg_kparams P) { imdct_run_body<AACG_RUN_BODY_ARGS(key), false, waves>(P); }
#define AACG_RUN_KERNEL_PV(name, key, waves, bounds) \
    static_assert(((key) & AACG_RK_RV) != 0, #name ": only a rendezvous kernel takes aacg_rv_args"); \
    extern "C" __global__ bounds void name(const aacg_kparams P, const aacg_rv_args V) { imdct_run_body<AACG_RUN_BODY_ARGS(key), false, waves>(P, &V); }
#define AACG_RUN_KERNEL_PRE(name, key, waves, bounds) \
    static_assert(((key) & AACG_RK_RV) != 0, #name ": only a rendezvous kernel takes aacg_rv_args"); \
    extern "C" __global__ bounds \
    void name(const aacg_run* runs, const aacg_tables* tab, const aacg_rv_link* links, const aacg_dev_unit* units, const void* coeffs, \
              const aacg_band_meta* meta, const aacg_kparams P, const aacg_rv_args V) \
    { imdct_run_body<AACG_RUN_BODY_ARGS(key), true, waves>(P, &V, runs, tab, links, units, coeffs, meta); }

#endif
