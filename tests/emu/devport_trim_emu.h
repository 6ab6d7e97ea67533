/*
 * devport_trim_emu.h — the CPU twin of devport.h's 16-byte streaming store of integers, included behind devport_emu.h.  TEST
 * INFRASTRUCTURE ONLY.
 *
 * dp_store_nt(dpi4*): the trim stage (aacg_pcm_trim.h) moves PCM elements as the bits they are, four words a vector.  dpi4 is aligned to
 * 16 bytes here, so a store to an address that is not shows under -fsanitize=undefined.
 */
#ifndef AACG_DEVPORT_TRIM_EMU_H
#define AACG_DEVPORT_TRIM_EMU_H

DP_DEVICE void dp_store_nt(dpi4* p, dpi4 v) { *p = v; }

#endif
