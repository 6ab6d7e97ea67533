/*
 * devport_truepeak_emu.h — the CPU twin of devport.h's atomic unsigned maximum in global memory, included behind devport_emu.h.
 * TEST INFRASTRUCTURE ONLY.
 *
 * dp_g_atomic_max_u32: the lanes of a workgroup are OS threads that run at once, so the maximum is a compare-and-swap loop on plain host
 * memory; workgroups run one after the other.  The device carries it out in the L2 in whatever order the requests arrive, and a maximum
 * is the same in any.
 */
#ifndef AACG_DEVPORT_TRUEPEAK_EMU_H
#define AACG_DEVPORT_TRUEPEAK_EMU_H

DP_DEVICE void dp_g_atomic_max_u32(unsigned* p, unsigned v)
{
    unsigned seen = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (seen < v && !__atomic_compare_exchange_n(p, &seen, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

#endif
