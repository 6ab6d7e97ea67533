/*
 * devport_conceal_emu.h — the CPU twin of devport.h's dp_wave_first, included behind devport_emu.h.  TEST INFRASTRUCTURE ONLY.
 *
 * dp_wave_first: the wave's 64 lanes put their predicate into the emulator's shuffle rows (as dp_any does), meet at the wave's barrier,
 * and every lane takes the lowest lane whose predicate holds, or 64.  All 64 lanes of the wave call it together.
 */
#ifndef AACG_DEVPORT_CONCEAL_EMU_H
#define AACG_DEVPORT_CONCEAL_EMU_H

DP_DEVICE unsigned dp_wave_first(bool p)
{
    g_emu.w->shfl[g_emu.lane][0] = p ? 1.0f : 0.0f;
    emu_wave_bar();
    unsigned r = 64u;
    for (int i = 63; i >= 0; i--) if (g_emu.w->shfl[i][0] != 0.0f) r = (unsigned)i;
    emu_wave_bar();
    return r;
}

#endif
