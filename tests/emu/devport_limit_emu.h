/*
 * devport_limit_emu.h — the CPU twin of devport.h's wave-wide maximum, included behind devport_emu.h.  TEST INFRASTRUCTURE ONLY.
 *
 * dp_wave_max: the wave's 64 lanes put their N values into the emulator's shuffle rows (as dp_shfl and dp_any do), meet at the wave's
 * barrier, and every lane takes the largest of each column, the lanes in turn from lane 0 — the device's butterfly takes them in
 * another order, and the maximum of floats that are no NaN is the same in any.  All 64 lanes of the wave call it together.
 */
#ifndef AACG_DEVPORT_LIMIT_EMU_H
#define AACG_DEVPORT_LIMIT_EMU_H

template <int N>
DP_DEVICE void dp_wave_max(float (&v)[N])
{
    static_assert(N <= 16, "shuffle payload");
    for (int i = 0; i < N; i++) g_emu.w->shfl[g_emu.lane][i] = v[i];
    emu_wave_bar();
    for (int i = 0; i < N; i++) {
        float m = g_emu.w->shfl[0][i];
        for (int l = 1; l < 64; l++) m = fmaxf(m, g_emu.w->shfl[l][i]);
        v[i] = m;
    }
    emu_wave_bar();
}

#endif
