/*
 * devport_mfma_emu.h — the CPU twin of devport.h's matrix-core primitive, included behind devport_emu.h.  TEST INFRASTRUCTURE ONLY.
 *
 * dp_mfma_16x16x4: the wave's 64 lanes exchange their operands through the emulator's shuffle (the wave's shfl rows and its barrier,
 * exactly as dp_shfl and dp_row_gather12 move values — one exchange in the place of the twenty single-source dp_shfl calls the
 * sixteen A and four B values of a lane would take), and each lane then computes its own four outputs as the hardware layout
 * assigns them: lane l holds D[4 (l >> 4) + i][l & 15], A[r][k] was given by lane 16 k + r, B[k][c] by lane 16 k + c, and every
 * output is the k-ordered fmaf chain on its accumulator.  All 64 lanes of the wave call it together, as they issue the instruction.
 */
#ifndef AACG_DEVPORT_MFMA_EMU_H
#define AACG_DEVPORT_MFMA_EMU_H

DP_DEVICE void dp_mfma_16x16x4(float a, float b, float (&acc)[4])
{
    const int l = g_emu.lane, g = l >> 4, c = l & 15;
    g_emu.w->shfl[l][0] = a;
    g_emu.w->shfl[l][1] = b;
    emu_wave_bar();
    for (int i = 0; i < 4; i++) {
        const int r = 4 * g + i;
        float d = acc[i];
        for (int k = 0; k < 4; k++) d = fmaf(g_emu.w->shfl[16 * k + r][0], g_emu.w->shfl[16 * k + c][1], d);
        acc[i] = d;
    }
    emu_wave_bar();
}

#endif
