/*
 * features_emu.cpp — the feature stage's kernel source (aac.js_amd/csrc/aacg_pcm_features.h: features_body, the body the host's switch
 * would launch) run lane by lane on CPU threads (tests/emu/devport_emu.h, the matrix-core primitive by tests/emu/devport_mfma_emu.h) over
 * one channel of PCM, tables, per-stream records and a history block that the test made, for tests/test_pcm_features_emu.py, which
 * compiles it into a library of its own — and, sharing no code with the body, the rule of include/aacgpu.h as a straight C loop
 * (emu_features_rule), which tests/test_pcm_features_gpu.py applies to the PCM a pipeline delivers without the stage.  With
 * -DFEATURES_EMU_MAIN the same driver is a program: int16 and f32 cases over exactly sized heap blocks, for a build with
 * -fsanitize=address,undefined.  TESTS ONLY.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pcm_features.h"
#include "emu_launch.h"

thread_local emu_lane_ctx g_emu;

extern "C" {

/* what the test lays its launches out by: threads of a workgroup, bytes of a stream's record, feature frames of an item, LDS bytes */
void emu_features_sizes(uint32_t out[4]) { out[0] = AACG_FEATURES_THREADS; out[1] = (uint32_t)sizeof(aacg_features_stream); out[2] = AACG_FEATURES_TILE; out[3] = AACG_FEATURES_LDS_BYTES; }

/* the limits as the host's part checks them: 0, or which one breaks */
int emu_features_check(uint32_t K, uint32_t H, uint32_t P, uint32_t R, uint32_t n_mels) { return aacg_features_check(K, H, P, R, n_mels); }

/* One launch of `blocks` workgroups, run in the order given by `reverse`.  Returns 0 if no body serves the launch. */
int emu_features(const void* src, float* dst, const void* rec, uint32_t n_streams, uint32_t n_items, const float* basis, const float* fb, float* hist,
                 uint32_t K, uint32_t H, uint32_t R, uint32_t n_mels, float floor, uint32_t log, uint32_t row, uint32_t elem, uint32_t blocks, int reverse)
{
    if (aacg_features_check(K, H, 0u, R, n_mels) || !n_items || !n_streams || (elem != 4u && elem != 2u)) return 0;
    aacg_features_args A;
    A.src = src; A.dst = dst; A.rec = (const aacg_features_stream*)rec; A.basis = basis; A.fb = fb; A.hist = hist;
    A.n_streams = n_streams; A.n_items = n_items; A.K = K; A.H = H; A.R = R; A.n_mels = n_mels; A.floor = floor; A.log = log; A.row = row; A.elem = elem;
    const int order = reverse ? EMU_BLOCKS_REVERSE : EMU_BLOCKS_FORWARD;
    if (elem == 4u) emu_launch((int)blocks, AACG_FEATURES_THREADS, AACG_FEATURES_LDS_BYTES, order, [&] { aacg_pipe::features_body<float>(A, blocks); });
    else emu_launch((int)blocks, AACG_FEATURES_THREADS, AACG_FEATURES_LDS_BYTES, order, [&] { aacg_pipe::features_body<int16_t>(A, blocks); });
    return 1;
}

/* THE RULE, as include/aacgpu.h states it, over a whole stream x[0 .. n) since its reset: every frame the n samples complete, frame j at
 * out[j * n_mels].  Returns the count.  (fmaf chains from +0; the power's products and sum each rounded — the volatiles keep a
 * compiler from fusing them, whatever its flags) */
uint64_t emu_features_rule(const float* x, uint64_t n, uint32_t K, uint32_t H, uint32_t P, uint32_t R, uint32_t n_mels, const float* basis, const float* fb,
                           float floor, uint32_t log, float* out)
{
    const uint32_t B = R / 2u;
    const uint64_t count = n + P < K ? 0u : (n + P - K) / H + 1u;
    float* lin = (float*)malloc((size_t)R * sizeof(float));
    float* pw = (float*)malloc((size_t)B * sizeof(float));
    for (uint64_t j = 0; j < count; j++) {
        for (uint32_t r = 0; r < R; r++) {
            float acc = 0.0f;
            for (uint32_t k = 0; k < K; k++) {
                const int64_t at = (int64_t)(j * H) - (int64_t)P + (int64_t)k;
                acc = fmaf(basis[(size_t)r * K + k], at < 0 ? 0.0f : x[at], acc);
            }
            lin[r] = acc;
        }
        for (uint32_t b = 0; b < B; b++) {
            volatile float u = lin[2u * b] * lin[2u * b], v = lin[2u * b + 1u] * lin[2u * b + 1u];
            volatile float sum = u + v;
            pw[b] = sum;
        }
        for (uint32_t m = 0; m < n_mels; m++) {
            float acc = 0.0f;
            for (uint32_t b = 0; b < B; b++) acc = fmaf(fb[(size_t)m * B + b], pw[b], acc);
            out[(size_t)j * n_mels + m] = log ? log10f(acc > floor ? acc : floor) : acc;
        }
    }
    free(lin); free(pw);
    return count;
}

}  // extern "C"

#ifdef FEATURES_EMU_MAIN
/* one case: two streams over heap blocks of exactly the buffers' sizes — a fresh one of n_a samples, and one in mid-stream (it has
 * consumed `before` samples, the last K - 1 of them its history) of n_b — against emu_features_rule over each whole stream */
template <typename T>
static int one_case(uint32_t K, uint32_t H, uint32_t P, uint32_t R, uint32_t NM, uint32_t n_a, uint32_t before, uint32_t n_b, int planar, int log, uint32_t blocks, int reverse)
{
    const uint32_t B = R / 2u, n_in[2] = {n_a, n_b};
    const uint64_t N[2] = {0u, before};
    aacg_features_stream* rec = (aacg_features_stream*)malloc(2 * sizeof(aacg_features_stream));
    if (!rec) return 2;
    uint32_t total = 0, longest = 0, items = 0;
    for (uint32_t s = 0; s < 2; s++) {
        aacg_features_span(K, H, P, N[s], n_in[s], &rec[s]);
        rec[s].in_first = s ? n_a : 0u; rec[s].out_first = total; rec[s].item_first = items; rec[s].slot = s; rec[s].flags = s ? 1u : 2u;
        total += rec[s].n_out; items += aacg_features_items(rec[s].n_out);
        if (rec[s].n_out > longest) longest = rec[s].n_out;
    }
    const uint32_t row = planar ? longest + 3u : 0u;
    const size_t n_src = (size_t)n_a + n_b, n_dst = planar ? (size_t)2 * NM * row : (size_t)total * NM, n_hist = (size_t)2 * 2 * (K - 1);
    T* src = (T*)malloc(n_src * sizeof(T));
    float* dst = (float*)malloc((n_dst ? n_dst : 1) * sizeof(float));
    float* basis = (float*)malloc((size_t)R * K * sizeof(float));
    float* fb = (float*)malloc((size_t)NM * B * sizeof(float));
    float* hist = (float*)malloc(n_hist * sizeof(float));
    float* whole = (float*)malloc(((size_t)before + n_b + n_a) * sizeof(float));
    if (!src || !dst || !basis || !fb || !hist || !whole) return 2;
    const float scale = sizeof(T) == 2 ? 0.000030517578125f : 1.0f;
    for (size_t i = 0; i < n_src; i++) src[i] = (T)(int16_t)(uint16_t)(i * 7u + 1u);
    for (size_t i = 0; i < n_hist; i++) hist[i] = -3.0f;
    for (size_t i = 0; i < (size_t)R * K; i++) basis[i] = (float)((int)((i * 5u) % 7u) - 3) * 0.5f;
    for (size_t i = 0; i < (size_t)NM * B; i++) fb[i] = (float)((int)((i * 3u) % 5u) - 2) * 0.25f;
    for (size_t i = 0; i < n_dst; i++) dst[i] = 12345.0f;
    /* stream 1's earlier samples: made up, the last K - 1 into the history buffer it reads (parity 1) */
    for (uint32_t i = 0; i < before; i++) whole[i] = (float)(int)(i % 13u) - 6.0f;
    for (uint32_t e = 0; e < K - 1u; e++) hist[(size_t)(1 * 2 + 1) * (K - 1) + e] = (int64_t)before - (int64_t)(K - 1u) + e < 0 ? 0.0f : whole[before - (K - 1u) + e];
    for (uint32_t i = 0; i < n_b; i++) whole[before + i] = (float)src[n_a + i] * scale;
    const int ran = emu_features(src, dst, rec, 2, items, basis, fb, hist, K, H, R, NM, 1e-3f, (uint32_t)log, row, (uint32_t)sizeof(T), blocks, reverse);
    size_t wrong = 0;
    for (uint32_t s = 0; s < 2; s++) {
        float* x = whole + (s ? 0 : before + n_b);
        if (!s) for (uint32_t i = 0; i < n_a; i++) x[i] = (float)src[i] * scale;
        const uint64_t n = N[s] + n_in[s], count = n + P < K ? 0u : (n + P - K) / H + 1u;
        float* want = (float*)malloc((size_t)(count ? count : 1) * NM * sizeof(float));
        if (!want) return 2;
        emu_features_rule(x, n, K, H, P, R, NM, basis, fb, 1e-3f, (uint32_t)log, want);
        const uint64_t j0 = count - rec[s].n_out;
        for (uint32_t j = 0; j < (planar ? row : rec[s].n_out); j++)
            for (uint32_t m = 0; m < NM; m++) {
                const float got = planar ? dst[((size_t)s * NM + m) * row + j] : dst[((size_t)rec[s].out_first + j) * NM + m];
                const float w = j < rec[s].n_out ? want[(size_t)(j0 + j) * NM + m] : log ? log10f(1e-3f) : 0.0f;
                wrong += std::memcmp(&got, &w, 4) != 0;
            }
        free(want);
    }
    free(src); free(dst); free(basis); free(fb); free(hist); free(whole); free(rec);
    if (wrong || !ran) std::fprintf(stderr, "features_emu: %zu-byte samples, K %u H %u P %u R %u mels %u, %s, %u workgroups%s: %zu elements differ\n", sizeof(T), K, H, P, R, NM,
                                    planar ? "planar" : "packed", blocks, reverse ? " in reverse" : "", wrong);
    return wrong || !ran ? 1 : 0;
}

int main()
{
    int bad = 0;
    bad |= one_case<int16_t>(32, 7, 31, 6, 1, 300, 45, 200, 0, 0, 1, 0);
    bad |= one_case<float>(32, 7, 31, 6, 1, 300, 45, 200, 1, 1, 3, 1);
    bad |= one_case<float>(64, 64, 0, 34, 5, 50, 100, 700, 0, 1, 2, 1);
    bad |= one_case<int16_t>(400, 160, 200, 10, 3, 1024, 333, 341, 1, 0, 5, 0);
    std::printf(bad ? "features_emu: FAILED\n" : "features_emu: ok\n");
    return bad;
}
#endif
