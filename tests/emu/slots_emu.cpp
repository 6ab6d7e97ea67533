/*
 * slots_emu.cpp — the resident route's slot state, record builders, commits and record block (aac.js_amd/csrc/aacg_pipe_slots.h) behind a
 * flat C interface, for tests/test_pipe_slots.py, which compiles it into a library of its own together with the host sources whose
 * aacg_*_counts the test cross-checks its oracle with.  One `emu_slots` is what aacg_pipeline.hip keeps: the stages' slots, and a batch's
 * records as check_batch, stage_batch and choose_plan make them, in their order.  Host code only: nothing is emulated.  TESTS ONLY.
 */
#include <cstring>

#include "../../aac.js_amd/csrc/aacg_pipe_slots.h"

using namespace aacg_pipe;

struct emu_slots {
    resample_slots rs; features_slots ft; loudness_slots ld; limiter_slots lim; conceal_slots cn; trim_slots tr;
    uint32_t C = 0; bool true_peak = false;
    /* the batch built last */
    std::vector<aacg_resample_stream> rs_rec; std::vector<aacg_features_stream> ft_rec; std::vector<aacg_loudness_stream> ld_rec;
    std::vector<aacg_limit_stream> lim_rec; std::vector<aacg_conceal_stream> cn_rec; std::vector<aacg_trim_stream> tr_rec;
    std::vector<uint32_t> tr_in, slots;
    uint32_t tr_items = 0, ft_items = 0; size_t ld_floats = 0, tp_floats = 0;
    aacg_exit_batch b = {};
    record_block R;
};

extern "C" {

/* cfg: n_slots, L, M, K, H, P, hop, true_peak, C, limiter, concealment, trim, skip, keep (a stage whose first word is 0 is not set) */
emu_slots* emu_slots_make(const uint64_t* cfg)
{
    emu_slots* e = new emu_slots();
    const size_t n = (size_t)cfg[0];
    if (cfg[1]) { e->rs.make(n); e->rs.L = (uint32_t)cfg[1]; e->rs.M = (uint32_t)cfg[2]; }
    if (cfg[3]) { e->ft.make(n); e->ft.K = (uint32_t)cfg[3]; e->ft.H = (uint32_t)cfg[4]; e->ft.P = (uint32_t)cfg[5]; }
    if (cfg[6]) { e->ld.make(n); e->ld.hop = (uint32_t)cfg[6]; }
    e->true_peak = cfg[7] != 0; e->C = (uint32_t)cfg[8];
    if (cfg[9]) { e->lim.make(n); e->lim.on = true; }
    if (cfg[10]) { e->cn.side.make(n); e->cn.on = true; }
    if (cfg[11]) { e->tr.make(n, cfg[12], cfg[13]); e->tr.on = true; }
    return e;
}
void emu_slots_free(emu_slots* e) { delete e; }

/* A batch's records from the slots as they stand, in the pipeline's order: resampler, trim, features, meter, limiter (check_batch), the
 * sections laid out from `base` (stage_batch), the concealment's from the table (choose_plan; tab: n_streams x {frame_first, frames,
 * unit_first, frame_units, slot, nch}, null without the stage).  Changes no slot */
void emu_slots_build(emu_slots* e, const uint32_t* slots, const uint32_t* frames_of, uint32_t n, int planar, const uint32_t* tab, uint64_t base)
{
    e->rs_rec.clear(); e->ft_rec.clear(); e->ld_rec.clear(); e->lim_rec.clear(); e->cn_rec.clear(); e->tr_rec.clear(); e->tr_in.clear();
    e->tr_items = e->ft_items = 0; e->ld_floats = e->tp_floats = 0;
    e->b = aacg_exit_batch();
    e->slots.assign(slots, slots + n);
    if (e->rs.L) build_resample(e->rs, slots, frames_of, n, e->rs_rec, e->b);
    if (e->tr.on) build_trim(e->tr, e->rs_rec, planar && !e->ft.K, slots, frames_of, n, e->tr_rec, e->tr_in, e->tr_items, e->b);
    if (e->ft.K) build_features(e->ft, e->rs_rec, e->tr_rec, slots, frames_of, n, e->ft_rec, e->ft_items, e->b);
    if (e->ld.hop) build_loudness(e->ld, e->C, e->true_peak, slots, frames_of, n, e->ld_rec, e->ld_floats, e->tp_floats);
    if (e->lim.on) build_limiter(e->lim, slots, frames_of, n, e->lim_rec);
    if (e->cn.on) e->cn_rec.assign(n, aacg_conceal_stream());
    e->R = record_block(e->rs_rec, e->ft_rec, e->ld_rec, e->lim_rec, e->cn_rec, e->tr_rec);
    e->R.lay((size_t)base);
    if (e->cn.on) {
        std::vector<aacg_shape_stream> t(n);
        for (uint32_t s = 0; s < n; s++) { t[s] = aacg_shape_stream(); t[s].frame_first = tab[6 * s]; t[s].frames = tab[6 * s + 1]; t[s].unit_first = tab[6 * s + 2];
                                           t[s].frame_units = tab[6 * s + 3]; t[s].slot = tab[6 * s + 4]; t[s].nch = tab[6 * s + 5]; }
        build_conceal(e->cn, t.data(), n, e->cn_rec);
    }
}

/* the batch is enqueued: every stage's commit, as enqueue_out calls them */
void emu_slots_commit(emu_slots* e, int planned)
{
    commit_resample(e->rs, e->rs_rec); commit_features(e->ft, e->ft_rec); commit_loudness(e->ld, e->ld_rec);
    commit_limiter(e->lim, e->lim_rec); commit_trim(e->tr, e->slots.data(), e->tr_in); commit_conceal(e->cn, e->cn_rec, planned != 0);
}

/* aacg_pipeline_reset_stream, aacg_pipeline_set_gain and aacg_pipeline_set_stream_trim, as far as the slots go */
void emu_slots_reset(emu_slots* e, uint32_t slot)
{
    if (e->rs.L) e->rs.reset(slot);
    if (e->ft.K) e->ft.reset(slot);
    if (e->ld.hop) e->ld.reset(slot);
    if (e->tr.on) e->tr.reset(slot);
    if (e->cn.on) e->cn.side.reset(slot);
    if (e->lim.on) e->lim.side.reset(slot);
}
void emu_slots_set_gain(emu_slots* e, uint32_t slot, float gain) { e->lim.gain[slot] = gain; }
void emu_slots_set_window(emu_slots* e, uint32_t slot, uint64_t skip, uint64_t keep) { e->tr.S[slot] = skip; e->tr.K[slot] = keep; e->tr.Q[slot] = 0; }

/* a slot's state: per stage (rs, ft, ld, lim, cn) clock, parity, fresh, flags — 0 for a stage that is not set or has no clock —, then
 * the trim's S, K, Q: 23 words; the limiter's gain beside them */
void emu_slots_state(const emu_slots* e, uint32_t slot, uint64_t* out, float* gain)
{
    std::memset(out, 0, 23 * sizeof(uint64_t));
    auto put = [&](int i, uint64_t clock, const sides& s) { out[4 * i] = clock; out[4 * i + 1] = s.parity[slot]; out[4 * i + 2] = s.fresh[slot]; out[4 * i + 3] = s.flags(slot); };
    if (e->rs.L) put(0, e->rs.N[slot], e->rs.side);
    if (e->ft.K) put(1, e->ft.N[slot], e->ft.side);
    if (e->ld.hop) put(2, e->ld.N[slot], e->ld.side);
    if (e->lim.on) put(3, 0, e->lim.side);
    if (e->cn.on) put(4, 0, e->cn.side);
    if (e->tr.on) { out[20] = e->tr.S[slot]; out[21] = e->tr.K[slot]; out[22] = e->tr.Q[slot]; }
    *gain = e->lim.on ? e->lim.gain[slot] : 0.0f;
}

/* the built batch's totals: rs_total, rs_most, tr_total, tr_most, tr_items, ft_total, ft_most, ft_items, ld_floats, tp_floats */
void emu_slots_totals(const emu_slots* e, uint64_t* out)
{
    const uint64_t v[10] = {e->b.rs_total, e->b.rs_most, e->b.tr_total, e->b.tr_most, e->tr_items, e->b.ft_total, e->b.ft_most, e->ft_items, e->ld_floats, e->tp_floats};
    std::memcpy(out, v, sizeof v);
}
/* ... what each stream brings the trim (n words; returns how many there are) */
uint32_t emu_slots_trim_in(const emu_slots* e, uint32_t* out) { std::memcpy(out, e->tr_in.data(), e->tr_in.size() * 4); return (uint32_t)e->tr_in.size(); }

/* the record block's sections (RS, FT, LD, LIM, CN, TR): out[2 i] = at, out[2 i + 1] = bytes; returns the end of the last */
uint64_t emu_slots_sections(const emu_slots* e, uint64_t* out)
{
    uint64_t end = 0;
    for (int i = 0; i < record_block::SECTIONS; i++) { out[2 * i] = e->R.at(i); out[2 * i + 1] = e->R.sec[i].bytes; end = e->R.at(i) + e->R.sec[i].bytes; }
    return end;
}
/* the sections (i < 0: all of them, else section i alone) into a block laid out as emu_slots_build's base says */
void emu_slots_copy(const emu_slots* e, void* block, int i) { if (i < 0) e->R.copy(block); else e->R.copy(block, i); }
/* a stage's records by themselves, as the builder left them (section as above; TR also with a feature stage): returns the bytes */
uint64_t emu_slots_records(const emu_slots* e, int section, void* out)
{
    const void* const data[] = {e->rs_rec.data(), e->ft_rec.data(), e->ld_rec.data(), e->lim_rec.data(), e->cn_rec.data(), e->tr_rec.data()};
    const size_t bytes[] = {e->rs_rec.size() * sizeof(aacg_resample_stream), e->ft_rec.size() * sizeof(aacg_features_stream), e->ld_rec.size() * sizeof(aacg_loudness_stream),
                            e->lim_rec.size() * sizeof(aacg_limit_stream), e->cn_rec.size() * sizeof(aacg_conceal_stream), e->tr_rec.size() * sizeof(aacg_trim_stream)};
    if (bytes[section]) std::memcpy(out, data[section], bytes[section]);
    return bytes[section];
}

}  // extern "C"
