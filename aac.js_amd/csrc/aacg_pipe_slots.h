/*
 * aacg_pipe_slots.h — what the resident route's host keeps per stream slot for its stateful stages, and what a batch makes of it: the
 * per-stream records that travel up in the lane's staging block.  Host only: no HIP, no devport.h — tests/emu/slots_emu.cpp compiles it
 * with a plain C++ compiler and tests/test_pipe_slots.py pins it against the counting rules restated in Python.
 *
 * A stage's slots hold the settings its records follow from and, per slot, a clock or a position and the two `sides` of its device state.
 * build_* makes a batch's records from the slots AS THEY STAND and changes nothing — a submission refused or failed leaves every slot
 * alone; commit_* advances them, once the batch has been enqueued.  record_block is the records' place in the staging block.  A stage
 * more with state per slot is a slots struct, a build_, a commit_ and a section here, and in aacg_pipeline.hip the calls.
 */
#ifndef AACG_PIPE_SLOTS_H
#define AACG_PIPE_SLOTS_H

#include <cstring>
#include <vector>

#define AACG_RESAMPLE_HOST_ONLY                           /* the limits, the records and the arithmetic: the bodies are the engine's */
#include "aacg_pcm_resample.h"
#define AACG_TRIM_HOST_ONLY
#include "aacg_pcm_trim.h"
#define AACG_FEATURES_HOST_ONLY
#include "aacg_pcm_features.h"
#define AACG_LOUDNESS_HOST_ONLY
#include "aacg_pcm_loudness.h"
#define AACG_LIMIT_HOST_ONLY
#include "aacg_pcm_limit.h"
#include "aacg_pipe_exit.h"

namespace aacg_pipe {

/* A slot's device state is double-buffered.  parity: the buffer its next batch reads (it writes the other); fresh: nothing consumed
 * since its reset — the state counts as zeros and is not read, so a reset clears nothing and either buffer serves */
struct sides {
    std::vector<uint8_t> parity, fresh;
    void make(size_t n_slots) { parity.assign(n_slots, 0); fresh.assign(n_slots, 1); }
    void reset(uint32_t slot) { fresh[slot] = 1; }
    void flip(uint32_t slot) { parity[slot] ^= 1; fresh[slot] = 0; }
    uint32_t flags(uint32_t slot) const { return (uint32_t)parity[slot] | (uint32_t)fresh[slot] << 1; }
};
/* ... and a clock per slot: samples since its reset */
template <typename CLOCK> struct clocked {
    std::vector<CLOCK> N; sides side;
    void make(size_t n_slots) { N.assign(n_slots, 0); side.make(n_slots); }
    void reset(uint32_t slot) { N[slot] = 0; side.reset(slot); }
};
struct resample_slots : clocked<uint32_t> { uint32_t L = 0, M = 0; };            /* L / M (L = 0: no resampler); the clocks are kept modulo M */
struct features_slots : clocked<uint64_t> { uint32_t K = 0, H = 0, P = 0; };     /* frame length, hop, left padding (K = 0: no stage); the clocks count the stage's input */
struct loudness_slots : clocked<uint64_t> { uint32_t hop = 0; };                 /* (0: no meter); the true peak shares clocks, sides and records */
struct limiter_slots {                                                           /* the slots' gains are the caller's: a reset leaves them */
    bool on = false; std::vector<float> gain; sides side;
    void make(size_t n_slots) { gain.assign(n_slots, 1.0f); side.make(n_slots); }
};
struct conceal_slots { bool on = false; sides side; };
/* the slots' windows (skip S, keep K: the caller's, a reset leaves them) and positions Q, in samples of what the stage receives; no device state */
struct trim_slots {
    bool on = false; std::vector<uint64_t> S, K, Q;
    void make(size_t n_slots, uint64_t skip, uint64_t keep) { S.assign(n_slots, skip); K.assign(n_slots, keep); Q.assign(n_slots, 0u); }
    void reset(uint32_t slot) { Q[slot] = 0; }
};

/* the samples a stream of `frames` frames emits at the clock n0 (modulo M): ceil((n0 + 1024 F) L / M) - ceil(n0 L / M), the first
 * through ceil((q M + n) L / M) = q L + ceil(n L / M) so that the one formula (aacg_resample_ceil) sees the arguments it is made for */
inline uint32_t resample_count(uint32_t L, uint32_t M, uint32_t n0, uint32_t frames)
{
    const uint64_t n1 = (uint64_t)n0 + 1024ull * frames;
    return (uint32_t)(n1 / M * L) + aacg_resample_ceil((uint32_t)(n1 % M), L, M) - aacg_resample_ceil(n0, L, M);
}

/* ---- A batch's records: stream s of n_streams is slot slots[s] and brings frames_of[s] frames, packed stream after stream.  The totals
 * the exit plan needs go into b (aacg_pipe_exit.h).  First, what each stream emits ---- */
inline void build_resample(const resample_slots& R, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, std::vector<aacg_resample_stream>& rec, aacg_exit_batch& b)
{
    rec.resize(n_streams);
    for (uint32_t s = 0, first = 0; s < n_streams; first += frames_of[s], s++) {
        const uint32_t slot = slots[s], n_out = resample_count(R.L, R.M, R.N[slot], frames_of[s]);
        rec[s] = {first, frames_of[s], (uint32_t)b.rs_total, n_out, R.N[slot], slot, R.side.parity[slot], R.side.fresh[slot]};
        b.rs_total += n_out;
        if (n_out > b.rs_most) b.rs_most = n_out;
    }
}
/* what each stream keeps of what the stage receives: the resampler's output (rs; empty: none, the transform's frames).  n_in: what each
 * stream brings, by which commit_trim advances its position; items: the launch's */
inline void build_trim(const trim_slots& T, const std::vector<aacg_resample_stream>& rs, int planar, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams,
                       std::vector<aacg_trim_stream>& rec, std::vector<uint32_t>& n_in, uint32_t& items, aacg_exit_batch& b)
{
    rec.resize(n_streams); n_in.resize(n_streams);
    items = 0;
    for (uint32_t s = 0, first = 0; s < n_streams; first += frames_of[s], s++) {
        const uint32_t slot = slots[s], place = rs.empty() ? first * 1024u : rs[s].out_first;
        uint32_t off, n_keep;
        n_in[s] = rs.empty() ? frames_of[s] * 1024u : rs[s].n_out;
        aacg_trim_span(T.Q[slot], T.S[slot], T.K[slot], n_in[s], &off, &n_keep);
        rec[s] = {place + off, n_keep, (uint32_t)b.tr_total, items};
        items += aacg_trim_items(n_keep, planar);
        b.tr_total += n_keep;
        if (n_keep > b.tr_most) b.tr_most = n_keep;
    }
}
/* what each stream's samples complete: one channel, so samples are elements.  The stage takes a trim's kept range where it lies (tr;
 * empty: none), possibly no sample at all, and its clock counts kept samples only; else the resampler's output (rs), else the frames */
inline void build_features(const features_slots& F, const std::vector<aacg_resample_stream>& rs, const std::vector<aacg_trim_stream>& tr, const uint32_t* slots,
                           const uint32_t* frames_of, uint32_t n_streams, std::vector<aacg_features_stream>& rec, uint32_t& items, aacg_exit_batch& b)
{
    rec.resize(n_streams);
    items = 0;
    for (uint32_t s = 0, first = 0; s < n_streams; first += frames_of[s], s++) {
        aacg_features_stream& r = rec[s];
        aacg_features_span(F.K, F.H, F.P, F.N[slots[s]], !tr.empty() ? tr[s].n_keep : !rs.empty() ? rs[s].n_out : frames_of[s] * 1024u, &r);
        r.in_first = !tr.empty() ? tr[s].src_first : !rs.empty() ? rs[s].out_first : first * 1024u;
        r.out_first = (uint32_t)b.ft_total; r.item_first = items; r.slot = slots[s]; r.flags = F.side.flags(slots[s]);
        items += aacg_features_items(r.n_out);
        b.ft_total += r.n_out;
        if (r.n_out > b.ft_most) b.ft_most = r.n_out;
    }
}
/* what each stream's frames complete, C channels.  ld_floats: the floats of the batch's records, two per record and channel; tp_floats:
 * of the true peak's, one (true_peak false: 0) */
inline void build_loudness(const loudness_slots& D, uint32_t C, bool true_peak, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams,
                           std::vector<aacg_loudness_stream>& rec, size_t& ld_floats, size_t& tp_floats)
{
    rec.resize(n_streams);
    uint64_t total = 0;
    for (uint32_t s = 0, first = 0; s < n_streams; first += frames_of[s], s++) {
        const uint32_t slot = slots[s], n_out = (uint32_t)aacg_loudness_emits(D.hop, D.N[slot], 1024ull * frames_of[s]);
        rec[s] = {first, frames_of[s], (uint32_t)total, n_out, (uint32_t)(D.N[slot] % D.hop), slot, D.side.parity[slot], D.side.fresh[slot]};
        total += n_out;
    }
    ld_floats = (size_t)total * C * 2u; tp_floats = true_peak ? (size_t)total * C : 0u;
}
/* the slots' gains as they stand */
inline void build_limiter(const limiter_slots& G, const uint32_t* slots, const uint32_t* frames_of, uint32_t n_streams, std::vector<aacg_limit_stream>& rec)
{
    rec.resize(n_streams);
    for (uint32_t s = 0, first = 0; s < n_streams; first += frames_of[s], s++)
        rec[s] = {first, frames_of[s], slots[s], G.side.parity[slots[s]], G.side.fresh[slots[s]], G.gain[slots[s]], {0u, 0u}};
}
/* the streams' words of the shaped plan's table again, with the side of the slot's state this batch reads */
inline void build_conceal(const conceal_slots& Cn, const aacg_shape_stream* tab, uint32_t n_streams, std::vector<aacg_conceal_stream>& rec)
{
    rec.resize(n_streams);
    for (uint32_t s = 0; s < n_streams; s++) rec[s] = {tab[s].frame_first, tab[s].frames, tab[s].unit_first, tab[s].frame_units, tab[s].slot, tab[s].nch, Cn.side.flags(tab[s].slot), 0u};
}

/* ---- The batch is enqueued: clocks and positions advance, the device state changes sides ---- */
inline void commit_resample(resample_slots& R, const std::vector<aacg_resample_stream>& rec)
{
    for (const auto& r : rec) { R.N[r.slot] = (uint32_t)(((uint64_t)r.n0 + 1024ull * r.frames) % R.M); R.side.flip(r.slot); }
}
inline void commit_features(features_slots& F, const std::vector<aacg_features_stream>& rec) { for (const auto& r : rec) { F.N[r.slot] += r.n_in; F.side.flip(r.slot); } }
inline void commit_loudness(loudness_slots& D, const std::vector<aacg_loudness_stream>& rec) { for (const auto& r : rec) { D.N[r.slot] += 1024ull * r.frames; D.side.flip(r.slot); } }
inline void commit_limiter(limiter_slots& G, const std::vector<aacg_limit_stream>& rec) { for (const auto& r : rec) G.side.flip(r.slot); }
inline void commit_trim(trim_slots& T, const uint32_t* slots, const std::vector<uint32_t>& n_in) { for (size_t s = 0; s < n_in.size(); s++) T.Q[slots[s]] += n_in[s]; }
/* the last good frames: only a batch with a plan was launched, and only a stream with kept units has been through the launch, which
 * wrote the other side of its slot's state */
inline void commit_conceal(conceal_slots& Cn, const std::vector<aacg_conceal_stream>& rec, bool planned)
{
    if (planned) for (const auto& r : rec) if ((r.frame_units >> 8) & 0xffu) Cn.side.flip(r.slot);
}

/* A batch's records in the staging block, behind the per-stream table: sections back to back from a 16-byte aligned base, every record
 * a multiple of 16 bytes.  With a feature stage the trim's stay down here: the stage has them in its own records */
struct record_block {
    enum { RS, FT, LD, LIM, CN, TR, SECTIONS };
    struct section { const void* data; size_t bytes, at; } sec[SECTIONS] = {};
    template <typename T> void set(int i, const std::vector<T>& v) { sec[i].data = v.data(); sec[i].bytes = v.size() * sizeof(T); }
    record_block() {}
    record_block(const std::vector<aacg_resample_stream>& rs, const std::vector<aacg_features_stream>& ft, const std::vector<aacg_loudness_stream>& ld,
                 const std::vector<aacg_limit_stream>& lim, const std::vector<aacg_conceal_stream>& cn, const std::vector<aacg_trim_stream>& tr)
    {
        set(RS, rs); set(FT, ft); set(LD, ld); set(LIM, lim); set(CN, cn);
        if (ft.empty()) set(TR, tr);
    }
    size_t lay(size_t base) { for (auto& s : sec) { s.at = base; base += s.bytes; } return base; }      /* the sections' places from `base`; returns the end of the last */
    size_t at(int i) const { return sec[i].at; }
    void copy(void* block, int i) const { if (sec[i].bytes) std::memcpy((char*)block + sec[i].at, sec[i].data, sec[i].bytes); }      /* section i into the block ... */
    void copy(void* block) const { for (int i = 0; i < SECTIONS; i++) copy(block, i); }                                                  /* ... or all of them */
};

}  // namespace aacg_pipe

#endif
