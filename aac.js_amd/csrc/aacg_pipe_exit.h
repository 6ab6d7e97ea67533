/*
 * aacg_pipe_exit.h — where a resident batch's PCM goes on its way out of aacg_pipeline.hip, as data: ONE pure function turns what the
 * pipeline is and what the batch is into a short list of stages, and the pipeline walks that list (enqueue_out) and decides nothing
 * about buffers anywhere else.  Host only: no HIP, no devport.h — tests/emu/exit_emu.cpp compiles it with a plain C++ compiler and
 * tests/test_pipe_exit_plan.py pins every row of the table below, like tests/test_pipe_map_emu.py pins the host planner of aacg_pipe_map.h.
 *
 * The way out.  n frames in n_streams streams, C channels from the transform, O from the mix (0: none), Oc = O ? O : C, E bytes an
 * element, sum n_out the samples a resampler emits for the batch's streams together:
 *
 *   stage      present        reads                       writes                                                     bytes
 *   transform  always         —                           CALLER if DEV_PACKED and neither mix nor resampler,        n C 1024 E
 *                                                         else LANE_PCM
 *   mix        O != 0         LANE_PCM                    CALLER if DEV_PACKED and no resampler, else LANE_MIX       n O 1024 E
 *   limit      a limiter      LANE_MIX if O, else         CALLER if DEV_PACKED and neither resampler nor feature     n Oc 1024 E
 *                             LANE_PCM                    stage, else LANE_LIM
 *   resample   a resampler    LANE_LIM, LANE_MIX or       CALLER for either device layout (row = stride_frames x     sum n_out Oc E
 *                             LANE_PCM: the last written  1024 if planar, else 0), else LANE_RS
 *   features   a feature      LANE_RS, LANE_LIM, LANE_MIX CALLER for either device layout (ft_row = stride_frames,    sum ft_out n_mels 4
 *              stage          or LANE_PCM: the last       FEATURE frames, if planar, else 0), else LANE_FT
 *                             written
 *   trim       a trim and no  LANE_RS, LANE_LIM, LANE_MIX CALLER for either device layout (row = stride_frames x     sum n_keep Oc E
 *              feature stage  or LANE_PCM: the last       1024 if planar, else 0), else LANE_TRIM
 *                             written
 *   tail       see `writes`   the last lane buffer        PLANAR_LAUNCH -> CALLER if DEV_PLANAR and neither resampler out_bytes
 *                             written                     nor trim nor feature stage; COPY_DOWN -> CALLER (page-locked) or
 *                                                         LANE_HOST (pageable, and collect copies it to the caller)
 *                                                         for a host batch; else there is no tail
 *
 * With a feature stage (aacg_pipeline_set_features: n_mels float32 per feature frame leave in the place of Oc = 1 channel of PCM) the
 * stages in front of it write lane buffers whatever the destination — the transform LANE_PCM, the mix LANE_MIX, the resampler LANE_RS
 * with row 0 — and the feature stage is the one that writes the caller's device memory.
 *
 * With a limiter (aacg_pipeline_set_limiter: a gain per stream and a look-ahead limiter, sample for sample) the stages in front of it
 * write lane buffers whatever the destination too — the transform LANE_PCM, the mix LANE_MIX — and the stages behind it read LANE_LIM
 * as the last written.  It emits what it receives: out_bytes, device_need and exit_host_capacity do not know it.
 *
 * With a trim (aacg_pipeline_set_trim: each stream's samples cut to its slot's window, sum n_keep of them kept) and no feature stage
 * the stages in front of it write lane buffers whatever the destination too — the resampler LANE_RS with row 0 — and the trim is the one
 * that writes the caller's device memory, in either layout: there is no PLANAR_LAUNCH tail.  With a feature stage there is NO trim row:
 * the feature stage reads each stream's kept range where it lies (its records' in_first and n_in), and ft_most / ft_total follow from
 * the trimmed counts.  A batch may keep nothing: out_bytes 0, and the walk enqueues neither a launch for a packed destination nor a copy.
 *
 * out_bytes, what leaves: sum ft_out n_mels 4 with a feature stage, else sum n_keep Oc E with a trim, else sum n_out Oc E with a
 * resampler, else n Oc 1024 E.
 * device_need, what a caller's device buffer must hold: n_streams n_mels stride_frames 4 (features) or n_streams Oc stride_frames 1024
 * E planar, out_bytes packed.  The caller's memory is written by exactly one stage, the last.
 *
 * A stage more on the way out (another layout, a filter) is a row more here and a block more in enqueue_out's walk.
 */
#ifndef AACG_PIPE_EXIT_H
#define AACG_PIPE_EXIT_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/aacgpu.h"

/* a buffer a stage reads or writes: the lane's d_pcm, d_mix, d_rs, its page-locked h_pcm, or the caller's memory (host or device) */
enum { AACG_EXIT_BUF_NONE = 0, AACG_EXIT_LANE_PCM, AACG_EXIT_LANE_MIX, AACG_EXIT_LANE_RS, AACG_EXIT_LANE_HOST, AACG_EXIT_CALLER,
       AACG_EXIT_LANE_FT,      /* (the lane's d_ft: a host batch's feature frames) */
       AACG_EXIT_LANE_LIM,     /* (the lane's d_lim: the limiter's PCM wherever it is not the last stage of a packed device batch) */
       AACG_EXIT_LANE_TRIM };  /* (the lane's d_trim: a host batch's trimmed PCM) */
/* where the caller wants the batch's PCM */
enum { AACG_EXIT_HOST_PINNED = 0, AACG_EXIT_HOST_PAGEABLE, AACG_EXIT_DEV_PACKED, AACG_EXIT_DEV_PLANAR };
enum { AACG_EXIT_XFORM = 0, AACG_EXIT_MIX, AACG_EXIT_RESAMPLE, AACG_EXIT_TAIL, AACG_EXIT_FEATURES, AACG_EXIT_LIMIT, AACG_EXIT_TRIM };
enum { AACG_EXIT_TAIL_NONE = 0, AACG_EXIT_TAIL_PLANAR_LAUNCH, AACG_EXIT_TAIL_COPY_DOWN };

/* what the pipeline is */
typedef struct aacg_exit_pipe {
    uint32_t C, O;             /* channels of the transform's PCM; of the mix's (0: no mix)                                     */
    uint32_t resampled;        /* a resampler is set                                                                            */
    uint32_t elem;             /* 4 or 2                                                                                        */
    uint32_t max_streams, max_frames;
    uint64_t lane_elems;       /* a resampler: elements of the largest batch's output (aacg_pipe::exit_resample_most x Oc)      */
    uint32_t n_mels;           /* a feature stage: floats per feature frame (0: none)                                           */
    uint64_t ft_lane_elems;    /* ... and the floats of the largest batch's output (aacg_pipe::exit_features_most x n_mels)     */
    uint32_t limited;          /* a limiter is set (the drivers that build this positionally leave it and what follows 0)       */
    uint32_t trimmed;          /* a trim is set                                                                                 */
} aacg_exit_pipe;

/* what the batch is */
typedef struct aacg_exit_batch {
    uint32_t n, n_streams, longest;       /* frames, streams, the largest frame count of a stream                               */
    uint32_t dest;                        /* AACG_EXIT_HOST_PINNED .. AACG_EXIT_DEV_PLANAR                                      */
    uint32_t stride_frames;               /* a device batch's (aacg_pcm_device_out)                                             */
    uint32_t rs_most;                     /* a resampler: the largest n_out of a stream ...                                     */
    uint64_t rs_total;                    /* ... and the sum of them                                                            */
    uint32_t ft_most;                     /* a feature stage: the largest count of feature frames of a stream ...               */
    uint64_t ft_total;                    /* ... and the sum of them                                                            */
    uint32_t tr_most;                     /* a trim: the largest n_keep of a stream ...                                         */
    uint64_t tr_total;                    /* ... and the sum of them                                                            */
} aacg_exit_batch;

typedef struct aacg_exit_stage {
    uint8_t what, src, dst, tail;         /* AACG_EXIT_XFORM .., two buffers, and for the tail AACG_EXIT_TAIL_*                  */
    uint64_t bytes;                       /* what it writes                                                                     */
} aacg_exit_stage;

typedef struct aacg_exit_plan {
    aacg_exit_stage stage[7];             /* in the order they are enqueued; the first is the transform                         */
    uint32_t n_stages;
    uint32_t row;                         /* a planar resample or trim, whichever writes the caller's tensor: elements per row; else 0 */
    uint64_t xform_bytes;                 /* what the transform writes: the clear for unlearnt streams acts on it               */
    uint64_t out_bytes;                   /* what leaves                                                                        */
    uint64_t device_need;                 /* a device batch: the bytes the caller's buffer must hold                            */
    uint32_t collect_copy;                /* collect copies out_bytes from LANE_HOST to the caller                              */
    uint32_t ft_row;                      /* planar features: feature frames per row; else 0                                    */
} aacg_exit_plan;

/* a refusal of aacg_pipeline_submit_device: AACG_OK, or the code and the text.  late: the rule comes BEHIND the runtime's answer
 * about the pointer in the order of refusals (check_device_out asks the runtime in between) */
struct aacg_exit_refusal { int code; bool late; std::string text; };

namespace aacg_pipe {

inline uint32_t exit_out_channels(const aacg_exit_pipe& P) { return P.O ? P.O : P.C; }

/* the most samples per channel a batch can emit: a stream of F frames emits at most ceil(1024 F L / M) samples, so a batch at most its
 * frames' share and one more per stream */
inline uint64_t exit_resample_most(uint32_t max_streams, uint32_t max_frames, uint32_t L, uint32_t M)
{
    return ((uint64_t)max_streams * max_frames * 1024u * L + M - 1u) / M + max_streams;
}

/* the most feature frames a batch can emit: a stream that brings n samples completes at most n / H + 1 frames.  most_samples: the
 * batch's most samples, exit_resample_most with a resampler, else max_streams x max_frames x 1024 */
inline uint64_t exit_features_most(uint32_t max_streams, uint64_t most_samples, uint32_t H)
{
    return most_samples / H + max_streams;
}

/* bytes of a lane's page-locked staging (h_pcm): the largest batch's out_bytes */
inline size_t exit_host_capacity(const aacg_exit_pipe& P)
{
    if (P.n_mels) return (size_t)P.ft_lane_elems * 4u;
    return (size_t)(P.resampled ? P.lane_elems : (uint64_t)P.max_streams * P.max_frames * exit_out_channels(P) * 1024u) * P.elem;
}

inline uint32_t exit_dest_device(int32_t layout) { return layout == AACG_PCM_PLANAR ? AACG_EXIT_DEV_PLANAR : AACG_EXIT_DEV_PACKED; }

inline aacg_exit_plan exit_plan(const aacg_exit_pipe& P, const aacg_exit_batch& B)
{
    const uint64_t E = P.elem, Oc = exit_out_channels(P);
    const bool ft = P.n_mels != 0, to_dev = B.dest == AACG_EXIT_DEV_PACKED || B.dest == AACG_EXIT_DEV_PLANAR;
    /* (the stages in front of a feature stage see neither device destination: they write lane buffers) */
    const bool packed = B.dest == AACG_EXIT_DEV_PACKED && !ft, planar = B.dest == AACG_EXIT_DEV_PLANAR && !ft, rs = P.resampled != 0;
    const bool lim = P.limited != 0;                     /* (... and so do the stages in front of a limiter) */
    const bool tr = P.trimmed != 0 && !ft;               /* (... and of a trim; with a feature stage the trim is no stage: it is in that stage's records) */
    aacg_exit_plan X = {};
    uint8_t last = AACG_EXIT_BUF_NONE;                   /* the buffer the stage before wrote */
    auto push = [&](uint8_t what, uint8_t dst, uint64_t bytes, uint8_t tail) { X.stage[X.n_stages++] = {what, last, dst, tail, bytes}; last = dst; };
    X.xform_bytes = (uint64_t)B.n * P.C * 1024u * E;
    const uint64_t mix_bytes = (uint64_t)B.n * Oc * 1024u * E;
    const uint64_t rs_bytes = rs ? B.rs_total * Oc * E : mix_bytes;
    X.out_bytes = tr ? B.tr_total * Oc * E : rs_bytes;
    X.device_need = planar ? (uint64_t)B.n_streams * Oc * B.stride_frames * 1024u * E : packed ? X.out_bytes : 0u;
    X.row = (rs || tr) && planar ? B.stride_frames * 1024u : 0u;
    push(AACG_EXIT_XFORM, packed && !P.O && !rs && !lim && !tr ? AACG_EXIT_CALLER : AACG_EXIT_LANE_PCM, X.xform_bytes, AACG_EXIT_TAIL_NONE);
    if (P.O) push(AACG_EXIT_MIX, packed && !rs && !lim && !tr ? AACG_EXIT_CALLER : AACG_EXIT_LANE_MIX, mix_bytes, AACG_EXIT_TAIL_NONE);
    if (lim) push(AACG_EXIT_LIMIT, packed && !rs && !tr ? AACG_EXIT_CALLER : AACG_EXIT_LANE_LIM, mix_bytes, AACG_EXIT_TAIL_NONE);
    if (rs) push(AACG_EXIT_RESAMPLE, (packed || planar) && !tr ? AACG_EXIT_CALLER : AACG_EXIT_LANE_RS, rs_bytes, AACG_EXIT_TAIL_NONE);
    if (tr) push(AACG_EXIT_TRIM, packed || planar ? AACG_EXIT_CALLER : AACG_EXIT_LANE_TRIM, X.out_bytes, AACG_EXIT_TAIL_NONE);
    if (ft) {
        X.out_bytes = B.ft_total * P.n_mels * 4u;        /* (the stage in front has its own bytes in its row) */
        X.ft_row = B.dest == AACG_EXIT_DEV_PLANAR ? B.stride_frames : 0u;
        X.device_need = B.dest == AACG_EXIT_DEV_PLANAR ? (uint64_t)B.n_streams * P.n_mels * B.stride_frames * 4u : to_dev ? X.out_bytes : 0u;
        push(AACG_EXIT_FEATURES, to_dev ? AACG_EXIT_CALLER : AACG_EXIT_LANE_FT, X.out_bytes, AACG_EXIT_TAIL_NONE);
    }
    if (planar && !rs && !tr) push(AACG_EXIT_TAIL, AACG_EXIT_CALLER, X.out_bytes, AACG_EXIT_TAIL_PLANAR_LAUNCH);
    else if (!to_dev) {
        X.collect_copy = B.dest == AACG_EXIT_HOST_PAGEABLE;
        push(AACG_EXIT_TAIL, X.collect_copy ? AACG_EXIT_LANE_HOST : AACG_EXIT_CALLER, X.out_bytes, AACG_EXIT_TAIL_COPY_DOWN);
    }
    return X;
}

/* aacg_pipeline_submit_device's refusals that need no runtime, in their order; X = exit_plan(P, B) with B.dest = exit_dest_device(out.layout).
 * planar_items: aacg_planar_items(B.n_streams, out.stride_frames, P.elem) — 0: more than one aacg_pcm_planar launch addresses */
inline aacg_exit_refusal exit_check(const aacg_exit_pipe& P, const aacg_exit_batch& B, const aacg_exit_plan& X, const aacg_pcm_device_out& out, uint32_t planar_items)
{
    const bool rs = P.resampled != 0;                    /* the rows hold samples at the new rate */
    const bool tr = P.trimmed != 0;                      /* the rows hold the kept samples, written by the trim */
    auto no = [](int code, bool late, std::string text) { return aacg_exit_refusal{code, late, "aacg_pipeline_submit_device: " + text}; };
    if ((uintptr_t)out.d_pcm & 15u) return no(AACG_ERR_INVALID_ARG, false, "d_pcm is not 16-byte aligned");
    if (out.layout != AACG_PCM_PACKED && out.layout != AACG_PCM_PLANAR) return no(AACG_ERR_INVALID_ARG, false, "unknown layout (AACG_PCM_PACKED or AACG_PCM_PLANAR)");
    if (out.layout == AACG_PCM_PACKED && out.stride_frames) return no(AACG_ERR_INVALID_ARG, false, "AACG_PCM_PACKED takes stride_frames 0");
    if (P.n_mels) {                                      /* a feature stage: stride_frames counts FEATURE frames per row, and no aacg_pcm_planar launch is involved */
        if (out.layout == AACG_PCM_PLANAR) {
            if (!out.stride_frames || out.stride_frames > (1u << 21)) return no(AACG_ERR_INVALID_ARG, false, "stride_frames is not in 1..2^21");
            if (out.stride_frames < B.ft_most) return no(AACG_ERR_INVALID_ARG, false, "stride_frames is below a stream's count of feature frames (aacg_pipeline_out_samples)");
        }
        if ((uint64_t)out.d_pcm_bytes < X.device_need) return no(AACG_ERR_CAPACITY, true, "d_pcm_bytes is smaller than the batch needs (" + std::to_string(X.device_need) + " bytes)");
        return {AACG_OK, false, std::string()};
    }
    if (out.layout == AACG_PCM_PLANAR && !rs && !tr && out.stride_frames < B.longest) return no(AACG_ERR_INVALID_ARG, false, "stride_frames is below the batch's largest frame count");
    if (out.layout == AACG_PCM_PLANAR && rs && !tr) {
        if (!out.stride_frames || out.stride_frames > (1u << 21)) return no(AACG_ERR_INVALID_ARG, false, "stride_frames is not in 1..2^21");
        if ((uint64_t)out.stride_frames * 1024u < B.rs_most) return no(AACG_ERR_INVALID_ARG, false, "stride_frames x 1024 is below a stream's resampled count (aacg_pipeline_out_samples)");
    }
    if (out.layout == AACG_PCM_PLANAR && tr) {
        if (!out.stride_frames || out.stride_frames > (1u << 21)) return no(AACG_ERR_INVALID_ARG, false, "stride_frames is not in 1..2^21");
        if ((uint64_t)out.stride_frames * 1024u < B.tr_most) return no(AACG_ERR_INVALID_ARG, false, "stride_frames x 1024 is below a stream's trimmed count (aacg_pipeline_out_samples)");
    }
    if ((uint64_t)out.d_pcm_bytes < X.device_need) return no(AACG_ERR_CAPACITY, true, "d_pcm_bytes is smaller than the batch needs (" + std::to_string(X.device_need) + " bytes)");
    if (out.layout == AACG_PCM_PLANAR && !rs && !tr && !planar_items) return no(AACG_ERR_CAPACITY, true, "n_streams x stride_frames is more than one aacg_pcm_planar launch addresses");
    return {AACG_OK, false, std::string()};
}

}  // namespace aacg_pipe

#endif
