/*
 * aacg_shape.cpp — the host's part of a plan shaped on the device (aacg_plan_shape.h): what the engine computes itself per batch
 * shape, in O(streams) — the counts of units, runs and links, the flags launch_run takes from aacg_plan_host for a kept plan
 * (zero_fill, pcm_floats, wide_frames, long_chains), the chains a launch advances, each stream's first run and first link in the
 * host planner's order, the capacity check — and the rule which consecutive launches of such a plan may meet in the cross-launch
 * cells.  Plain C++, as aacg_pipeline_order is in aacg_routes.cpp: the engine calls it, tests/emu_shape links it next to
 * aacg_plan_build, which is the reference for every figure here.
 */
#include "aacg_plan_shape.h"
#include "aacg_shape_carry.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace {

int fail(std::string* err, int code, const char* fmt, long a = 0, long b = 0, long c = 0)
{
    if (err) {
        char buf[256];
        std::snprintf(buf, sizeof buf, fmt, a, b, c);
        *err = buf;
    }
    return code;
}

}  // namespace

aacg_shape_limits aacg_shape_capacity(uint32_t max_streams, uint32_t max_frames, uint32_t max_elems, uint32_t channels)
{
    aacg_shape_limits lim;
    lim.max_streams = max_streams; lim.max_frames = max_frames;
    lim.max_elems = std::min(std::min(max_elems, channels), 8u);              /* every element has a channel of its own at least */
    const size_t chains = (size_t)max_streams * lim.max_elems, runs = (max_frames + AACG_RUN_W - 1u) / AACG_RUN_W;
    lim.max_units = chains * max_frames;
    lim.max_runs = chains * runs;
    lim.max_links = chains * (runs - 1u);
    return lim;
}

int aacg_shape_plan(aacg_shape_stream* table, uint32_t n_streams, uint32_t n_slots, uint32_t channels, uint32_t Cp, const uint8_t* parity,
                    const aacg_shape_limits& lim, aacg_shape_info* out, std::string* err)
{
    if (!table || !n_streams || !out || channels < 1 || channels > AACG_MAX_CHANNELS || Cp < channels) return fail(err, AACG_ERR_INVALID_ARG, "aacg_shape_plan: bad arguments");
    if (n_streams > lim.max_streams) return fail(err, AACG_ERR_CAPACITY, "the batch has %ld streams, the shaped plan was made for %ld", n_streams, lim.max_streams);
    /* the caller's part: the kernel writes where these words say */
    uint64_t frames = 0, units = 0, runs = 0, links = 0;
    bool zero_fill = false, long_chains = false;
    uint32_t pcm_frames = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        const aacg_shape_stream& t = table[s];
        const uint32_t n = t.frame_units & 0xffu, kept = (t.frame_units >> 8) & 0xffu, F = t.frames;
        if (t.slot >= n_slots) return fail(err, AACG_ERR_CAPACITY, "stream %ld of the batch: slot %ld >= max_streams", s, t.slot);
        if (!F) return fail(err, AACG_ERR_INVALID_ARG, "stream %ld of the batch brings no frame", s);
        if (F > lim.max_frames) return fail(err, AACG_ERR_CAPACITY, "stream %ld of the batch brings %ld frames, the shaped plan was made for %ld", s, F, lim.max_frames);
        if (kept > n || n > 8 || (t.frame_units >> 16)) return fail(err, AACG_ERR_INVALID_ARG, "stream %ld of the batch: %ld elements of %ld kept", s, kept, n);
        if (kept > lim.max_elems) return fail(err, AACG_ERR_CAPACITY, "stream %ld of the batch keeps %ld elements, the shaped plan was made for %ld", s, kept, lim.max_elems);
        if (t.frame_first != frames || t.unit_first != units) return fail(err, AACG_ERR_INVALID_ARG, "stream %ld of the batch: frame_first / unit_first are not the prefix sums", s);
        uint32_t chan = 0;
        for (uint32_t e = 0; e < kept; e++) {
            const uint32_t c = (t.nch >> (2 * e)) & 3u;
            if (c < 1 || c > 2) return fail(err, AACG_ERR_INVALID_ARG, "stream %ld of the batch: element %ld has %ld channels", s, e, c);
            chan += c;
        }
        if (chan > channels) return fail(err, AACG_ERR_INVALID_ARG, "stream %ld of the batch: its kept elements have %ld channels, the engine %ld", s, chan, channels);
        const uint32_t nr = (F + AACG_RUN_W - 1u) / AACG_RUN_W;
        frames += F; units += (uint64_t)F * kept; runs += (uint64_t)nr * kept; links += (uint64_t)(nr - 1u) * kept;
        if (kept) {
            if (chan != channels) zero_fill = true;
            if (F > AACG_RUN_W) long_chains = true;
            pcm_frames = (uint32_t)frames;
        }
    }
    if (units > lim.max_units || runs > lim.max_runs || links > lim.max_links)
        return fail(err, AACG_ERR_CAPACITY, "the batch's %ld units / %ld runs exceed the shaped plan's capacity (%ld units)", (long)units, (long)runs, (long)lim.max_units);
    if (frames * 1024u * channels > UINT32_MAX || frames * Cp > UINT32_MAX - 2u) return fail(err, AACG_ERR_CAPACITY, "the batch's PCM / block offsets do not fit 32 bits");
    /* the host planner's chain order: by slot, then channel (aacg_plan_build's std::map) */
    std::vector<uint32_t> order(n_streams);
    for (uint32_t s = 0; s < n_streams; s++) order[s] = s;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return table[a].slot < table[b].slot; });
    for (uint32_t k = 1; k < n_streams; k++)
        if (table[order[k]].slot == table[order[k - 1]].slot) return fail(err, AACG_ERR_INVALID_ARG, "slot %ld is listed twice in one batch", table[order[k]].slot);

    /* nothing can fail from here on */
    aacg_shape_info info;
    info.n_units = (uint32_t)units; info.n_runs = (uint32_t)runs; info.n_links = (uint32_t)links;
    info.zero_fill = zero_fill; info.long_chains = long_chains;
    info.wide_frames = channels > 2 && units > 0;          /* every unit's frame has `channels` channels: all of them wide, or none */
    info.pcm_floats = (size_t)pcm_frames * 1024u * channels;
    info.chains.reserve((size_t)std::min<uint64_t>(runs, (uint64_t)n_streams * 8u));
    uint32_t run = 0, link = 0;
    for (uint32_t k = 0; k < n_streams; k++) {
        aacg_shape_stream& t = table[order[k]];
        const uint32_t kept = (t.frame_units >> 8) & 0xffu, nr = (t.frames + AACG_RUN_W - 1u) / AACG_RUN_W;
        t.run_first = run; t.link_first = link;
        t.rot = 0;
        for (uint32_t c = 0; c < channels; c++) t.rot |= (uint32_t)((parity ? parity[(size_t)t.slot * channels + c] : 0) & 15u) << (4 * c);
        for (uint32_t e = 0, chan = 0; e < kept; e++) {
            aacg_chain ch;
            ch.stream = t.slot; ch.channel = (uint16_t)chan; ch.n_ch = (uint8_t)((t.nch >> (2 * e)) & 3u);
            for (uint32_t c = 0; c < 2; c++) ch.parity[c] = c < ch.n_ch ? (uint8_t)((t.rot >> (4 * (chan + c))) & 15u) : 0;
            ch.first_run = run; ch.n_runs = nr;
            info.chains.push_back(ch);
            chan += ch.n_ch; run += nr; link += nr - 1u;
        }
    }
    /* plan unit 0: the first listed stream with a layout, its first frame's first element */
    for (uint32_t s = 0; s < n_streams; s++)
        if ((table[s].frame_units >> 8) & 0xffu) { info.unit0_coef = table[s].frame_first * Cp; info.unit0_nch = table[s].nch & 3u; break; }
    *out = std::move(info);
    return AACG_OK;
}

bool aacg_shape_same(const aacg_shape_stream* a, size_t na, const aacg_shape_stream* b, size_t nb)
{
    if (na != nb) return false;
    for (size_t s = 0; s < na; s++) {
        aacg_shape_stream x = a[s], y = b[s];
        x.rot = y.rot = 0;                                 /* the rotation moves on with every launch */
        if (std::memcmp(&x, &y, sizeof x) != 0) return false;
    }
    return true;
}

/* aacg_shape_carry.h: the listing the carry kernel finds a unit's predecessor in */
bool aacg_carry_listing_ok(const aacg_unit_desc* units, size_t n_units, std::string* why)
{
    std::vector<uint32_t> closed;                          /* streams whose stretch has ended */
    size_t i = 0;
    while (i < n_units) {
        const uint32_t stream = units[i].stream;
        if (std::find(closed.begin(), closed.end(), stream) != closed.end())
            return fail(why, 0, "the plan lists stream %ld in more than one stretch (unit %ld): a stream's frames must be consecutive", (long)stream, (long)i) != 0;
        /* the first frame's elements */
        size_t k = 0;
        while (i + k < n_units && units[i + k].stream == stream && units[i + k].pcm_offset == units[i].pcm_offset) k++;
        if (k > 8) return fail(why, 0, "a frame of stream %ld lists %ld units: at most 8", (long)stream, (long)k) != 0;
        size_t j = i + k;
        while (j < n_units && units[j].stream == stream) {    /* every further frame: the same elements in the same order */
            for (size_t e = 0; e < k; e++)
                if (j + e >= n_units || units[j + e].stream != stream || units[j + e].pcm_offset != units[j].pcm_offset ||
                    units[j + e].channel != units[i + e].channel || units[j + e].n_ch != units[i + e].n_ch)
                    return fail(why, 0, "the frames of stream %ld do not list the same elements next to each other (unit %ld)", (long)stream, (long)(j + e)) != 0;
            if (j + k < n_units && units[j + k].stream == stream && units[j + k].pcm_offset == units[j].pcm_offset)
                return fail(why, 0, "a frame of stream %ld lists more units than the stream's first (unit %ld)", (long)stream, (long)(j + k)) != 0;
            j += k;
        }
        closed.push_back(stream);
        i = j;
    }
    return true;
}
