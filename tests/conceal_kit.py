"""The rule of the conceal stage (aacg_plan_conceal_refused / aacg_pipeline_set_concealment, include/aacgpu.h) stated in numpy, frame
by frame in a stream's order, and what its tests share (test infrastructure): tests/test_units_conceal_emu.py holds the kernel's source,
run lane by lane on CPU threads, to it byte for byte; tests/test_units_conceal_gpu.py holds the resident route to the host-planned
route over records this rule has rewritten.  Nothing here calls into the kernel's header.

The rule.  Each stream slot holds G, the records of its last good frame, or nothing, and r, the refused frames since G; empty / 0 in
a fresh slot.  A stream's frames of a batch in order; refused iff results[frame].status != 0 after the refresh.
  good:     G := for each kept unit its flags and ch[0..1], for each of its channels the block's 1024 int16 and 120 band words; r := 0.
  refused:  r := min(r + 1, hold + 1); if G exists and r <= hold the frame is concealed: each kept unit takes G's flags and ch[]
            (and the group map derived from them), its channels' blocks G's 1024 values and G's 120 words, the scalefactor field
            (bits 0..8) of every word of band type (bits 12..15) 1..11 lowered by r * fade_steps and kept at 0 or above; the result's
            flags gain PARSE_CONCEALED.  Nothing else of the frame changes.
A stream without kept elements is not touched.  The state's bytes: a batch reads side `parity` of its slot and writes side
`parity ^ 1` — the head (has, r; r is 0 where there is no G), the kept elements' records and, where there is a G, the kept channels'
blocks; no other byte."""
import numpy as np

import aacgpu
import refresh_rule

DEV_UNIT_DTYPE = refresh_rule.DEV_UNIT_DTYPE
RESULT_DTYPE = aacgpu.PARSE_RESULT_DTYPE
STREAM_DTYPE = aacgpu.CONCEAL_STREAM_DTYPE
CHAN_DTYPE = aacgpu.UNIT_DTYPE["ch"].base
CONCEALED = aacgpu.PARSE_CONCEALED
EIGHT_SHORT = refresh_rule.EIGHT_SHORT
HEAD_BYTES, ELEM_BYTES, BLOCK_BYTES = 16, 48, 2048 + 240
ELEMS_AT, BLOCKS_AT = HEAD_BYTES, HEAD_BYTES + 8 * ELEM_BYTES


def side_bytes(Cp):
    return BLOCKS_AT + Cp * BLOCK_BYTES


def nch_word(layout):
    return sum((n & 3) << (2 * e) for e, n in enumerate(layout))


def fade(words, down):
    """120 band words behind `down` steps of fade"""
    w = np.asarray(words, np.uint16).astype(np.int64)
    bt, sf = w >> 12, w & 0x1ff
    coded = (bt >= 1) & (bt <= 11)
    return np.where(coded, (w & ~0x1ff) | np.maximum(sf - down, 0), w).astype(np.uint16)


class State:
    """per slot: G (None, or {"elems": [(flags, ch[2])], "blocks": {channel: (q[1024], words[120])}}), r, and the device's bytes —
    [slot][side][side_bytes(Cp)], poisoned — with the parities and fresh flags the host keeps"""

    def __init__(self, n_slots, Cp, poison=0xA5):
        self.Cp = Cp
        self.G, self.r = [None] * n_slots, [0] * n_slots
        self.parity, self.fresh = [0] * n_slots, [1] * n_slots
        self.bytes = np.full((n_slots, 2, side_bytes(Cp)), poison, np.uint8)

    def reset(self, slot):
        self.G[slot], self.r[slot], self.fresh[slot] = None, 0, 1

    def word(self, slot):
        return self.parity[slot] | (2 if self.fresh[slot] else 0)

    def write_side(self, slot, kept_layout):
        """what a launch leaves in the side it writes"""
        side = self.bytes[slot, self.parity[slot] ^ 1]
        G = self.G[slot]
        side[:HEAD_BYTES].view(np.uint32)[:] = [1 if G else 0, self.r[slot] if G else 0, 0, 0]
        if G is None:
            return
        chan = 0
        for e, nch in enumerate(kept_layout):
            el = side[ELEMS_AT + e * ELEM_BYTES:ELEMS_AT + (e + 1) * ELEM_BYTES]
            el[:16].view(np.uint32)[:] = [G["elems"][e][0], 0, 0, 0]
            el[16:] = np.frombuffer(G["elems"][e][1].tobytes(), np.uint8)
            for k in range(nch):
                b = side[BLOCKS_AT + (chan + k) * BLOCK_BYTES:BLOCKS_AT + (chan + k + 1) * BLOCK_BYTES]
                b[:2048] = G["blocks"][chan + k][0].view(np.uint8)
                b[2048:] = G["blocks"][chan + k][1].view(np.uint8)
            chan += nch


def rule(d, gmap, results, q, meta, streams, S, fade_steps, hold, advance=True):
    """One batch, in place.  d: aacgpu.UNIT_DTYPE records of the plan's units as refreshed; gmap: (n, 2) uint32 or None; results:
    RESULT_DTYPE; q: (blocks, 1024) int16; meta: (blocks, 120) uint16; streams: [dict(frame_first, frames, unit_first, slot, layout: the
    channels of the stream's elements, kept: how many of them are decoded)].  S: a State; advance: the batch is enqueued — its slots'
    state changes sides.  -> the concealed frames' indices."""
    concealed = []
    for t in streams:
        kept = t["kept"]
        if not kept:
            continue
        lay, slot = list(t["layout"])[:kept], t["slot"]
        G, r = (None, 0) if S.fresh[slot] else (S.G[slot], S.r[slot])
        for f in range(t["frames"]):
            i = t["frame_first"] + f
            us = [t["unit_first"] + f * kept + e for e in range(kept)]
            if int(results["status"][i]) == 0:
                G, r, chan = {"elems": [], "blocks": {}}, 0, 0
                for e, u in enumerate(us):
                    G["elems"].append((int(d["flags"][u]), d["ch"][u].copy()))
                    for k in range(lay[e]):
                        G["blocks"][chan + k] = (q[int(d["coef_offset"][u]) + k].copy(), meta[int(d["meta_offset"][u]) + k].copy())
                    chan += lay[e]
                continue
            r = min(r + 1, hold + 1)
            if G is None or r > hold:
                continue
            chan = 0
            for e, u in enumerate(us):
                d["flags"][u] = G["elems"][e][0]
                d["ch"][u] = G["elems"][e][1]
                for k in range(2):
                    short = k < int(d["n_ch"][u]) and int(G["elems"][e][1]["window_sequence"][k]) == EIGHT_SHORT
                    if gmap is not None:
                        gmap[u, k] = refresh_rule.group_map(G["elems"][e][1][k]) if short else 0
                for k in range(lay[e]):
                    q[int(d["coef_offset"][u]) + k] = G["blocks"][chan + k][0]
                    meta[int(d["meta_offset"][u]) + k] = fade(G["blocks"][chan + k][1], r * fade_steps)
                chan += lay[e]
            results["flags"][i] |= CONCEALED
            concealed.append(i)
        S.G[slot], S.r[slot] = G, (r if G else 0)
        S.write_side(slot, lay)
        if advance:
            S.parity[slot] ^= 1
            S.fresh[slot] = 0
    return concealed


def stream_records(streams, S):
    """the launch's per-stream table (aacg_conceal_stream) for the batch, with the slots' sides as S has them"""
    tab = np.zeros(len(streams), STREAM_DTYPE)
    for s, t in enumerate(streams):
        tab[s] = (t["frame_first"], t["frames"], t["unit_first"], len(t["layout"]) | (t["kept"] << 8), t["slot"], nch_word(t["layout"]), S.word(t["slot"]), 0)
    return tab


# ---- truncated table entries: how the GPU and JavaScript tests drop a frame ---------------------------------------------------------
DROP_BYTES = 9


def dropped(table, drops):
    """the frame table with the entries `drops` cut to 9 bytes: an ADTS header and two bytes of a raw_data_block, which end inside
    the first element"""
    out = table.copy()
    out["byte_length"][list(drops)] = DROP_BYTES
    return out


# ---- the host route: parse on the host, the rule over the records, a plan per batch, decode_pipelined --------------------------------
class ConcealRoute:
    """the yardstick of tests/test_units_conceal_gpu.py: aacg_parse_batch -> the plan's units as the refresh leaves them -> rule() ->
    window_shape_prev by the carry's rule (or 0) -> Engine.plan -> decode_pipelined; and the oracle over the same substituted records.
    A stream's layout is its first frame's, which the tests never drop for streams of more than two channels."""

    def __init__(self, S, C_, si, fade_steps, hold, oracle=None, carry=True, options=aacgpu.PARSE_REFERENCE_QUIRKS, conceal=True, i16=False):
        import torch
        import resident_kit as rk
        self.torch, self.rk, self.S, self.C, self.si, self.carry, self.options = torch, rk, S, C_, si, carry, options
        self.fade_steps, self.hold, self.conceal = fade_steps, hold, conceal
        self.U, self.Cp = rk.parse_dims(C_)
        self.parser = aacgpu.Parser(sample_index=si)
        self.i16 = i16
        self.eng = aacgpu.Engine(aacgpu.INPUT_QUANT_I16, max_streams=S, max_channels=C_, sample_index=si,
                                 output_kind=aacgpu.OUTPUT_I16 if i16 else aacgpu.OUTPUT_F32)
        self.oracle, self.ov = oracle, np.zeros((S, C_, 1024), np.float32)
        self.W = np.zeros((S, C_), np.uint8)
        self.state = State(S, self.Cp)
        self.layout = [None] * S
        self.statuses, self.flags, self.refused, self.concealed = [[] for _ in range(S)], [[] for _ in range(S)], 0, 0

    def reset(self, s):
        self.eng.reset_stream(s)
        self.W[s] = 0
        self.ov[s] = 0
        self.state.reset(s)
        if self.C > 2:
            self.layout[s] = None

    def decode(self, data, fr, live, counts):
        torch, rk = self.torch, self.rk
        out = self.parser.parse_batch(data, fr, self.U, self.Cp, self.options, False)
        res = out["results"].copy()
        n, per = len(fr), 1024 * self.C
        first = np.concatenate([[0], np.cumsum(counts)])
        units, streams = [], []
        for k, s in enumerate(live):
            if self.layout[s] is None:
                if self.C <= 2:
                    self.layout[s] = ([self.C], 1)
                else:
                    i = int(first[k])
                    assert int(res["status"][i]) == 0, "the first frame of a stream of more than two channels parses"
                    lay, kept, chan = [], 0, 0
                    for e in range(int(res["n_units"][i])):
                        nch = int(out["units"]["n_ch"][i * self.U + e])
                        lay.append(nch)
                        if chan + nch <= self.C and kept == e:
                            kept = e + 1
                        chan += nch
                    self.layout[s] = (lay, kept)
            lay, kept = self.layout[s]
            streams.append(dict(frame_first=int(first[k]), frames=int(counts[k]), unit_first=len(units), slot=int(s), layout=lay, kept=kept))
            for i in range(first[k], first[k + 1]):
                good = int(res["status"][i]) == 0 and int(res["n_units"][i]) == len(lay) and \
                    all(int(out["units"]["n_ch"][i * self.U + e]) == lay[e] for e in range(len(lay)))
                if not good:
                    self.refused += 1
                    if int(res["status"][i]) == 0:
                        res["status"][i] = aacgpu.PARSE_LAYOUT
                chan = 0
                for e in range(kept):
                    if good:
                        u = out["units"][i * self.U + e].copy()
                        u["tns_offset"] = 0
                        u["ch"]["flags"] &= 0xff ^ aacgpu.CHAN_TNS_PRESENT
                    else:
                        u = np.zeros((), aacgpu.UNIT_DTYPE)
                        u["n_ch"], u["channel"], u["coef_offset"], u["meta_offset"] = lay[e], chan, i * self.Cp + chan, i * self.Cp + chan
                        rk.silent(u)
                    u["stream"], u["n_out_ch"], u["pcm_offset"] = s, self.C, i * per
                    units.append(u)
                    chan += lay[e]
        units = np.array(units, aacgpu.UNIT_DTYPE).reshape(-1)
        q, meta = out["q"].reshape(-1, 1024).copy(), out["meta"].reshape(-1, 120).copy()
        if self.conceal:
            self.concealed += len(rule(units, None, res, q, meta, streams, self.state, self.fade_steps, self.hold))
        # the carry's rule over the records as they now stand
        for t in streams:
            s, (lay, kept) = t["slot"], self.layout[t["slot"]]
            for f in range(t["frames"]):
                for e in range(kept):
                    u = units[t["unit_first"] + f * kept + e:][:1]
                    for c in range(int(u["n_ch"][0])):
                        ch = int(u["channel"][0]) + c
                        u["ch"]["window_shape_prev"][0, c] = self.W[s, ch] if self.carry else 0
                        self.W[s, ch] = u["ch"]["window_shape"][0, c]
        for k, s in enumerate(live):
            self.statuses[s].append(res["status"][first[k]:first[k + 1]].copy())
            self.flags[s].append(res["flags"][first[k]:first[k + 1]].copy())
        plan = self.eng.plan(units)
        d_q, d_meta = torch.from_numpy(q).cuda(), torch.from_numpy(meta.view(np.int16)).cuda()
        d_pcm = torch.zeros(n * per, dtype=torch.int16 if self.i16 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.eng.decode_pipelined(plan, d_q.data_ptr(), d_meta.data_ptr(), d_pcm.data_ptr())
        self.eng.synchronize()
        pcm = d_pcm.cpu().numpy()
        plan.destroy()
        ref = None
        if self.oracle is not None:
            ref = self.oracle.decode_batch(units, q, meta, n * per, self.ov, sample_index=self.si)
        return pcm, ref, res

    def close(self):
        self.eng.close()
        self.parser.close()
