"""The edge workload (test infrastructure): a make_batch() batch's skeleton (streams, layout, frames per stream, PCM positions) with
its side info and coefficients rewritten to the corners of the format at one sample index.  The skeleton decides the route, so a
recipe of tests/test_route_matrix.py takes the same route on this workload as on make_batch's.

Side info, per unit and channel (edge_side_info):
  window sequences    every ordered pair of the four sequences, legal and illegal, follows somewhere in every stream channel
  shapes              all four (window_shape, window_shape_prev) pairs
  CPEs                common windows and split ones (then each channel its own window info, no MS mask)
  max_sfb             0, 1, the table's own top (long and short, from orc.swb_offsets), random values
  groupings           GROUPINGS of aacgpu_workload, [1] * 8 with the top short count (8 x 15 = 120 band records at 15-band rates)
  MS masks            none, per band, all
  intensity           both books (14, 15), with and without the MS bit flipping the sign
  band words          beyond group_count * max_sfb: junk, as random_batch has it (never NOISE)
Coefficients (edge_coeffs): geometric magnitudes everywhere, and in the "seam bands" (codebook bands at a scalefactor 2^-9 below
the others) every q of SEAM in turn, across the live bands of the batch, plus +-8190 in "escape bands" (2^-13 below).  edge_nan() puts |q| = 8191 or -32768 into
chosen frames: the reference's out-of-range IQ_TABLE read, NaN."""
import numpy as np

import aacgpu_workload as W

SAMPLE_INDICES = (0, 2, 3, 4, 5, 6, 8, 11)      # every distinct (long table, short table, TNS_MAX_BANDS) combination
SAME_TABLES = {1: 0, 7: 6, 9: 8, 10: 8}         # the other four indices: the band tables of these
SEAM = np.arange(-520, 521)                     # both seams of the IQ tables in LDS (+-256 eight-wave body, +-512 the others)
ESCAPE = 8190
DEBRUIJN = (0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3)    # cyclic: every ordered pair of window sequences once
CODEBOOKS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11)
SEAM_SF, SF = 212, 248                          # 2^-9 apart: the seam's magnitudes (up to 520^(4/3)) at the level of the rest
ESCAPE_SF = 196                                 # one band per channel 2^-13 below the rest: 8190^(4/3) there is a louder coefficient, not a louder frame


def tables(oracle, si):
    """(long band offsets, short band offsets) of sample index si"""
    return [np.asarray(oracle.swb_offsets(si, is_long), np.int64) for is_long in (True, False)]


def edge_side_info(wl, si, oracle, seed):
    """wl: a make_batch() dict.  Returns (units, meta): copies with the window info and band words rewritten."""
    rng = np.random.default_rng(seed)
    lo, so = tables(oracle, si)
    top = (len(lo) - 1, len(so) - 1)
    units, meta = wl["units"].copy(), np.zeros_like(wl["meta"])
    L = len(units) // wl["n_frames_total"]
    streams = np.unique(units["stream"])
    T = wl["n_frames_total"] // len(streams)
    for i in range(len(units)):
        u = units[i]
        f, e = divmod(i, L)
        s, t = divmod(f, T)
        n_ch = int(u["n_ch"])
        common = n_ch == 2 and (f + e) % 3 != 2
        mask_mode = (f + 2 * s + e) % 3 if common else 0           # 0 none, 1 per band, 2 all
        u["flags"] = (1 if common else 0) | (2 if mask_mode else 0)
        infos = []
        for c in range(n_ch):
            if c == 1 and common:
                infos.append(infos[0])
                continue
            seq = DEBRUIJN[(t + 5 * s + 3 * e + 7 * c) % 16]
            pair = (t + s + 2 * c + e) % 4
            pick = (f + 2 * e + c) % 5
            if e == 0 and pick < 2 and t in (15, T - 1, T // 2):
                pick = 4                                 # frames edge_nan may poison keep live bands in their first element
            elif pick < 2 and t == 0:
                pick = 2                                 # batch 1 follows batch 0's last frame: no silence or single band there
            n = top[seq == 2]
            max_sfb = (0, 1, n, n, int(rng.integers(2, n)))[pick]
            if seq == 2:
                gl = [1] * 8 if pick == 2 or (pick == 3 and t % 2 == 0) else W.GROUPINGS[int(rng.integers(0, len(W.GROUPINGS)))]
            else:
                gl = [1]
            infos.append(dict(seq=seq, shape=pair & 1, prev=pair >> 1, max_sfb=max_sfb, gl=gl))
        for c, inf in enumerate(infos):
            short = inf["seq"] == 2
            ch = u["ch"][c]
            ch["window_sequence"], ch["window_shape"], ch["window_shape_prev"] = inf["seq"], inf["shape"], inf["prev"]
            ch["max_sfb"], ch["group_count"] = inf["max_sfb"], len(inf["gl"])
            ch["group_len"] = 0
            ch["group_len"][:len(inf["gl"])] = inf["gl"]
            nb = len(inf["gl"]) * inf["max_sfb"]
            bt = np.asarray(CODEBOOKS, np.uint16)[rng.integers(0, len(CODEBOOKS), 120)]
            bt = np.where(rng.random(120) < 0.08, 0, bt).astype(np.uint16)
            sf = np.where(rng.random(120) < 0.3, SEAM_SF + rng.integers(-4, 5, 120), SF + rng.integers(-8, 9, 120)).astype(np.uint16)
            if c == 1 and n_ch == 2:
                isb = rng.random(120) < 0.2
                bt = np.where(isb, rng.integers(14, 16, 120), bt).astype(np.uint16)
                sf = np.where(isb, 200 + rng.integers(-16, 17, 120), sf).astype(np.uint16)
            coded = np.nonzero((np.arange(120) < nb) & (bt >= 1) & (bt <= 11))[0]
            if len(coded):
                sf[coded[rng.integers(0, len(coded))]] = ESCAPE_SF
            sf = np.where(np.arange(120) < nb, sf + _boost(ch, lo, so), sf).astype(np.uint16)
            m = sf | (bt << 12)
            if c == 0 and mask_mode:
                used = np.ones(120, bool) if mask_mode == 2 else rng.random(120) < 0.5
                m = m | np.where(used, 0x400, 0).astype(np.uint16)
            m = np.where(np.arange(120) < nb, m, rng.integers(0, 65536, 120) & 0xCFFF).astype(np.uint16)
            meta[int(u["meta_offset"]) + c] = m
        units[i] = u
    return units, meta


def _boost(ch, lo, so):
    """Frames of one or a few bands at about the level of full ones (a quiet block after a loud one carries the loud one's error
    in its first half, at its own scale): scalefactor steps of 2^(1/4) added to every live band, the RMS ~ sqrt(coefficients)"""
    short = int(ch["window_sequence"]) == 2
    width = int((so if short else lo)[int(ch["max_sfb"])]) * (8 if short else 1)
    return int(round(2 * np.log2(1024 / max(width, 4))))


def level_noise(units, meta, si, oracle):
    """The NOISE bands add_pns() made (energy scalefactors at an absolute level) raised by the frame's _boost, like the coded
    bands: a copy of meta"""
    lo, so = tables(oracle, si)
    meta = meta.copy()
    for u in units:
        for c in range(int(u["n_ch"])):
            m = meta[int(u["meta_offset"]) + c]
            nb = int(u["ch"]["group_count"][c]) * int(u["ch"]["max_sfb"][c])
            noise = (np.arange(120) < nb) & (m >> 12 == 13)
            m[noise] += _boost(u["ch"][c], lo, so)
    return meta


def live_positions(u, c, meta_word, lo, so, sf=None):
    """Coefficient positions of channel c of unit u in codebook bands (1..11) below max_sfb; sf: those at scalefactor indices sf
    (a range) only"""
    ch = u["ch"][c]
    off = so if int(ch["window_sequence"]) == 2 else lo
    out, idx, w0 = [], 0, 0
    for g in range(int(ch["group_count"])):
        n_w = int(ch["group_len"][g])
        for sfb in range(int(ch["max_sfb"])):
            word = int(meta_word[idx])
            idx += 1
            if not 1 <= word >> 12 <= 11 or (sf is not None and (word & 0x1FF) - _boost(ch, lo, so) not in sf):
                continue
            for w in range(w0, w0 + n_w):
                out.append(w * 128 + np.arange(off[sfb], off[sfb + 1]))
        w0 += n_w
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def edge_coeffs(units, meta, si, oracle, seed, start=0):
    """Quantised spectra for the side info (units, meta): geometric magnitudes with the seam bands filled from SEAM in turn, from
    position `start` on (consecutive batches continue the sweep), and one 8190 or -8190 (in turn) in the escape band of every fifth block that has one.
    Returns (q, next start)."""
    rng = np.random.default_rng(seed)
    lo, so = tables(oracle, si)
    q = np.zeros((meta.shape[0], 1024), np.int16)
    k = np.arange(1024)
    lam_long, lam_short = 3.0 + 21.0 * np.exp(-k / 300.0), np.tile(3.0 + 21.0 * np.exp(-np.arange(128) * 8 / 300.0), 8)
    at, n_esc = start, 0
    for i, u in enumerate(units):
        for c in range(int(u["n_ch"])):
            blk = int(u["coef_offset"]) + c
            lam = lam_short if int(u["ch"][c]["window_sequence"]) == 2 else lam_long
            mag = np.floor(rng.exponential(1.0, 1024) * lam * 0.5)
            q[blk] = (mag * (rng.integers(0, 2, 1024) * 2 - 1)).astype(np.int16)
            m = meta[int(u["meta_offset"]) + c]
            pos = live_positions(u, c, m, lo, so, range(SEAM_SF - 4, SEAM_SF + 5))
            q[blk, pos] = SEAM[(at + np.arange(len(pos))) % len(SEAM)]
            at += len(pos)
            pos = live_positions(u, c, m, lo, so, (ESCAPE_SF,))
            if len(pos) and blk % 5 == 0:
                q[blk, pos[rng.integers(0, len(pos))]] = ESCAPE if n_esc % 2 else -ESCAPE
                n_esc += 1
    return q, at


def edge_nan(q, units, meta, L, si, oracle, frames):
    """A copy of q with |q| = 8191 or -32768 at one live codebook coefficient of each frame in `frames` (frame index f of the
    skeleton, whose units are f * L .. f * L + L - 1: L elements per frame, coupling elements not yet added)."""
    lo, so = tables(oracle, si)
    q = q.copy()
    for j, f in enumerate(frames):
        for u in units[f * L:(f + 1) * L]:
            hit = False
            for c in range(int(u["n_ch"])):
                pos = live_positions(u, c, meta[int(u["meta_offset"]) + c], lo, so)
                if len(pos):
                    q[int(u["coef_offset"]) + c, pos[len(pos) // 2]] = 8191 if j % 2 == 0 else -32768
                    hit = True
                    break
            if hit:
                break
        else:
            raise AssertionError("frame %d has no live codebook band" % f)
    return q


def covered(units, meta, qs, si, oracle):
    """The q values found at live codebook positions of the batches qs"""
    lo, so = tables(oracle, si)
    seen = set()
    for q in qs:
        for u in units:
            for c in range(int(u["n_ch"])):
                pos = live_positions(u, c, meta[int(u["meta_offset"]) + c], lo, so)
                seen |= set(np.unique(q[int(u["coef_offset"]) + c, pos]).tolist())
    return seen


def stretch_max_sfb(oracle, wl, sample_index, max_long):
    """random_batch's max_sfb (0..49 long, 0..14 short) stretched onto the band counts of sample_index, the first channel of
    each kind (long, short) at the table's top; band words that become live get an escape-coded word (the generator leaves junk there).
    Returns (units, meta) copies."""
    n_long, n_short = len(oracle.swb_offsets(sample_index, True)) - 1, len(oracle.swb_offsets(sample_index, False)) - 1
    assert max_long <= n_long
    units, meta = wl["units"].copy(), wl["meta"].copy()
    topped = set()
    for i in range(len(units)):
        for c in range(int(units[i]["n_ch"])):
            ch = units[i]["ch"][c]
            short = int(ch["window_sequence"]) == 2
            old = int(ch["max_sfb"])
            new = int(round(old * (n_short / 14.0 if short else n_long / 49.0)))
            if short not in topped and not (c == 1 and units[i]["flags"] & 1):    # the first of each kind at the top
                new = n_short if short else n_long
                topped.add(short)
            ch["max_sfb"] = new
            g = int(ch["group_count"])
            m = meta[int(units[i]["meta_offset"]) + c]
            if g * new > g * old:
                m[g * old:g * new] = (11 << 12) | (232 + np.arange(g * new - g * old) % 9)
    tops = [(int(ch["window_sequence"]) == 2, int(ch["max_sfb"])) for u in units for ch in u["ch"][:int(u["n_ch"])]]
    assert (False, n_long) in tops and (True, n_short) in tops, "the stretched batch reaches both tops"
    return units, meta
