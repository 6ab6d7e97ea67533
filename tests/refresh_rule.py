"""The rule of aacg_units_refresh (aacg_plan_refresh_from_parse / _ex, include/aacgpu.h) stated in numpy, unit by unit, and the made
inputs its tests share (test infrastructure): tests/test_units_refresh_emu.py holds the kernel's source, run lane by lane on CPU
threads, to it byte for byte; tests/test_units_refresh_gpu.py holds the engine to it through the ABI.  Nothing here calls into the
kernel's header.

The rule, for plan unit i.  Without a map src = i and want = 0; with one src = map[i].parsed_index, want = frame_units & 0xff and
listed = (frame_units >> 8) & 0xff, or want where that is 0.  frame = src // max_units, e = src % max_units.
  matches(a, p): n_ch, channel, coef_offset and meta_offset equal, and not (refuse_pns and p.flags & HAS_PNS).
  want == 0: the unit is accepted iff status == 0 and e < n_units and matches(units[i], parsed[src]).
  want > 0:  the frame is accepted iff status == 0 and n_units == want and matches(units[i - e + k], parsed[src - e + k]) for all
             k < listed; results[frame].status becomes PARSE_LAYOUT exactly where it was 0 and the frame is refused.
  accepted:  flags = p.flags; ch = p.ch, both entries, byte for byte, CHAN_TNS_PRESENT cleared unless keep_tns; tns_offset =
             p.tns_offset with keep_tns, else 0; gmap[c], for c < p.n_ch with EIGHT_SHORT, nibble w = the group of window w (at most
             eight windows; windows beyond the sum of the group lengths 0), else 0.
  refused:   flags = 0, tns_offset = 0, gmap = 0, both ch entries zero but group_count = 1 and group_len[0] = 1.
  The counter grows by 1 per refused unit without a map, by 1 per refused frame with one.  Every other byte of a record is the
  input's."""
import numpy as np

import aacgpu

DEV_UNIT_DTYPE = np.dtype([("d", aacgpu.UNIT_DTYPE), ("gmap", "<u4", (2,)), ("cpl_first", "<u4"), ("cpl_n", "<u4")])      # aacg_dev_unit
MAP_DTYPE = aacgpu.REFRESH_MAP_DTYPE                                                                                    # aacg_refresh_map
RESULT_DTYPE = aacgpu.PARSE_RESULT_DTYPE                                                                                # aacg_parse_result
PARSE_LAYOUT = aacgpu.PARSE_LAYOUT
HAS_PNS = aacgpu.UNIT_HAS_PNS
TNS_PRESENT = aacgpu.CHAN_TNS_PRESENT
EIGHT_SHORT = 2
COMPARED = ("n_ch", "channel", "coef_offset", "meta_offset")


def matches(a, p, refuse_pns):
    return all(int(a[k]) == int(p[k]) for k in COMPARED) and not (refuse_pns and int(p["flags"]) & HAS_PNS)


def group_map(chan):
    """nibble w = the group of window w, for the first eight windows the group lengths cover"""
    gmap, w = 0, 0
    for g in range(int(chan["group_count"])):
        for _ in range(int(chan["group_len"][g])):
            if w < 8:
                gmap |= g << (4 * w)
            w += 1
    return gmap & 0xffffffff


def refresh(units, parsed, results, rmap, max_units, refuse_pns, keep_tns):
    """-> (the records, the results, the counter's growth, per unit: accepted?).  units: DEV_UNIT_DTYPE (only the first len(rmap) —
    or, without a map, all — are plan units); parsed: aacgpu.UNIT_DTYPE [frames * max_units]; results: RESULT_DTYPE [frames];
    rmap: MAP_DTYPE or None."""
    out, res = units.copy(), results.copy()
    n = len(units) if rmap is None else len(rmap)
    taken = np.zeros(n, bool)
    refused = 0
    for i in range(n):
        if rmap is None:
            src, want, listed = i, 0, 0
        else:
            src, fu = int(rmap["parsed_index"][i]), int(rmap["frame_units"][i])
            want = fu & 0xff
            listed = (fu >> 8) & 0xff or want
        frame, e = divmod(src, max_units)
        status, n_units = int(results["status"][frame]), int(results["n_units"][frame])
        if want == 0:
            ok = status == 0 and e < n_units and matches(units["d"][i], parsed[src], refuse_pns)
            refused += not ok
        else:
            ok = status == 0 and n_units == want and all(matches(units["d"][i - e + k], parsed[src - e + k], refuse_pns) for k in range(listed))
            if not ok and e == 0:
                refused += 1
                if status == 0:
                    res["status"][frame] = PARSE_LAYOUT
        taken[i] = ok
        d = out["d"][i]
        if ok:
            p = parsed[src]
            d["flags"] = p["flags"]
            d["ch"] = p["ch"]
            if not keep_tns:
                d["ch"]["flags"] &= 0xff ^ TNS_PRESENT
            d["tns_offset"] = p["tns_offset"] if keep_tns else 0
            for c in range(2):
                short = c < int(p["n_ch"]) and int(p["ch"][c]["window_sequence"]) == EIGHT_SHORT
                out["gmap"][i, c] = group_map(p["ch"][c]) if short else 0
        else:
            d["flags"] = 0
            d["tns_offset"] = 0
            d["ch"] = np.zeros((), d["ch"].dtype)
            d["ch"]["group_count"] = 1
            d["ch"]["group_len"][:, 0] = 1
            out["gmap"][i] = 0
    return out, res, refused, taken


# ---- made inputs -------------------------------------------------------------------------------------------------------------
def cuts():
    """all 128 ways to cut eight windows into groups, as lists of group lengths"""
    out = []
    for bits in range(128):
        lens, run = [], 1
        for w in range(7):
            if bits >> w & 1:
                lens.append(run)
                run = 1
            else:
                run += 1
        out.append(lens + [run])
    return out


def poison_parser_part(units, fill=0xA5):
    """what a launch may not rely on: a set is stale memory from an older batch — flags, ch, tns_offset and gmap filled"""
    raw = units.view(np.uint8).reshape(len(units), DEV_UNIT_DTYPE.itemsize)
    D = aacgpu.UNIT_DTYPE.fields
    for first, size in [(D["flags"][1], 1), (D["ch"][1], D["ch"][0].itemsize), (D["tns_offset"][1], 4), (DEV_UNIT_DTYPE.fields["gmap"][1], 8)]:
        raw[:, first:first + size] = fill
    return units


def parsed_frame(rng, frame, layout, max_units, parse_channels, window=None, groups=None):
    """the parser's records of one frame that parses with the elements `layout` (channels per element): max_units records, those
    behind the layout 0xFF.  Every byte the parser may put anything in is random; window: the window sequence (default random),
    groups: the group lengths of an EIGHT_SHORT channel (default a random cut)."""
    recs = np.frombuffer(b"\xff" * (max_units * aacgpu.UNIT_DTYPE.itemsize), aacgpu.UNIT_DTYPE).copy()
    chan = 0
    all_cuts = cuts()
    for e, nch in enumerate(layout):
        u = np.frombuffer(rng.integers(0, 256, aacgpu.UNIT_DTYPE.itemsize, dtype=np.uint8).tobytes(), aacgpu.UNIT_DTYPE).copy()
        u["n_ch"], u["channel"] = nch, chan
        u["coef_offset"] = u["meta_offset"] = frame * parse_channels + chan
        u["flags"] &= 0xff ^ HAS_PNS
        for c in range(2):
            seq = int(rng.integers(0, 4)) if window is None else window
            u["ch"]["window_sequence"][0, c] = seq
            lens = (groups if groups is not None else all_cuts[int(rng.integers(0, 128))]) if seq == EIGHT_SHORT else [1]
            u["ch"]["group_count"][0, c] = len(lens)
            u["ch"]["group_len"][0, c] = 0
            u["ch"]["group_len"][0, c, :len(lens)] = lens
        if int(u["tns_offset"][0]) == 0:
            u["tns_offset"] = 1
        recs[e] = u[0]
        chan += nch
    return recs


def plan_units(rng, parsed, picks, streams, n_out_ch):
    """plan records for the parsed records `picks` (indices into parsed), in that order: the planner's part as the parser's blocks
    say, the other bytes random, the parser's part poisoned"""
    units = np.frombuffer(rng.integers(0, 256, len(picks) * DEV_UNIT_DTYPE.itemsize, dtype=np.uint8).tobytes(), DEV_UNIT_DTYPE).copy()
    for k in COMPARED:
        units["d"][k] = parsed[k][picks]
    units["d"]["stream"] = streams
    units["d"]["n_out_ch"] = n_out_ch
    return poison_parser_part(units)
