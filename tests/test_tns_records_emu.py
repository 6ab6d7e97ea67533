"""A batch's TNS records made on the device (aacg_tns_records, aac.js_amd/csrc/aacg_tns_prep.h: tns_records_body, and the matrices
kernel behind it) against what the host makes of the same parser outputs (aacg_tns_prepare, aac.js_amd/csrc/aacg_plan.cpp; the
matrices from tns_matrix_row), BYTE FOR BYTE.  The kernels' source runs lane by lane on the CPU (tests/emu/tnsprep_emu.cpp
with tests/emu/devport_emu.h) into a poisoned buffer laid out as aacg_tns_records_bytes lays it out; nothing may be left of the
poison inside it and nothing may be written outside it.

The inputs come from a seeded generator, for every sample index that has band tables (0..11: the TNS limits know a thirteenth, the
engine and aacg_swb_offsets refuse it), and the test asserts of the inputs themselves that they hold what it means to check."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import aacgpu
from resident_kit import NODE, ROOT
from resident_kit import emu_tns as lib          # noqa: F401  (fixture: tests/emu/tnsprep_emu.cpp, built with g++)
from resident_kit import records_layout as layout

POISON = 0xA5
GUARD = 4096                       # poisoned bytes in front of and behind the buffer
SHORT = 2                          # AACG_EIGHT_SHORT_SEQUENCE
# TNS_MAX_BANDS_1024 / _128 (ISO/IEC 14496-3 Table 4.138) and the band counts, to place max_sfb below, at and above the limit
TNS_LONG = [31, 31, 34, 40, 42, 51, 46, 46, 42, 42, 42, 39]
TNS_SHORT = [9, 9, 10, 14, 14, 14, 14, 14, 14, 14, 14, 14]
N_LONG = [41, 41, 47, 49, 49, 51, 47, 47, 43, 43, 43, 40]
N_SHORT = [12, 12, 12, 14, 14, 14, 15, 15, 15, 15, 15, 15]


def coef_tables():
    """tns.js:50-63: -sin(q / iqfac) on a 3- or 4-bit grid, [2 * coef_compress + coef_res]"""
    out = []
    for compress in range(2):
        for res in range(2):
            bits = res + 3
            fields, half = 1 << (bits - compress), 1 << (bits - 1)
            vals = []
            for i in range(fields):
                s = i - fields if i >= fields // 2 else i
                vals.append(np.float32(-math.sin(s / (((half - 0.5) if s >= 0 else (half + 0.5)) / (math.pi / 2.0)))))
            out.append(vals)
    return out


def run(lib, si, units, results, info, max_units, Cp, blocks=None):
    """both makers on the same parser outputs -> (device records, device matrices, host records, host matrices)"""
    F = len(results)
    n = F * Cp
    assert len(units) == F * max_units and len(info) == n
    m_off, total = layout(lib, n)
    host = np.zeros(total, np.uint8)
    assert lib.emu_tns_host(si, units.ctypes.data, results.ctypes.data, info.ctypes.data, F, max_units, Cp, host.ctypes.data) == 0, \
        "aacg_tns_prepare refused a channel: the generator made a record outside the syntax"
    raw = np.full(total + 2 * GUARD + 256, POISON, np.uint8)
    at = (-raw.ctypes.data - GUARD) % 256 + GUARD                  # 256-byte aligned like a device allocation
    dev = raw[at:at + total]
    blocks = -(-n // 64) if blocks is None else blocks
    assert lib.emu_tns_records(si, units.ctypes.data, results.ctypes.data, info.ctypes.data, F, max_units, Cp, blocks, dev.ctypes.data) == 0
    assert (raw[:at] == POISON).all() and (raw[at + total:] == POISON).all(), "the kernels wrote outside the batch's records and matrices"
    d_recs, h_recs = dev[:n * 512].view(aacgpu.DEV_TNS_DTYPE), host[:n * 512].view(aacgpu.DEV_TNS_DTYPE)
    assert (dev[n * 512:m_off] == POISON).all(), "the alignment gap between the records and the matrices belongs to nobody"
    return d_recs, dev[m_off:].view(np.float64).reshape(n, 3, 12, 12), h_recs, host[m_off:].view(np.float64).reshape(n, 3, 12, 12)


def check(lib, si, units, results, info, max_units, Cp, blocks=None):
    d_recs, d_m, h_recs, h_m = run(lib, si, units, results, info, max_units, Cp, blocks)
    for k in range(len(h_recs)):
        assert d_recs[k].tobytes() == h_recs[k].tobytes(), "record %d (frame %d, block %d) differs from aacg_tns_prepare's:\n%s\n%s" % (k, k // Cp, k % Cp, d_recs[k], h_recs[k])
    assert d_m.tobytes() == h_m.tobytes(), "the transition matrices differ from tns_matrix_row's"
    return h_recs


class Tally:
    """what the generated records hold, counted from the host's records and the side info: the conditions on the inputs"""
    def __init__(self):
        self.records = self.nonempty = 0
        self.seen = set()


def random_filter(rng, tables, is_short, n_bands, tally, force_order=None):
    f = np.zeros((), aacgpu.TNS_DTYPE["filt"].base)
    kind = int(rng.integers(0, 6))
    # lengths: short ones, ones that run bottom to 0 (beyond the band count), 0 (top == bottom: size <= 0)
    f["length"] = [int(rng.integers(1, 8)), int(rng.integers(1, n_bands + 1)), n_bands + int(rng.integers(0, 9)), 0, int(rng.integers(1, 4)), int(rng.integers(4, 16))][kind]
    if is_short:
        f["length"] = min(int(f["length"]), 15)                                 # 4-bit field
    else:
        f["length"] = min(int(f["length"]), 63)                                 # 6-bit field
    order = int(rng.integers(0, 8 if is_short else 13)) if force_order is None else force_order
    f["order"] = order
    if order:
        f["direction"] = int(rng.integers(0, 2))
        t = int(rng.integers(0, 4))
        tally.seen.add("table %d" % t)
        f["coef"][:order] = rng.choice(tables[t], order)
        tally.seen.add("direction %d" % int(f["direction"]))
        tally.seen.add(("short order %d" if is_short else "long order %d") % order)
    else:
        tally.seen.add("short order 0" if is_short else "long order 0")
    if int(f["length"]) == 0 and order:
        tally.seen.add("length 0 (size <= 0)")
    return f


def random_info(rng, tables, si, seq, tally):
    """one aacg_tns_info within the syntax (tns.js:68-103): long windows 0..3 filters, eight short windows 0..1 each"""
    info = np.zeros((), aacgpu.TNS_DTYPE)
    if seq == SHORT:
        for w in range(8):
            nf = int(rng.integers(0, 2))
            info["n_filt"][w] = nf
            if nf:
                info["filt"][w] = random_filter(rng, tables, True, N_SHORT[si], tally)
        tally.seen.add("short with %s" % ("filters" if info["n_filt"].any() else "no filter"))
    else:
        nf = int(rng.integers(0, 4))
        info["n_filt"][0] = nf
        gap = nf == 3 and rng.integers(0, 2)                                     # an order-0 filter between two real ones
        for f in range(nf):
            force = (0 if f == 1 else int(rng.integers(1, 13))) if gap else None
            info["filt"][f] = random_filter(rng, tables, False, N_LONG[si], tally, force)
        if gap:
            tally.seen.add("order 0 between two filters")
        total = sum(int(info["filt"][f]["length"]) for f in range(nf))
        if nf and total >= N_LONG[si]:
            tally.seen.add("bottom reaches 0")
        tally.seen.add("long with %d filters" % nf)
    return info


def random_batch(rng, si, n_frames, max_units, Cp, tally, layouts, refuse=()):
    """parser outputs of n_frames frames as aacg_parse_device leaves them for frames that parse — and garbage where it promises
    nothing or nobody may look: a refused frame's records, the element slots beyond a frame's count, the side info of channels
    without AACG_CHAN_TNS_PRESENT"""
    tables = coef_tables()
    units = np.zeros(n_frames * max_units, aacgpu.UNIT_DTYPE)
    results = np.zeros(n_frames, aacgpu.PARSE_RESULT_DTYPE)
    info = np.frombuffer(rng.integers(0, 256, n_frames * Cp * 424, dtype=np.uint8).tobytes(), aacgpu.TNS_DTYPE).copy()
    owners = {}
    for f in range(n_frames):
        lay = layouts[int(rng.integers(0, len(layouts)))]
        assert len(lay) <= max_units and sum(lay) <= Cp
        refused = f in refuse
        chan = 0
        for e in range(max_units):
            u = units[f * max_units + e]
            ghost = e >= len(lay) or refused                        # a slot nobody may read: looks like a unit with TNS on this frame's blocks
            nch = lay[e] if e < len(lay) else int(rng.integers(1, 3))
            block = f * Cp + (chan if e < len(lay) else int(rng.integers(0, Cp)))
            u["n_ch"], u["channel"], u["coef_offset"], u["meta_offset"] = nch, chan, block, block
            any_tns = False
            for c in range(nch):
                seq = int(rng.integers(0, 4))
                limit, bands = (TNS_SHORT[si], N_SHORT[si]) if seq == SHORT else (TNS_LONG[si], N_LONG[si])
                where = int(rng.integers(0, 4))
                max_sfb = [int(rng.integers(0, limit)), limit, int(rng.integers(limit, bands + 1)), bands][where]
                ch = u["ch"][c]
                ch["window_sequence"], ch["max_sfb"], ch["window_shape"] = seq, max_sfb, int(rng.integers(0, 2))
                ch["group_count"], ch["group_len"][0] = 1, 1
                present = ghost or rng.integers(0, 4) != 0
                if nch == 2 and c == 1 and not ghost and rng.integers(0, 3) == 0:
                    present = not (int(u["ch"][0]["flags"]) & aacgpu.CHAN_TNS_PRESENT)      # a CPE with TNS on one channel only
                ch["flags"] = aacgpu.CHAN_TNS_PRESENT if present else 0
                any_tns = any_tns or present
                if present and not ghost:
                    info[block + c] = random_info(rng, tables, si, seq, tally)
                    owners[block + c] = (seq, max_sfb)
                    tally.seen.add("max_sfb %s the limit" % ("below" if max_sfb < limit else "at" if max_sfb == limit else "above"))
            if nch == 2 and not ghost and bool(u["ch"][0]["flags"]) != bool(u["ch"][1]["flags"]):
                tally.seen.add("pair with TNS on one channel")
            u["tns_offset"] = block if any_tns else 0
            if e < len(lay):
                chan += nch
        results[f]["status"] = 8 if refused else 0                  # (a refused frame keeps its counts: they must not be looked at)
        results[f]["n_units"], results[f]["n_channels"] = len(lay), chan
        if len(lay) < max_units and not refused:
            tally.seen.add("fewer units than max_units")
        if refused:
            tally.seen.add("refused frame")
    return units, results, info, owners


def account(tally, recs, owners):
    """every record nobody owns is empty; of the owned ones, count those that end with a filter to run"""
    for k in range(len(recs)):
        if k not in owners:
            assert not recs[k].tobytes().strip(b"\0"), "a record no accepted unit owns is not empty"
            continue
        tally.records += 1
        if recs[k]["order"].any():
            tally.nonempty += 1
            assert (recs[k]["size"][recs[k]["order"] > 0] > 0).all()


WANTED = (["table %d" % t for t in range(4)] + ["direction 0", "direction 1"] + ["long order %d" % o for o in range(13)] + ["short order %d" % o for o in range(8)] +
          ["long with %d filters" % n for n in range(4)] + ["short with filters", "short with no filter", "order 0 between two filters", "bottom reaches 0",
           "length 0 (size <= 0)", "max_sfb below the limit", "max_sfb at the limit", "max_sfb above the limit", "pair with TNS on one channel",
           "fewer units than max_units", "refused frame"])


def test_generated_records_every_sample_index(lib):
    """long windows with 0..3 filters, eight short windows with 0..1 each, orders 0..12 / 0..7 (an order-0 filter between two real
    ones among them), both directions, lengths that run bottom to 0 or leave nothing to filter, max_sfb below / at / above the TNS
    limit, all four coefficient tables; refused frames, frames with fewer units than max_units, pairs with TNS on one channel."""
    assert [len(t) for t in coef_tables()] == [8, 16, 4, 8]
    tally = Tally()
    for si in range(12):
        rng = np.random.default_rng(1000 + si)
        for max_units, Cp, layouts in [(1, 2, [[2]]), (2, 3, [[1], [2], [1, 2], [2, 1]]), (4, 6, [[1, 2, 2, 1], [2], [1, 1]])]:
            F = 23
            refuse = set(int(v) for v in rng.choice(F, 3, replace=False))
            units, results, info, owners = random_batch(rng, si, F, max_units, Cp, tally, layouts, refuse)
            account(tally, check(lib, si, units, results, info, max_units, Cp), owners)
    missing = [w for w in WANTED if w not in tally.seen]
    assert not missing, "the generator never made: %s" % missing
    assert tally.records > 1000 and 3 * tally.nonempty >= tally.records, "too few records end with a filter to run: %d of %d" % (tally.nonempty, tally.records)


def test_fewer_workgroups_than_records(lib):
    """one workgroup, and a count that is no multiple of the workgroup: every record is still written, once"""
    tally = Tally()
    rng = np.random.default_rng(7)
    units, results, info, owners = random_batch(rng, 3, 150, 1, 2, tally, [[2]], refuse={4, 149})
    assert len(info) == 300 and 300 > 64 and 300 % 64
    for blocks in (1, 3, 5, 64):
        account(tally, check(lib, 3, units, results, info, 1, 2, blocks=blocks), owners)
    assert tally.nonempty


def test_beyond_the_syntax_leaves_empty_slots(lib):
    """what the parser never hands over (it refuses the frame: AACG_PARSE_TNS_ORDER) and the host refuses in its turn: an order
    above twelve, more filters than a window may have.  The kernel indexes nothing past twelve and leaves the slots empty, the
    record's other filters are made as ever."""
    tables = coef_tables()
    units = np.zeros(3, aacgpu.UNIT_DTYPE)
    results = np.zeros(3, aacgpu.PARSE_RESULT_DTYPE)
    info = np.zeros(3, aacgpu.TNS_DTYPE)
    for f in range(3):
        units[f]["n_ch"], units[f]["coef_offset"], units[f]["tns_offset"] = 1, f, f
        units[f]["ch"][0]["max_sfb"], units[f]["ch"][0]["flags"], units[f]["ch"][0]["group_count"] = 40, aacgpu.CHAN_TNS_PRESENT, 1
        results[f]["n_units"] = 1
    # frame 0: three long filters, the second of order 200 (its length still moves bottom).  48 kHz has 49 long bands and a TNS
    # limit of 40: the first filter covers bands 34..40, the third 21..28
    info[0]["n_filt"][0] = 3
    for k, (length, order) in enumerate([(15, 4), (6, 200), (7, 3)]):
        info[0]["filt"][k]["length"], info[0]["filt"][k]["order"] = length, order
        info[0]["filt"][k]["coef"][:] = tables[1][3]
    # frame 1: seven filters in a long window; frame 2: short windows, window 2 with two filters and window 5 with an order-9 filter
    info[1]["n_filt"][0] = 7
    info[1]["filt"][0]["length"], info[1]["filt"][0]["order"] = 5, 4
    units[2]["ch"][0]["window_sequence"], units[2]["ch"][0]["max_sfb"] = SHORT, 12
    for w, nf, order in [(1, 1, 5), (2, 2, 5), (5, 1, 9)]:
        info[2]["n_filt"][w] = nf
        info[2]["filt"][w]["length"], info[2]["filt"][w]["order"] = 6, order
        info[2]["filt"][w]["coef"][:] = tables[0][2]
    n = 3
    m_off, total = layout(lib, n)
    raw = np.full(total + 2 * GUARD + 256, POISON, np.uint8)
    at = (-raw.ctypes.data - GUARD) % 256 + GUARD
    assert lib.emu_tns_records(3, units.ctypes.data, results.ctypes.data, info.ctypes.data, 3, 1, 1, 1, raw[at:].ctypes.data) == 0
    assert (raw[:at] == POISON).all() and (raw[at + total:] == POISON).all()
    recs = raw[at:at + n * 512].view(aacgpu.DEV_TNS_DTYPE)
    assert list(recs[0]["order"]) == [4, 0, 3, 0, 0, 0, 0, 0]
    # the same filters with order 0 in the place of the order the syntax does not have, as the host makes them
    one = np.zeros(1, aacgpu.TNS_DTYPE)
    one[0]["n_filt"][0] = 3
    for k, (length, order) in enumerate([(15, 4), (6, 0), (7, 3)]):
        one[0]["filt"][k]["length"], one[0]["filt"][k]["order"] = length, order
        one[0]["filt"][k]["coef"][:] = tables[1][3]
    d, _, h, _ = run(lib, 3, units[:1], results[:1], one, 1, 1)
    assert d[0].tobytes() == h[0].tobytes() == recs[0].tobytes(), "an order beyond twelve must leave what an order-0 filter leaves"
    assert not recs[1].tobytes().strip(b"\0"), "seven filters in a long window: the window's slots stay empty"
    assert list(recs[2]["order"]) == [0, 5, 0, 0, 0, 0, 0, 0]


@pytest.mark.skipif(NODE is None, reason="node not present")
def test_fuzzed_frames_of_the_javascript_front_end(lib, tmp_path):
    """tests/js/parse_cases.js's `fuzz` case (random bytes, valid frames with bits flipped; TNS records wanted): the records and
    results the JavaScript front end makes of it, through the emulated kernel against the host function"""
    out = str(tmp_path)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "parse_cases.js"), out, "standard"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    case = [c for c in json.load(open(os.path.join(out, "manifest.json"))) if c["name"] == "fuzz"][0]
    assert case["wantTns"]
    f = lambda ext, dt: np.fromfile(os.path.join(out, "fuzz" + ext), dt)
    units, results, info = f(".units", aacgpu.UNIT_DTYPE), f(".results", aacgpu.PARSE_RESULT_DTYPE), f(".tns", aacgpu.TNS_DTYPE)
    U, Cp = case["maxUnits"], case["maxChannels"]
    assert len(results) == case["frames"] and len(info) == case["frames"] * Cp
    recs = check(lib, case["sampleIndex"], units, results, info, U, Cp)
    ok = results["status"] == 0
    assert ok.sum() > 50 and (~ok).sum() > 50
    assert sum(1 for k in range(len(recs)) if recs[k]["order"].any()) > 50
